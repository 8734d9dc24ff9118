"""The distillation loss kernels (csrc/distill.hip) per element against the fp64 specification and the derived bounds of
tests/distill_ref64.py, at the smallest shapes at which each form can still go wrong. The cases are distill_ref64.cases();
tests/test_distill_loss_cpu.py shows on the same cases that an fp32 evaluation stays inside every bound.

Scaffolding as tests/test_policy_ref_gpu.py: every buffer is a glue_ref.Flat between NaN guards; logits [rows, ld], teacher
[rows, ldt] and dlogits [rows, ldd] are blocks whose logical part is the first n / count / n columns. dlogits starts as NaN
and must come back fully written. Every case runs twice, with finite filler and with NaN in everything the header calls never
read (logits outside the range, logits and teacher of ignored rows, the row padding of both): the two runs' allocations must
agree bit for bit.

Form → case
  distill_rows_wave_kernel   count 8, 256 x the three kinds; 37 rows leave the last workgroup of four part empty
  distill_rows_kernel        count 264 (the first size), 1032 (a thread loops twice) x the three kinds
  the range                  at column 0, ending at n, strictly inside, and the unranged (0, n)
  the teacher                dense (one row of mass 1 + 5e-4), exact zeros, one-hot, the student's own softmax (D and dlogits
                             inside their bounds round 0), against a student whose tail underflows; ignored rows between valid
                             ones; every row ignored (all outputs exactly 0)
  wave form == workgroup form on <= 256 columns: NOT asserted. The wave kernel is written to add the same numbers in the same
      order (distill.hip's header), but only the wave form is reachable through the entry point at those sizes, so there is
      nothing to compare it with; what is asserted is that it meets the same per-element bounds.
  determinism                two calls, bit-identical                                            test_two_calls_are_bit_identical
  rejections                 every code, outputs untouched                                      test_argument_checks
"""
import numpy as np
import pytest
import torch

import distill_ref64 as D64
import glue_ref as G
import policy_ref64 as P64
from glue_ref import Flat
from policy_ref64 import IGN
from test_distill_loss_cpu import CASES, ref_of

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
NAN = float("nan")
NAMES = ("logp", "entropy", "divergence", "row_loss", "agree", "m", "log_s", "c")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def run(dev, c, poison):
    from bridgelang_amd import train_ops as T
    rows, n = c.logits.shape
    first, count = c.cfg.token_range or (0, n)
    fill = NAN if poison else 3.0
    ign = torch.from_numpy(c.tgt == IGN)
    lb = torch.full((rows, n + c.pad), fill, dtype=f32)
    lb[:, first:first + count] = torch.from_numpy(c.logits[:, first:first + count])
    lb[ign] = fill
    tb = torch.full((rows, count + c.tpad), NAN if poison else 0.25, dtype=f32)
    tb[:, :count] = torch.from_numpy(c.teacher)
    tb[ign] = NAN if poison else 0.25
    L, Q = Flat((rows, n + c.pad), dev, f32, data=lb), Flat((rows, count + c.tpad), dev, f32, data=tb)
    tgt = torch.from_numpy(c.tgt).to(dev)
    out = dict(rs=Flat((rows, 8), dev, f32), st=Flat((8,), dev, f32), dl=Flat((rows, n + c.dpad), dev, bf16))
    T.distill_loss(L.v[:, :n], tgt, Q.v[:, :count], out["rs"].v, out["st"].v, c.cfg)
    T.distill_loss_backward(L.v[:, :n], tgt, Q.v[:, :count], out["rs"].v, out["st"].v, out["dl"].v[:, :n], c.cfg)
    torch.cuda.synchronize()
    for k, x in (("logits", L), ("teacher", Q)):         # the inputs are inputs
        G.assert_bits(x, Flat(x.shape, "cpu", f32, data=lb if k == "logits" else tb), f"{c.name}: {k} was written")
    return out


def host(x):
    return x.v.detach().float().cpu().numpy().astype(np.float64)


def outputs(out, n):
    rs = host(out["rs"])
    got = {name: rs[:, i] for i, name in enumerate(NAMES)}
    got["stats"] = host(out["st"])
    got["dlogits"] = host(out["dl"])[:, :n]
    return got


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_distill_kernels(dev, c):
    ref, _ = ref_of(c)
    n = c.logits.shape[1]
    clean, poisoned = run(dev, c, False), run(dev, c, True)
    for k, x in poisoned.items():
        P64.window_intact(x, n if k == "dl" else x.shape[-1], f"{c.name} {k}")
    got = outputs(poisoned, n)
    P64.check(got, ref, c.name, tag="distill ")
    for k in clean:
        G.assert_bits(clean[k], poisoned[k], f"{c.name} {k}: NaN in what is never read changed the output")
    v = c.tgt != IGN
    first, count = c.cfg.token_range or (0, n)
    dl_bits = G.bits(poisoned["dl"].v[:, :n].detach().cpu()).numpy()
    outside = np.ones((len(v), n), dtype=bool)
    outside[np.ix_(v, np.arange(first, first + count))] = False
    assert (dl_bits[outside] == 0).all(), "dlogits outside the range or on an ignored row is not +0"
    assert (G.bits(poisoned["rs"].v.detach().cpu()).numpy()[~v] == 0).all()
    if not v.any():
        assert (G.bits(poisoned["st"].v.detach().cpu()).numpy() == 0).all()
    else:
        assert got["stats"][1] == v.sum() and np.abs(got["dlogits"][v]).max() > 0


def test_two_calls_are_bit_identical(dev):
    for c in (c for c in CASES if "-rows37-" in c.name):
        a, b = run(dev, c, True), run(dev, c, True)
        for k in a:
            G.assert_bits(a[k], b[k], f"{c.name} {k}: two calls differ")


def test_argument_checks(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n = 4, 32
    L, Q = torch.zeros(rows * 32 + 8, device=dev), torch.full((rows * 16 + 8,), 1.0 / 16, device=dev)
    tg = torch.full((rows,), 9, dtype=torch.int64, device=dev)
    rs, st = torch.full((rows, 8), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    dl = torch.full((rows * 32 + 16,), 7.0, dtype=bf16, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    base = dict(logits=L.data_ptr(), ld=32, n=n, targets=tg.data_ptr(), teacher=Q.data_ptr(), ldt=16, kind=2, beta=0.5, sft=0.0, T=1.0,
                rs=rs.data_ptr(), st=st.data_ptr(), dl=dl.data_ptr(), ldd=32, first=8, count=16)

    def fwd(**kw):
        a = {**base, **kw}
        return lib.bl_distill_loss_f32(a["logits"], a["ld"], rows, a["n"], a["targets"], -100, a["teacher"], a["ldt"], a["kind"], a["beta"],
                                       a["sft"], a["T"], a["rs"], a["st"], a["first"], a["count"], s)

    def bwd(**kw):
        a = {**base, **kw}
        return lib.bl_distill_loss_backward_f32(a["logits"], a["ld"], rows, a["n"], a["targets"], -100, a["teacher"], a["ldt"], a["rs"],
                                                a["st"], a["kind"], a["beta"], a["sft"], a["T"], a["dl"], a["ldd"], a["first"], a["count"], s)
    arg = [dict(logits=None), dict(targets=None), dict(teacher=None), dict(rs=None), dict(st=None), dict(kind=3), dict(kind=-1),
           dict(beta=0.0), dict(beta=1.0), dict(beta=float("nan")), dict(T=0.0), dict(T=float("nan")), dict(sft=-0.5), dict(sft=float("nan"))]
    shape = [dict(first=4), dict(count=12), dict(first=24, count=16), dict(count=0), dict(n=28), dict(ld=34), dict(ld=24), dict(ldt=8),
             dict(ldt=18)]
    align = [dict(logits=L.data_ptr() + 4), dict(teacher=Q.data_ptr() + 4)]
    for call, more in ((fwd, ([], [], [])), (bwd, ([dict(dl=None)], [dict(ldd=36), dict(ldd=24)], [dict(dl=dl.data_ptr() + 2)]))):
        for kws, code in ((arg + more[0], _lib.BL_E_ARG), (shape + more[1], _lib.BL_E_SHAPE), (align + more[2], _lib.BL_E_ALIGN)):
            for kw in kws:
                assert call(**kw) == code, (call.__name__, kw)
    assert fwd(kind=0, beta=float("nan")) == _lib.BL_OK  # beta is jsd's alone
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all())                       # no launch on a rejection; the accepted forward wrote its two outputs
    assert not bool((rs == 7.0).any()) and not bool((st == 7.0).any())
    rs.fill_(7.0), st.fill_(7.0)
    for kw in arg[:1] + shape[:1] + align[:1]:
        fwd(**kw)
    torch.cuda.synchronize()
    assert bool((rs == 7.0).all()) and bool((st == 7.0).all())


def test_report_largest_ratios():
    """Not a check of its own: prints the largest err / bound per output that the tests above recorded (each was <= 1)."""
    for k in sorted(k for k in P64.RATIOS if k.startswith("distill ")):
        print(f"distill_ref64: {k}: largest err/bound {P64.RATIOS[k]:.4f}")
    assert all(v <= 1.0 for k, v in P64.RATIOS.items() if k.startswith("distill "))
