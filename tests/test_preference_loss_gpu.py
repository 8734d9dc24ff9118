"""bl_preference_loss_f32 (and the policy loss's backward kernels behind it) against the fp64 specification
training/preference_loss.py, at the smallest shapes that reach every branch: the wave and the workgroup row kernels, ranged
and not, more sequences and more pairs than a wave."""
import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import IGNORE_INDEX
from bridgelang_amd.training.preference_loss import KINDS, SEQ_NORMS, PreferenceLossConfig, preference_loss
from test_policy_loss_gpu import grad_close, scalars_close

pytestmark = pytest.mark.gpu

GUARD = 16            # floats on either side of every output


def make_case(name):
    """→ dict(logits, tgt, pair, ref, group_rows, token_range). Inputs are fp32 values, so spec and kernel read the same."""
    B, gr, n, rng, pair = {"a": (6, 5, 64, (8, 32), [1, -1, 2, 2, -2, 0]),
                           "b": (4, 3, 2048, None, [1, -1, -2, 2]),
                           "c": (4, 3, 1024, (0, 512), [1, -1, -2, 2]),
                           "d": (130, 2, 8, None, None)}[name]
    g = torch.Generator().manual_seed(ord(name))
    rows = B * gr
    first, count = rng or (0, n)
    logits = (torch.randn(rows, n, generator=g) * 2).to(torch.bfloat16).float()
    tgt = first + torch.randint(0, count, (rows,), generator=g)
    keep = torch.rand(rows, generator=g) < 0.7
    keep.view(B, gr)[:, 0] = True                              # every sequence keeps a row
    if name == "a":
        keep[:gr] = torch.tensor([False, False, True, False, False])       # a single valid row
        keep[gr:2 * gr] = True                                             # all five
        tgt[gr], tgt[gr + 1] = first, first + count - 1                    # the ends of the range
    if name == "d":                                             # scattered ids: pair k is sequences k - 1 (chosen) and 129 - (k - 1)
        pair = [b + 1 if b < 65 else -(130 - b) for b in range(130)]
    tgt = torch.where(keep, tgt, torch.tensor(IGNORE_INDEX))
    ref = (-float(np.log(count)) + 0.5 * torch.randn(rows, generator=g)).float()
    return dict(logits=logits, tgt=tgt, pair=np.array(pair, dtype=np.int32), ref=ref, group_rows=gr, token_range=rng)


def guarded(dev, *shape, dtype=torch.float32):
    """A NaN-filled output between two guard regions of 1.0 → (view, check())."""
    numel = int(np.prod(shape))
    buf = torch.ones(numel + 2 * GUARD, dtype=dtype, device=dev)
    buf[GUARD:GUARD + numel] = float("nan")
    return buf[GUARD:GUARD + numel].view(*shape), lambda: bool((buf[:GUARD] == 1).all() and (buf[GUARD + numel:] == 1).all())


def run_kernels(dev, case, cfg, pad=0, cap=None, n_pairs_dev=False, poison=True):
    from bridgelang_amd import train_ops as T
    logits, tgt, pair, ref, gr = case["logits"], case["tgt"], case["pair"], case["ref"], case["group_rows"]
    rows, n = logits.shape
    first, count = cfg.token_range or (0, n)
    L = torch.full((rows, n + pad), float("nan"), device=dev)
    L[:, :n] = logits.to(dev)
    if poison:                                                  # never read: ignored rows, columns outside the range
        L[(tgt == IGNORE_INDEX).to(dev)] = float("nan")
        L[:, :first] = float("inf")
        L[:, first + count:n] = float("nan")
    L = L[:, :n]
    P = int(np.abs(pair).max())
    cap = cap or P
    (rs, rs_ok), (st, st_ok), (ps, ps_ok), (ss, ss_ok) = (guarded(dev, rows, 8), guarded(dev, 8), guarded(dev, cap, 4),
                                                          guarded(dev, rows // gr, 4))
    refd = None if cfg.reference_free else torch.where(tgt == IGNORE_INDEX, torch.tensor(float("nan")), ref).to(dev)
    npd = torch.tensor([P], dtype=torch.int32, device=dev) if n_pairs_dev else None
    T.preference_loss(L, tgt.to(dev), torch.from_numpy(pair).to(dev), refd, rs, st, ps, ss, cfg, group_rows=gr, n_pairs=npd)
    dlb = torch.ones(rows * (n + pad) + 2 * GUARD, dtype=torch.bfloat16, device=dev)
    dl = dlb[GUARD:GUARD + rows * (n + pad)].view(rows, n + pad)[:, :n]
    dl.fill_(float("nan"))
    T.policy_loss_backward(L, tgt.to(dev), rs, st, dl, cfg.backward_config())
    torch.cuda.synchronize()
    assert rs_ok() and st_ok() and ps_ok() and ss_ok() and bool((dlb[:GUARD] == 1).all() and (dlb[-GUARD:] == 1).all())
    if pad:
        assert bool((dlb[GUARD:GUARD + rows * (n + pad)].view(rows, n + pad)[:-1, n:] == 1).all())     # ld > n: the gap is not written
    return rs.cpu().numpy(), st.cpu().numpy(), ps.cpu().numpy(), ss.cpu().numpy(), dl.float().cpu()


def check(dev, case, cfg, **kw):
    logits, tgt, pair, gr = case["logits"].numpy(), case["tgt"].numpy(), case["pair"], case["group_rows"]
    ref = None if cfg.reference_free else case["ref"].numpy()
    want = preference_loss(logits, tgt, pair, ref, cfg, group_rows=gr)
    rs, st, ps, ss, dl = run_kernels(dev, case, cfg, **kw)
    v = want.valid
    P = want.n_pairs
    print(f"[{cfg.kind}/{cfg.seq_norm}] loss {st[0]:.6f} vs {want.loss:.6f}; max |h err| {np.abs(ps[:P, 0] - want.pair_stats[:, 0]).max():.3g}; "
          f"max |logp err| {np.abs(rs[:, 0] - want.logp).max():.3g}")
    assert np.isfinite(rs).all() and np.isfinite(st).all() and np.isfinite(ps).all() and np.isfinite(ss).all()
    scalars_close(rs[:, 0], want.logp, "logp")
    scalars_close(rs[:, 1], want.entropy, "entropy")
    scalars_close(rs[:, 7], want.g, "g")
    assert (rs[:, 2:5] == 0).all() and (rs[~v] == 0).all()
    assert st[1] == P
    scalars_close(st, want.stats, "step statistics")
    scalars_close(ps[:P], want.pair_stats, "pair statistics")
    assert (ps[P:] == 0).all()
    scalars_close(ss, want.seq_stats, "sequence statistics")
    assert np.array_equal(ss[:, 1], want.seq_stats[:, 1])
    grad_close(dl, torch.from_numpy(want.dlogits), "dlogits", 1e-2)
    assert torch.isfinite(dl).all()
    dl = dl.numpy()
    first, count = cfg.token_range or (0, dl.shape[1])
    unpaired = np.repeat(pair == 0, gr)
    assert (dl[~v] == 0).all() and (dl[unpaired] == 0).all() and (dl[:, :first] == 0).all() and (dl[:, first + count:] == 0).all()
    assert np.abs(dl[v & ~unpaired]).max() > 0
    return want, (rs, st, ps, ss, dl)


def config(kind, norm, ref_free=False, **kw):
    base = dict(beta=0.3, kind=kind, seq_norm=norm, reference_free=ref_free, sft_coef=0.2, temperature=0.8,
                label_smoothing=0.1 if kind == "sigmoid" else 0.0, margin=0.0 if kind == "ipo" else 0.25)
    base.update(kw)
    return PreferenceLossConfig(**base)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("norm", SEQ_NORMS)
def test_wave_row_kernel_every_kind_and_norm(dev, kind, norm):
    """(a): 6 sequences of 5 rows, n = 64, range (8, 32); a 2-vs-1 pair, a labelled sequence in no pair, a sequence with
    one valid row and one with all five. ld > n on the way."""
    case = make_case("a")
    cfg = config(kind, norm, token_range=case["token_range"])
    want, _ = check(dev, case, cfg, pad=8)
    n_b = want.seq_stats[:, 1]
    assert n_b[0] == 1 and n_b[1] == 5 and n_b[5] > 0
    if kind == "hinge":
        assert (np.abs(want.pair_stats[:, 0] - 1.0) >= 1e-2).all()


def test_reference_free_and_device_pair_count(dev):
    """(a) without a reference; P from the device scalar with a pair_stats buffer longer than P."""
    case = make_case("a")
    check(dev, case, config("sigmoid", "mean", True, token_range=case["token_range"]), cap=3, n_pairs_dev=True)


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_workgroup_row_kernel_and_many_pairs(dev, name):
    """(b) n = 2048 unranged and (c) n = 1024, range (0, 512): the workgroup row kernel. (d) 130 sequences of 2 rows in 65
    pairs, n = 8: more sequences and more pairs than a wave, a pair's sides far apart."""
    case = make_case(name)
    want, _ = check(dev, case, config("sigmoid", "sum", token_range=case["token_range"]), n_pairs_dev=name == "d")
    assert want.n_pairs == (65 if name == "d" else 2)


def test_second_run_is_bit_identical(dev):
    case = make_case("d")
    cfg = config("sigmoid", "mean")
    a, b = run_kernels(dev, case, cfg), run_kernels(dev, case, cfg)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and torch.equal(a[4], b[4])


def test_ids_beyond_the_pair_count_are_no_pair(dev):
    """An id with |pair[b]| > P is 0 on the device (the host refuses it): with P = 2 from the device scalar, a third pair's
    sequences contribute nothing and get zero gradients."""
    case = make_case("a")
    cfg = config("sigmoid", "sum", token_range=case["token_range"])
    want, (rs0, st0, ps0, ss0, dl0) = check(dev, case, cfg, cap=3, n_pairs_dev=True)
    wild = dict(case, pair=np.array([1, -1, 2, 2, -2, 2 ** 31 - 1], dtype=np.int32))
    from bridgelang_amd import train_ops as T
    rows, n = case["logits"].shape
    L, tg = case["logits"].to(dev), case["tgt"].to(dev)
    rs, st, ps, ss = (torch.full(s, float("nan"), device=dev) for s in ((rows, 8), (8,), (3, 4), (6, 4)))
    for last in (2 ** 31 - 1, -2 ** 31, 3, -3):
        wild["pair"][5] = last
        T.preference_loss(L, tg, torch.from_numpy(wild["pair"]).to(dev), case["ref"].to(dev), rs, st, ps, ss, cfg, group_rows=5,
                          n_pairs=torch.tensor([2], dtype=torch.int32, device=dev))
        assert np.array_equal(st.cpu().numpy(), st0) and np.array_equal(ps.cpu().numpy(), ps0) and np.array_equal(rs.cpu().numpy()[:, 7], rs0[:, 7])


def test_argument_checks(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n, gr = 8, 16, 2
    L = torch.zeros(rows * 32 + 8, device=dev)
    tg = torch.zeros(rows, dtype=torch.int64, device=dev)
    pair = torch.tensor([1, -1, 2, -2], dtype=torch.int32, device=dev)
    rs, st, ps, ss = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(2, 4, device=dev), torch.zeros(4, 4, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    base = dict(logits=L.data_ptr(), ld=16, n=n, targets=tg.data_ptr(), pair=pair.data_ptr(), ref=None, P=2, gr=gr, kind=0, norm=0,
                beta=0.1, eps=0.0, margin=0.0, alpha=0.0, T=1.0, rs=rs.data_ptr(), st=st.data_ptr(), ps=ps.data_ptr(), ss=ss.data_ptr(),
                first=0, count=n)

    def call(**kw):
        a = {**base, **kw}
        return lib.bl_preference_loss_f32(a["logits"], a["ld"], rows, a["n"], a["targets"], -100, a["pair"], a["ref"], a["P"], None,
                                          a["gr"], a["kind"], a["norm"], a["beta"], a["eps"], a["margin"], a["alpha"], a["T"],
                                          a["rs"], a["st"], a["ps"], a["ss"], a["first"], a["count"], s)
    assert call() == _lib.BL_OK
    torch.cuda.synchronize()
    before = [t.clone() for t in (rs, st, ps, ss)]
    for kw in (dict(logits=None), dict(targets=None), dict(pair=None), dict(rs=None), dict(st=None), dict(ps=None), dict(ss=None),
               dict(beta=0.0), dict(beta=-1.0), dict(beta=float("nan")), dict(T=0.0), dict(P=0), dict(P=-1), dict(eps=0.5),
               dict(margin=-1.0), dict(alpha=-1.0)):
        assert call(**kw) == _lib.BL_E_ARG, kw
    for kw in (dict(gr=3), dict(gr=0), dict(n=12, count=12), dict(ld=18), dict(ld=8), dict(first=4), dict(count=12), dict(first=8, count=16),
               dict(count=0), dict(kind=3), dict(kind=-1), dict(norm=2)):
        assert call(**kw) == _lib.BL_E_SHAPE, kw
    assert call(logits=L.data_ptr() + 4) == _lib.BL_E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (rs, st, ps, ss)))          # no launch on a rejection


def test_policy_loss_afterwards_still_matches_its_specification(dev):
    """The row code is shared with bl_policy_loss_f32: a preference-loss call before it leaves it what its own test asks."""
    import test_policy_loss_gpu as TP
    case = make_case("b")
    run_kernels(dev, case, config("sigmoid", "sum"))
    TP.test_kernels_match_specification(dev, 2056, 0.7, 0.01, 0.1, 0)
    case = make_case("a")
    run_kernels(dev, case, config("sigmoid", "sum", token_range=case["token_range"]))
    TP.test_kernels_match_specification(dev, 8, 0.7, 0.01, 0.1, 0)
