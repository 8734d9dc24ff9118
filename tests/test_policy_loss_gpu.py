"""bl_policy_loss_f32 / bl_policy_loss_backward_f32 against their fp64 specification (training/policy_loss.py), against the
cross-entropy kernels where the two losses coincide, and against the sampler's own log-probabilities."""
import ctypes as C

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd.training.policy_loss import IGNORE_INDEX, ROW_STAT_NAMES, PolicyLossConfig, policy_loss

pytestmark = pytest.mark.gpu

ROWS = 24


def grad_close(got, ref, what, tol):
    got, ref = got.float().cpu(), ref.float()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def scalars_close(got, ref, what):
    """The project's bound on loss scalars (test_cross_entropy_backward), per value: 1e-4 of max(|ref|, 1)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.abs(got - ref) > 1e-4 * np.maximum(np.abs(ref), 1.0)
    assert not bad.any(), f"{what}: got {got[bad][:4]} vs {ref[bad][:4]} at {np.argwhere(bad)[:4].ravel()}"


def make_case(n, T, seed):
    """24 rows, a third ignored; targets include 0 and n - 1; a peaked row (+60) and an all-equal row; A of both signs and
    0; q placed for ratios on both clipped sides and inside. All inputs are fp32 values, so spec and kernel read the same."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(ROWS, n, generator=g) * 2).to(torch.bfloat16).float()
    tgt = torch.randint(0, n, (ROWS,), generator=g)
    tgt[1], tgt[2] = 0, n - 1
    tgt[::3] = IGNORE_INDEX
    logits[4] = 0.0
    logits[4, int(tgt[4])] = 60.0                      # peaked on its token
    logits[5] = 0.0
    logits[5, (int(tgt[5]) + 1) % n] = 60.0            # peaked on another token: log π(a) = −60 / T
    logits[7] = 1.25                                   # all equal
    A = torch.randn(ROWS, generator=g)
    A[8] = 0.0
    A[4], A[5] = 1.5, -0.5
    on = policy_loss(logits.numpy(), tgt.numpy(), np.zeros(ROWS), np.zeros(ROWS), cfg=PolicyLossConfig(temperature=T)).logp
    want = np.resize(np.array([0.5, 0.9, 1.0, 1.1, 1.6, 0.7, 1.35]), ROWS)
    q = torch.from_numpy(on - np.log(want)).float()
    ref = torch.from_numpy(on).float() + torch.randn(ROWS, generator=g) * 0.3
    return logits, tgt, A, q, ref


def run_kernels(dev, logits, tgt, A, q, ref, cfg, pad=0, backward=True):
    from bridgelang_amd import train_ops as T
    rows, n = logits.shape
    L = torch.full((rows, n + pad), 3.0, device=dev)
    L[:, :n] = logits.to(dev)
    L = L[:, :n]
    to = lambda t: None if t is None else t.to(dev).contiguous()
    row_stats, stats = torch.full((rows, 8), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    T.policy_loss(L, tgt.to(dev), to(A), to(q), to(ref), row_stats, stats, cfg)
    dl = None
    if backward:
        dl = torch.full((rows, n + pad), 7.0, dtype=torch.bfloat16, device=dev)[:, :n]
        T.policy_loss_backward(L, tgt.to(dev), row_stats, stats, dl, cfg)
    return row_stats.cpu().numpy(), stats.cpu().numpy(), dl


@pytest.mark.parametrize("n,T,ent,klc,pad", [(8, 1.0, 0.0, 0.0, 0), (8, 0.7, 0.01, 0.1, 0),
                                             (2056, 1.0, 0.01, 0.0, 8), (2056, 0.7, 0.0, 0.1, 0),
                                             (32064, 1.0, 0.0, 0.0, 0), (32064, 0.7, 0.01, 0.1, 0)])
def test_kernels_match_specification(dev, n, T, ent, klc, pad):
    cfg = PolicyLossConfig(temperature=T, clip_low=0.2, clip_high=0.25, entropy_coef=ent, kl_coef=klc)
    logits, tgt, A, q, ref = make_case(n, T, seed=n % 97)
    ref = ref if klc else None
    want = policy_loss(logits.numpy(), tgt.numpy(), A.numpy(), q.numpy(), None if ref is None else ref.numpy(), cfg)
    v = want.valid
    r = want.ratio[v]
    assert (np.abs(r - (1 - cfg.clip_low)) >= 1e-3).all() and (np.abs(r - (1 + cfg.clip_high)) >= 1e-3).all()     # no tie within reach
    assert want.clipped.any() and (v & ~want.clipped).any() and (r > 1 + cfg.clip_high).any() and (r < 1 - cfg.clip_low).any()
    assert v.sum() == 16 and (A.numpy()[v] > 0).any() and (A.numpy()[v] < 0).any() and (A.numpy()[v] == 0).any()
    rs, st, dl = run_kernels(dev, logits, tgt, A, q, ref, cfg, pad)
    col = {name: rs[:, i] for i, name in enumerate(ROW_STAT_NAMES)}
    print(f"[n={n} T={T}] loss {st[0]:.6f} vs {want.loss:.6f}; max |logp err| {np.abs(col['logp'] - want.logp).max():.3g}")
    for name, ref_v in (("logp", want.logp), ("entropy", want.entropy), ("ratio", want.ratio), ("row_loss", want.row_loss), ("g", want.g)):
        scalars_close(col[name], ref_v, name)
    assert np.array_equal(col["clipped"], want.clipped.astype(np.float32))
    assert (rs[~v] == 0).all()
    assert st[1] == v.sum()
    scalars_close(st, want.stats, "step statistics")
    grad_close(dl, torch.from_numpy(want.dlogits), "dlogits", 1e-2)
    assert (dl.float().cpu().numpy()[~v] == 0).all()
    assert torch.isfinite(dl.float()).all()


def test_agrees_with_cross_entropy(dev):
    """A ≡ 1, q = the kernel's own logp, T = 1, no bonus terms: the surrogate's gradient is cross-entropy's."""
    from bridgelang_amd import ops, train_ops as T
    n = 32064
    cfg = PolicyLossConfig()
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(ROWS, n, generator=g) * 2).to(torch.bfloat16).float()
    tgt = torch.randint(0, n, (ROWS,), generator=g)
    tgt[::3] = IGNORE_INDEX
    ones, zeros = torch.ones(ROWS), torch.zeros(ROWS)
    rs0, _, _ = run_kernels(dev, logits, tgt, ones, zeros, None, cfg, backward=False)
    q = torch.from_numpy(rs0[:, 0].copy())
    rs, st, dl = run_kernels(dev, logits, tgt, ones, q, None, cfg)
    v = (tgt != IGNORE_INDEX).numpy()
    assert (rs[v, 2] == 1.0).all() and st[5] == 0.0 and st[7] == 1.0 and st[6] == 0.0
    L, Tg = logits.to(dev), tgt.to(dev)
    row_loss, mc = torch.empty(ROWS, device=dev), torch.empty(2, device=dev)
    ops.cross_entropy(L, Tg, row_loss, mc)
    ce = torch.empty(ROWS, n, dtype=torch.bfloat16, device=dev)
    T.cross_entropy_backward(L, Tg, mc, ce)
    grad_close(dl, ce.float().cpu(), "dlogits vs cross_entropy_backward", 1e-2)
    err = np.abs(-rs[:, 0] - row_loss.cpu().numpy()).max()
    print(f"max |−logp − CE row_loss| = {err:.3g}")
    assert err <= 1e-4


def test_agrees_with_the_sampler(dev):
    """Tokens drawn by the sampler's specification at T = 0.7 (temperature only): the kernel's log π equals the sampler's
    log(w / total) within 1 / w_token + 1e-4 — the token's integer weight carries at most half a unit of rounding, the
    kept total at most 16032 / 2^30 relative, the rest is fp32 log-sum-exp error."""
    rows, n, T = 16, 32064, 0.7
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(rows, n, generator=g) * 2).to(torch.bfloat16).float()
    tok, wt = S.sample_rows(logits.numpy(), [T] * rows, [0] * rows, [1.0] * rows, list(range(100, 100 + rows)), 0)
    want = S.logprob(wt)
    assert np.isfinite(want).all()
    cfg = PolicyLossConfig(temperature=T)
    rs, _, _ = run_kernels(dev, logits, torch.from_numpy(tok), torch.ones(rows), torch.zeros(rows), None, cfg, backward=False)
    err = np.abs(rs[:, 0] - want)
    print(f"max |logp − sampler logprob| = {err.max():.3g}; smallest token weight {wt[:, 0].min()}")
    assert (err <= 1.0 / wt[:, 0] + 1e-4).all()


def test_argument_checks(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n = 4, 16
    L = torch.zeros(rows * 32 + 8, device=dev)
    tg = torch.zeros(rows, dtype=torch.int64, device=dev)
    f = torch.zeros(rows, device=dev)
    rs, st = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    dl = torch.zeros(rows * 32 + 8, dtype=torch.bfloat16, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def fwd(ptr, ld, n_, temperature=1.0):
        return lib.bl_policy_loss_f32(ptr, ld, rows, n_, tg.data_ptr(), -100, f.data_ptr(), f.data_ptr(), None, temperature, 0.2, 0.2,
                                      0.0, 0.0, rs.data_ptr(), st.data_ptr(), s)

    def bwd(ptr, ld, n_, dptr, ldd):
        return lib.bl_policy_loss_backward_f32(ptr, ld, rows, n_, tg.data_ptr(), -100, rs.data_ptr(), st.data_ptr(), 1.0, 0.0, dptr, ldd, s)
    assert fwd(L.data_ptr(), 16, n) == _lib.BL_OK
    assert fwd(L.data_ptr(), 16, 12) == _lib.BL_E_SHAPE and fwd(L.data_ptr(), 18, n) == _lib.BL_E_SHAPE
    assert fwd(L.data_ptr() + 4, 16, n) == _lib.BL_E_ALIGN
    assert fwd(None, 16, n) == _lib.BL_E_ARG and fwd(L.data_ptr(), 16, n, temperature=0.0) == _lib.BL_E_ARG
    assert bwd(L.data_ptr(), 16, n, dl.data_ptr(), 16) == _lib.BL_OK
    assert bwd(L.data_ptr(), 16, 12, dl.data_ptr(), 16) == _lib.BL_E_SHAPE and bwd(L.data_ptr(), 18, n, dl.data_ptr(), 16) == _lib.BL_E_SHAPE
    assert bwd(L.data_ptr(), 16, n, dl.data_ptr(), 20) == _lib.BL_E_SHAPE
    assert bwd(L.data_ptr() + 4, 16, n, dl.data_ptr(), 16) == _lib.BL_E_ALIGN and bwd(L.data_ptr(), 16, n, dl.data_ptr() + 2, 16) == _lib.BL_E_ALIGN
    torch.cuda.synchronize()
