"""The four ranged entry points against their specifications (`sampling.py` with `vocab=`, `training/policy_loss.py` with
`token_range`): bl_sample_range_f32 / bl_score_range_f32 bit for bit, bl_policy_loss_range_f32 /
bl_policy_loss_backward_range_f32 to the bounds of tests/test_policy_loss_gpu.py. Everything outside the range is NaN and
+inf in every ranged case: a finite and correct result shows that nothing outside is read. With (0, n) every ranged
entry point equals its unranged twin bit for bit."""
import functools

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd.training.policy_loss import IGNORE_INDEX, ROW_STAT_NAMES, PolicyLossConfig, policy_loss
from test_policy_loss_gpu import grad_close, make_case, scalars_close

pytestmark = pytest.mark.gpu

SAMPLE_SHAPES = [(64, 60, 4), (64, 8, 8), (2056, 1032, 256), (32064, 31744, 256), (32064, 0, 32064)]
POLICY_SHAPES = SAMPLE_SHAPES[1:]
PAD = 8                                                    # the padded leading dimension: ld = n + PAD
GRID = [(T, k, p) for T in (0.5, 1.0, 2.0) for k in (0, 3, 50) for p in (0.5, 0.9, 1.0)]
ROWS = 32
STEPS = (0, 3)


def poisoned(rows, n, first, count, inside):
    """[rows, n + PAD] fp32: `inside` in the range's columns, NaN and +inf alternating everywhere else (padding included)."""
    buf = torch.empty(rows, n + PAD)
    buf[:, 0::2], buf[:, 1::2] = float("nan"), float("inf")
    buf[:, first:first + count] = torch.as_tensor(inside)
    return buf


@functools.lru_cache(maxsize=None)
def sample_case(n, first, count):
    """Rows whose range holds bf16-rounded randn·3 logits with planted ties, settings cycling greedy / temperature only /
    top-k / top-p / both, a seed per row — and the specification's draws at two steps, once."""
    seed = n + first + count
    g = torch.Generator().manual_seed(seed)
    l = (torch.randn(ROWS, count, generator=g) * 3).to(torch.bfloat16).float().numpy()
    T, k, p = (np.array([GRID[r % len(GRID)][c] for r in range(ROWS)]) for c in range(3))
    T[4::9] = 0.0
    for r in range(ROWS):
        if r % 4 == 1 and 0 < k[r] < count:                 # exact ties at the k-th largest value of the range
            l[r, (np.arange(3) * 5 + r) % count] = np.sort(l[r])[-int(k[r])]
        if r % 4 == 2:                                      # coarse logits: the top-p boundary falls among equal weights
            l[r] = np.round(l[r] * 2) / 2
        if r % 4 == 3:                                      # ties at the maximum
            l[r, (np.arange(2) * 3 + r) % count] = l[r].max()
    l[7] = -1.25                                            # an all-equal row
    seeds = np.random.default_rng(seed).integers(-(1 << 63), (1 << 63) - 1, ROWS, dtype=np.int64)
    full = poisoned(ROWS, n, first, count, l)
    T, k, p = T.astype(np.float32), k.astype(np.int32), p.astype(np.float32)
    draws = [S.sample_rows(full.numpy()[:, :n], T, k, p, seeds, t, vocab=(first, count)) for t in STEPS]
    return full, T, k, p, seeds, draws


@pytest.mark.parametrize("n,first,count", SAMPLE_SHAPES)
def test_sampler_and_scorer_equal_the_specification(dev, n, first, count):
    from bridgelang_amd import ops
    full, T, k, p, seeds, draws = sample_case(n, first, count)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    logits, dT, dk, dp, dseed = full.to(dev)[:, :n], d(T), d(k), d(p), d(seeds)
    greedy = T == 0
    for t, (want_ids, want_wt) in zip(STEPS, draws):
        ids = torch.full((ROWS,), -1, dtype=torch.int64, device=dev)
        wt = torch.full((ROWS, 2), -1, dtype=torch.int64, device=dev)
        op = ops.sample(logits, dT, dk, dp, dseed, t, ids, wt, vocab=(first, count))
        assert op.name == "bl_sample_range_f32"
        got_ids, got_wt = ids.cpu().numpy(), wt.cpu().numpy()
        bad = np.flatnonzero((got_ids != want_ids) | (got_wt != want_wt).any(axis=1))
        assert bad.size == 0, (t, [(int(r), float(T[r]), int(k[r]), float(p[r]), int(got_ids[r]), int(want_ids[r]), got_wt[r].tolist(),
                                    want_wt[r].tolist()) for r in bad[:8]])
        assert ((got_ids >= first) & (got_ids < first + count)).all() and (got_wt[greedy] == 1).all()
    assert not np.array_equal(draws[0][0], draws[1][0])                       # two steps, two draws
    # the scorer on the sampler's own draws, with a few tokens moved outside the range, and two report ranges
    tok = draws[1][0].copy()
    moved = np.zeros(ROWS, bool)
    if first > 0:
        tok[2], tok[9], moved[[2, 9]] = first - 1, 0, True
    if first + count < n:
        tok[5], tok[13], moved[[5, 13]] = first + count, n - 1, True          # rows 13 (greedy) and 5 (sampled)
    for rf, rc in ((first, count), (first + 1, min(37, count - 1)), (0, 0)):
        want_wt, want_rw = S.score_rows(full.numpy()[:, :n], T, k, p, tok, rf, rc, vocab=(first, count))
        assert np.array_equal(want_wt[~moved], draws[1][1][~moved]) and (want_wt[moved, 0] == 0).all()
        wt = torch.full((ROWS, 2), -1, dtype=torch.int64, device=dev)
        guard = 16
        flat = torch.full((ROWS * rc + 2 * guard,), -1, dtype=torch.int32, device=dev)
        op = ops.score(logits, dT, dk, dp, d(tok), wt, rf, flat[guard:guard + ROWS * rc].view(ROWS, rc) if rc else None,
                       vocab=(first, count))
        assert op.name == "bl_score_range_f32"
        got = flat.cpu().numpy()
        assert np.array_equal(wt.cpu().numpy(), want_wt), (rf, rc)
        assert (got[:guard] == -1).all() and (got[len(got) - guard:] == -1).all()
        assert np.array_equal(got[guard:len(got) - guard].reshape(ROWS, rc), want_rw), (rf, rc)
        if rc == count:                                                       # the whole policy: its weights sum to the kept total
            assert np.array_equal(want_rw.astype(np.int64).sum(-1), want_wt[:, 1])


@pytest.mark.parametrize("n", [64, 2056, 32064])
def test_full_range_equals_the_unranged_entry_points(dev, n):
    from bridgelang_amd import ops
    full, T, k, p, seeds, _ = sample_case(n, 0, n)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    logits, dT, dk, dp, dseed = full.to(dev)[:, :n], d(T), d(k), d(p), d(seeds)
    out = []
    for vocab in (None, (0, n)):
        ids, wt = torch.full((ROWS,), -1, dtype=torch.int64, device=dev), torch.full((ROWS, 2), -1, dtype=torch.int64, device=dev)
        op = ops.sample(logits, dT, dk, dp, dseed, 3, ids, wt, vocab=vocab)
        swt, rw = torch.full((ROWS, 2), -1, dtype=torch.int64, device=dev), torch.full((ROWS, 24), -1, dtype=torch.int32, device=dev)
        op2 = ops.score(logits, dT, dk, dp, ids, swt, 5, rw, vocab=vocab)
        assert (op.name, op2.name) == (("bl_sample_f32", "bl_score_f32") if vocab is None else ("bl_sample_range_f32", "bl_score_range_f32"))
        out.append((ids, wt, swt, rw))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert torch.equal(out[0][1], out[0][2])                                  # and the scorer returns the sampler's pairs


def test_sample_and_score_argument_checks(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n = 2, 64
    z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=dev)
    L, f, ki, i64, wt, rw = z(torch.float32, rows * n + 4), z(torch.float32, rows), z(torch.int32, rows), z(torch.int64, rows), \
        z(torch.int64, rows, 2), z(torch.int32, rows * 8 + 1)
    s = torch.cuda.current_stream().cuda_stream

    def sample(first, count, ptr=L.data_ptr(), n_=n, ids=i64.data_ptr()):
        return lib.bl_sample_range_f32(ptr, n, rows, n_, f.data_ptr(), ki.data_ptr(), f.data_ptr(), i64.data_ptr(), 0, ids, wt.data_ptr(),
                                       first, count, s)

    def score(first, count, rf=0, rc=0, ptr=L.data_ptr(), rwp=rw.data_ptr()):
        return lib.bl_score_range_f32(ptr, n, rows, n, f.data_ptr(), ki.data_ptr(), f.data_ptr(), i64.data_ptr(), wt.data_ptr(), rf, rc,
                                      rwp, first, count, s)
    assert sample(8, 8) == _lib.BL_OK and sample(60, 4) == _lib.BL_OK and sample(0, n) == _lib.BL_OK
    for first, count in ((6, 8), (8, 6), (60, 8), (64, 4), (-4, 8), (8, 0), (8, -4)):      # misaligned, past n, empty
        assert sample(first, count) == _lib.BL_E_SHAPE and score(first, count) == _lib.BL_E_SHAPE, (first, count)
    assert sample(8, 8, n_=4) == _lib.BL_E_SHAPE and sample(8, 8, n_=0) == _lib.BL_E_SHAPE       # the range leaves a shorter row
    assert sample(8, 8, ptr=None) == _lib.BL_E_ARG and sample(8, 8, ids=None) == _lib.BL_E_ARG
    assert sample(8, 8, ptr=L.data_ptr() + 4) == _lib.BL_E_ALIGN and sample(8, 8, ids=i64.data_ptr() + 4) == _lib.BL_E_ALIGN
    assert score(8, 8) == _lib.BL_OK and score(8, 8, 8, 8) == _lib.BL_OK and score(8, 8, 9, 7) == _lib.BL_OK
    for rf, rc in ((7, 2), (15, 2), (0, 4), (8, 9), (40, 4)):                               # a report range that leaves the vocabulary range
        assert score(8, 8, rf, rc) == _lib.BL_E_SHAPE, (rf, rc)
    assert score(8, 8, 8, 4, rwp=None) == _lib.BL_E_ARG and score(8, 8, ptr=None) == _lib.BL_E_ARG
    assert score(8, 8, ptr=L.data_ptr() + 4) == _lib.BL_E_ALIGN and score(8, 8, 8, 4, rwp=rw.data_ptr() + 2) == _lib.BL_E_ALIGN
    torch.cuda.synchronize()


# ---- the policy loss ---------------------------------------------------------------------------------------------------------
P_ROWS = 23                                                # not a multiple of the four rows a workgroup of the wave kernel takes


@functools.lru_cache(maxsize=None)
def policy_case(n, first, count, T):
    """`make_case` on the range (peaked row, all-equal row, advantages of both signs and 0, ratios on both clipped sides),
    embedded into poisoned full rows with the targets in full-row numbering."""
    logits, tgt, A, q, ref = (x[:P_ROWS] for x in make_case(count, T, seed=(n + first) % 97))
    full = poisoned(P_ROWS, n, first, count, logits)
    return full, torch.where(tgt != IGNORE_INDEX, tgt + first, tgt), A, q, ref


def run_policy(dev, full, n, tgt, A, q, ref, cfg, backward=True):
    from bridgelang_amd import train_ops as T
    rows = full.shape[0]
    L = full.to(dev)[:, :n]
    to = lambda t: None if t is None else t.to(dev).contiguous()
    row_stats, stats = torch.full((rows, 8), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    op = T.policy_loss(L, tgt.to(dev), to(A), to(q), to(ref), row_stats, stats, cfg)
    names, base = [op.name], None
    if backward:
        base = torch.full((rows, n + PAD), 7.0, dtype=torch.bfloat16, device=dev)
        names.append(T.policy_loss_backward(L, tgt.to(dev), row_stats, stats, base[:, :n], cfg).name)
    return row_stats.cpu().numpy(), stats.cpu().numpy(), base, names


@pytest.mark.parametrize("n,first,count", POLICY_SHAPES)
@pytest.mark.parametrize("T,ent,klc", [(1.0, 0.0, 0.0), (0.7, 0.01, 0.1)])
def test_policy_kernels_match_specification(dev, n, first, count, T, ent, klc):
    cfg = PolicyLossConfig(temperature=T, clip_low=0.2, clip_high=0.25, entropy_coef=ent, kl_coef=klc, token_range=(first, count))
    full, tgt, A, q, ref = policy_case(n, first, count, T)
    ref = ref if klc else None
    want = policy_loss(full.numpy()[:, :n], tgt.numpy(), A.numpy(), q.numpy(), None if ref is None else ref.numpy(), cfg)
    v = want.valid
    r = want.ratio[v]
    assert (np.abs(r - (1 - cfg.clip_low)) >= 1e-3).all() and (np.abs(r - (1 + cfg.clip_high)) >= 1e-3).all()     # no tie within reach
    assert want.clipped.any() and (v & ~want.clipped).any() and (r > 1 + cfg.clip_high).any() and (r < 1 - cfg.clip_low).any()
    assert v.sum() == 15 and (A.numpy()[v] > 0).any() and (A.numpy()[v] < 0).any() and (A.numpy()[v] == 0).any()
    rs, st, base, names = run_policy(dev, full, n, tgt, A, q, ref, cfg)
    assert names == ["bl_policy_loss_range_f32", "bl_policy_loss_backward_range_f32"]
    col = {name: rs[:, i] for i, name in enumerate(ROW_STAT_NAMES)}
    print(f"[n={n} range=({first}, {count}) T={T}] loss {st[0]:.6f} vs {want.loss:.6f}; max |logp err| {np.abs(col['logp'] - want.logp).max():.3g}")
    for name, ref_v in (("logp", want.logp), ("entropy", want.entropy), ("ratio", want.ratio), ("row_loss", want.row_loss), ("g", want.g)):
        scalars_close(col[name], ref_v, name)
    assert np.array_equal(col["clipped"], want.clipped.astype(np.float32))
    assert (rs[~v] == 0).all() and st[1] == v.sum()
    scalars_close(st, want.stats, "step statistics")
    dl = base.float().cpu()
    assert (dl[:, n:] == 7.0).all()                                           # the padding columns beyond n: untouched
    dl = dl[:, :n]
    assert torch.isfinite(dl).all()
    grad_close(dl, torch.from_numpy(want.dlogits), "dlogits", 1e-2)
    outside = np.ones(n, bool)
    outside[first:first + count] = False
    assert (dl.numpy()[:, outside] == 0).all() and (dl.numpy()[~v] == 0).all()
    assert (dl.numpy()[v][:, ~outside] != 0).any()


@pytest.mark.parametrize("n", [64, 2056, 32064])
def test_policy_full_range_equals_the_unranged_kernels(dev, n):
    """n = 64 takes the wave-per-row forward on the ranged side and the workgroup kernel on the unranged one."""
    base = dict(temperature=0.7, clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.1)
    full, tgt, A, q, ref = policy_case(n, 0, n, 0.7)
    out = []
    for cfg in (PolicyLossConfig(**base), PolicyLossConfig(token_range=(0, n), **base)):
        rs, st, dl, names = run_policy(dev, full, n, tgt, A, q, ref, cfg)
        assert all(("_range_" in name) == (cfg.token_range is not None) for name in names)
        out.append((rs, st, dl.cpu().view(torch.int16).numpy()))
    for a, b, what in zip(*out, ("row statistics", "step statistics", "dlogits")):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b), what


def test_policy_agrees_with_the_ranged_sampler(dev):
    """Tokens the restricted sampler draws at T = 0.7: the ranged kernel's log π equals the sampler's log(w / total) within
    1 / w_token + 1e-4 (the bound of test_policy_loss_gpu.py: half a unit of rounding on the token's weight, the rest is
    fp32 log-sum-exp error). The unranged loss on the same rows is a different distribution altogether."""
    rows, n, T = 16, 32064, 0.7
    first, count = 31744, 256
    g = torch.Generator().manual_seed(11)
    inside = (torch.randn(rows, count, generator=g) * 2).to(torch.bfloat16).float()
    full = poisoned(rows, n, first, count, inside)
    tok, wt = S.sample_rows(full.numpy()[:, :n], [T] * rows, [0] * rows, [1.0] * rows, list(range(100, 100 + rows)), 0, vocab=(first, count))
    want = S.logprob(wt)
    assert np.isfinite(want).all()
    cfg = PolicyLossConfig(temperature=T, token_range=(first, count))
    rs, _, _, _ = run_policy(dev, full, n, torch.from_numpy(tok), torch.ones(rows), torch.zeros(rows), None, cfg, backward=False)
    err = np.abs(rs[:, 0] - want)
    print(f"max |logp − ranged sampler logprob| = {err.max():.3g}; smallest token weight {wt[:, 0].min()}")
    assert (err <= 1.0 / wt[:, 0] + 1e-4).all()


def test_policy_argument_checks_and_targets_outside(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n = 4, 64
    L = torch.zeros(rows * n + 8, device=dev)
    tg = torch.full((rows,), 20, dtype=torch.int64, device=dev)
    f = torch.zeros(rows, device=dev)
    rs, st = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    dl = torch.zeros(rows * n + 8, dtype=torch.bfloat16, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def fwd(first, count, ptr=L.data_ptr(), n_=n, temperature=1.0):
        return lib.bl_policy_loss_range_f32(ptr, n, rows, n_, tg.data_ptr(), -100, f.data_ptr(), f.data_ptr(), None, temperature, 0.2, 0.2,
                                            0.0, 0.0, rs.data_ptr(), st.data_ptr(), first, count, s)

    def bwd(first, count, ptr=L.data_ptr(), dptr=dl.data_ptr(), ldd=n):
        return lib.bl_policy_loss_backward_range_f32(ptr, n, rows, n, tg.data_ptr(), -100, rs.data_ptr(), st.data_ptr(), 1.0, 0.0, dptr, ldd,
                                                     first, count, s)
    assert fwd(16, 8) == _lib.BL_OK and bwd(16, 8) == _lib.BL_OK and fwd(0, n) == _lib.BL_OK and bwd(0, n) == _lib.BL_OK
    for first, count in ((12, 8), (16, 12), (60, 8), (64, 8), (-8, 16), (16, 0), (16, -8)):
        assert fwd(first, count) == _lib.BL_E_SHAPE and bwd(first, count) == _lib.BL_E_SHAPE, (first, count)
    assert fwd(16, 8, n_=60) == _lib.BL_E_SHAPE and bwd(16, 8, ldd=n + 4) == _lib.BL_E_SHAPE
    assert fwd(16, 8, ptr=None) == _lib.BL_E_ARG and fwd(16, 8, temperature=0.0) == _lib.BL_E_ARG and bwd(16, 8, dptr=None) == _lib.BL_E_ARG
    assert fwd(16, 8, ptr=L.data_ptr() + 4) == _lib.BL_E_ALIGN and bwd(16, 8, dptr=dl.data_ptr() + 2) == _lib.BL_E_ALIGN
    # a valid target outside the range: NaN in that row's statistics (never a stray read), the other rows unharmed
    tg[1], tg[2] = 15, 24
    assert fwd(16, 8) == _lib.BL_OK
    got = rs.cpu().numpy()
    assert np.isnan(got[1, 0]) and np.isnan(got[2, 0]) and np.isfinite(got[[0, 3]]).all()
    assert got[0, 0] == pytest.approx(-np.log(8.0), abs=1e-6)                 # uniform over the 8 tokens of the range
