"""bl_policy_loss_is_f32 (the policy loss with the rollout correction: a truncated importance weight between the proximal
policy and the one that drew the tokens) against its fp64 specification (training/policy_loss.py with rollout_is_cap) at
both ratio levels and in both proximal modes; against the uncorrected kernels, bit for bit, where the weight is 1; and its
determinism and argument checks. Bounds are those of tests/test_action_ratio_gpu.py (helpers copied, not imported)."""
import functools

import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import (GROUP_STAT_NAMES, IGNORE_INDEX, IS_STAT_NAMES, ROW_STAT_NAMES, PolicyLossConfig,
                                                 policy_loss)

pytestmark = pytest.mark.gpu

PAD = 8                                                    # the padded leading dimension: ld = n + PAD
# (group_rows, valid rows per sequence). "24" is the token-level case: 24 rows, 16 of them valid at scattered positions.
# The action-level layouts: five sequences in two workgroups of the group kernel, and sequences longer than a wave so that
# lanes stride — three of those, so that a truncated, a masked and an untouched action all occur.
CASES = {"24": (24, (16,)), "5x24": (24, (0, 1, 2, 7, 23)), "3x96": (96, (70, 3, 40))}
# per unit (a valid row at token level, a sequence at action level), in turn: π_θ/π_prox wanted and π_prox/μ wanted. With
# cap 1.5 and mask (0.5, 3): untouched, masked above (truncated without mask), truncated, untouched, masked below
RATIOS, RHOS = (1.0, 0.5, 1.6, 1.1, 0.7), (1.2, 4.0, 2.0, 0.8, 0.3)
CAP, MASK = 1.5, (0.5, 3.0)
LEVELS = [("24", "token", "sum"), ("5x24", "action", "sum"), ("5x24", "action", "mean"), ("3x96", "action", "sum"),
          ("3x96", "action", "mean")]
SHAPES = [(8, None), (2056, None), (2056, (1792, 256)), (2056, (1792, 264))]      # the last two: wave / workgroup row kernel
CLIP = dict(clip_low=0.2, clip_high=0.25)


def grad_close(got, ref, what, tol):
    got, ref = got.float().cpu(), ref.float()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def scalars_close(got, ref, what):
    """The project's bound on loss scalars, per value: 1e-4 of max(|ref|, 1)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.abs(got - ref) > 1e-4 * np.maximum(np.abs(ref), 1.0)
    assert not bad.any(), f"{what}: got {got[bad][:4]} vs {ref[bad][:4]} at {np.argwhere(bad)[:4].ravel()}"


def poisoned(shape, dtype=torch.float32, dev="cpu"):
    """Every byte 0x7F: a large finite fp32 / bf16 value no kernel writes."""
    width = torch.empty((), dtype=dtype).element_size()
    return torch.full((*shape[:-1], shape[-1] * width), 0x7F, dtype=torch.uint8, device=dev).view(dtype)


def out_buffers(dev, rows, groups, n):
    """row_stats, stats, group_stats, the padded dlogits, is_rows and is_stats, all poisoned."""
    return (poisoned((rows, 8), dev=dev), poisoned((8,), dev=dev), poisoned((groups, 4), dev=dev),
            poisoned((rows, n + PAD), torch.bfloat16, dev=dev), poisoned((rows, 2), dev=dev), poisoned((8,), dev=dev))


def units_of(tgt, level, group_rows):
    valid = [r for r in range(len(tgt)) if int(tgt[r]) != IGNORE_INDEX]
    if level == "token":
        return [[r] for r in valid]
    return [[r for r in valid if r // group_rows == k] for k in range(len(tgt) // group_rows)]     # empty sequences kept: k is the turn


@functools.lru_cache(maxsize=None)
def make_case(name, n, rng, T, level, norm, given, counts=None):
    """Sequences of group_rows rows whose valid rows sit at scattered positions; targets reach both ends of the policy's
    columns; every group of three or more has advantages of both signs and a zero. q (given proximal) and μ are placed from
    the specification's on-policy logp so that unit k has the ratio and the ρ wanted in its turn; self-proximal has q None
    and μ placed from that logp itself. Everything outside a token range is NaN / +inf. All inputs are fp32 values, so
    specification and kernel read the same."""
    group_rows, cnts = CASES[name]
    cnts = counts or cnts
    first, count = rng or (0, n)
    rows = group_rows * len(cnts)
    g = torch.Generator().manual_seed(n + first + count + rows)
    full = torch.empty(rows, n + PAD)
    full[:, 0::2], full[:, 1::2] = float("nan"), float("inf")
    full[:, first:first + count] = (torch.randn(rows, count, generator=g) * 2).to(torch.bfloat16).float()
    full[3, first:first + count] = 1.25                                        # an all-equal row
    tgt = torch.full((rows,), IGNORE_INDEX, dtype=torch.int64)
    A = torch.randn(rows, generator=g)
    for k, c in enumerate(cnts):
        pos = torch.randperm(group_rows, generator=g)[:c].sort().values + k * group_rows
        tgt[pos] = first + torch.randint(0, count, (c,), generator=g)
        if c >= 2:
            tgt[pos[0]], tgt[pos[-1]] = first, first + count - 1
        if c >= 3:
            A[pos[0]], A[pos[1]], A[pos[2]] = 1.5, -0.5, 0.0
        if c == 1:
            A[pos[0]] = 1.0 if k % 2 == 0 else -1.0
    base = PolicyLossConfig(temperature=T, token_range=rng)
    on = policy_loss(full.numpy()[:, :n], tgt.numpy(), np.zeros(rows), np.zeros(rows), cfg=base).logp
    q = torch.from_numpy(on).float()
    mu = q.clone()
    for k, idx in enumerate(units_of(tgt, level, group_rows)):
        if not idx:
            continue
        share = 1 if (norm == "mean" or level == "token") else len(idx)
        if given:
            q[idx] -= float(np.log(RATIOS[k % 5])) / share
        mu[idx] = q[idx] - float(np.log(RHOS[k % 5])) / share
    ref = torch.from_numpy(on).float() + torch.randn(rows, generator=g) * 0.3
    return full, tgt, A, (q if given else None), mu, ref, group_rows


def run_is(dev, full, n, tgt, A, q, mu, ref, cfg, group_rows, backward=True):
    """→ (row_stats, stats, group_stats, padded dlogits, is_rows, is_stats); group_stats stays poisoned at token level."""
    from bridgelang_amd import train_ops as T
    rows = full.shape[0]
    L = full.to(dev)[:, :n]
    to = lambda t: None if t is None else t.to(dev).contiguous()
    row_stats, stats, group_stats, base, is_rows, is_stats = out_buffers(dev, rows, rows // group_rows, n)
    op = T.policy_loss(L, tgt.to(dev), to(A), to(q), to(ref), row_stats, stats, cfg, group_rows=group_rows, group_stats=group_stats,
                       behaviour_logprob=to(mu), is_rows=is_rows, is_stats=is_stats)
    assert op.name == "bl_policy_loss_is_f32"
    if backward:
        T.policy_loss_backward(L, tgt.to(dev), row_stats, stats, base[:, :n], cfg)
    return row_stats, stats, group_stats, base, is_rows, is_stats


def run_plain(dev, full, n, tgt, A, q, ref, cfg, group_rows):
    """The uncorrected kernels on the same inputs: bl_policy_loss_range_f32 / bl_policy_loss_grouped_f32 and the backward."""
    from bridgelang_amd import train_ops as T
    rows = full.shape[0]
    L = full.to(dev)[:, :n]
    to = lambda t: None if t is None else t.to(dev).contiguous()
    row_stats, stats, group_stats, base, _, _ = out_buffers(dev, rows, rows // group_rows, n)
    op = T.policy_loss(L, tgt.to(dev), to(A), to(q), to(ref), row_stats, stats, cfg, group_rows=group_rows, group_stats=group_stats)
    assert op.name == ("bl_policy_loss_grouped_f32" if cfg.ratio_level == "action" else "bl_policy_loss_range_f32")
    T.policy_loss_backward(L, tgt.to(dev), row_stats, stats, base[:, :n], cfg)
    return row_stats, stats, group_stats, base


def check_clear_and_mixed(want, cfg):
    """On the specification alone, before any kernel runs: no ρ within 1e-3 (relative) of cap, low or high, so the exact
    comparison of the flags is well defined; truncated, masked (where there is a mask) and untouched rows all occur."""
    v = want.valid
    rho = np.exp(want.log_rho[v])
    for bound in (cfg.rollout_is_cap,) + tuple(cfg.rollout_is_mask or ()):
        if 0 < bound < np.inf:
            assert (np.abs(rho / bound - 1) >= 1e-3).all(), bound
    assert want.truncated.any() and (v & ~want.masked & ~want.truncated).any()
    assert bool(want.masked.any()) == (cfg.rollout_is_mask is not None)


@pytest.mark.parametrize("T,ent,klc", [(1.0, 0.0, 0.0), (0.7, 0.01, 0.1)])
@pytest.mark.parametrize("mask", [None, MASK], ids=["nomask", "mask"])
@pytest.mark.parametrize("given", [True, False], ids=["given", "self"])
@pytest.mark.parametrize("n,rng", SHAPES)
@pytest.mark.parametrize("name,level,norm", LEVELS)
def test_kernels_match_specification(dev, name, level, norm, n, rng, given, mask, T, ent, klc):
    cfg = PolicyLossConfig(temperature=T, entropy_coef=ent, kl_coef=klc, token_range=rng, ratio_level=level, ratio_norm=norm,
                           rollout_is_cap=CAP, rollout_is_mask=mask, **CLIP)
    full, tgt, A, q, mu, ref, group_rows = make_case(name, n, rng, T, level, norm, given)
    counts = np.array(CASES[name][1])
    ref = ref if klc else None
    want = policy_loss(full.numpy()[:, :n], tgt.numpy(), A.numpy(), None if q is None else q.numpy(),
                       None if ref is None else ref.numpy(), cfg, group_rows=group_rows, behaviour_logprobs=mu.numpy())
    # the reference alone
    v = want.valid
    check_clear_and_mixed(want, cfg)
    lo, hi = 1 - cfg.clip_low, 1 + cfg.clip_high
    r = want.ratio[v]
    assert (np.abs(r - lo) >= 1e-3).all() and (np.abs(r - hi) >= 1e-3).all()
    if given:
        assert want.clipped.any() and (v & ~want.clipped).any() and (r > hi).any() and (r < lo).any()
    else:
        assert (r == 1).all() and not want.clipped.any()
    a = A.numpy()[v]
    assert (a > 0).any() and (a < 0).any() and (a == 0).any()

    row_stats, stats, group_stats, base, is_rows, is_stats = run_is(dev, full, n, tgt, A, q, mu, ref, cfg, group_rows)
    rs, st, ir, ist = row_stats.cpu().numpy(), stats.cpu().numpy(), is_rows.cpu().numpy(), is_stats.cpu().numpy()
    col = {k: rs[:, i] for i, k in enumerate(ROW_STAT_NAMES)}
    lam, w = ir[:, 0], ir[:, 1]
    print(f"[{name} {level} {norm} n={n} range={rng} given={given} mask={mask} T={T}] loss {st[0]:.6f} vs {want.loss:.6f}; "
          f"max |logp err| {np.abs(col['logp'] - want.logp).max():.3g}; max |λ err| {np.abs(lam - want.log_rho).max():.3g}; "
          f"max |w err| {np.abs(w - want.weight).max():.3g}; is_stats {ist[:6]} vs {want.is_stats[:6]}")
    assert np.isfinite(rs).all() and np.isfinite(st).all() and np.isfinite(ir).all() and np.isfinite(ist).all()
    for k, ref_v in (("logp", want.logp), ("entropy", want.entropy), ("ratio", want.ratio), ("row_loss", want.row_loss), ("g", want.g)):
        scalars_close(col[k], ref_v, k)
    scalars_close(lam, want.log_rho, "λ")
    scalars_close(w, want.weight, "w")
    # counts and flags, exactly: the clip's side, and the weight's kind read off w itself (cap is an fp32 value)
    assert np.array_equal(col["clipped"], want.clipped.astype(np.float32))
    assert np.array_equal(v & (w == 0), want.masked) and np.array_equal(v & (w == np.float32(CAP)), want.truncated)
    nv = int(v.sum())
    assert st[1] == nv                                                         # a masked row still counts
    assert abs(ist[2] * nv - want.truncated.sum()) < 1e-3 and abs(ist[3] * nv - want.masked.sum()) < 1e-3     # the counts
    assert (ist[6:] == 0).all()
    scalars_close(ist, want.is_stats, "rollout statistics")
    scalars_close(st, want.stats, "step statistics")
    if not given:                                                              # self-proximal: log ratio 0, exactly
        assert (col["ratio"][v] == 1).all() and st[5] == 0 and st[6] == 0 and st[7] == 1      # clip_frac, approx_kl, ratio
    assert (rs[~v] == 0).all() and (ir[~v] == 0).all()
    # λ alone: the specification's λ over the KERNEL's own logp (self-proximal) or the given q — fp64 sums of the fp32
    # differences q − μ. A lane adds at most two terms, the butterfly six more levels, then the product with c (and 1 / n_G
    # itself): at most 10 roundings of 2^-24 relative to a partial sum that never exceeds c·Σ|δ|; one row: exact
    prox = col["logp"] if q is None else q.numpy()
    delta = np.where(v, (prox - mu.numpy()).astype(np.float64), 0.0)
    if level == "token":
        assert np.array_equal(lam[v], (prox - mu.numpy())[v])
    else:
        gs = group_stats.cpu().numpy()
        gs_want = want.group_stats
        full_g = counts > 0
        assert np.isfinite(gs).all() and (gs[~full_g] == 0).all() and np.array_equal(gs[:, 2], counts.astype(np.float32))
        for i, k in enumerate(GROUP_STAT_NAMES):
            scalars_close(gs[:, i], gs_want[:, i], f"group {k}")
        c = 1.0 / np.maximum(counts, 1) if norm == "mean" else np.ones(len(counts))
        d2 = delta.reshape(len(counts), group_rows)
        own, own_abs = c * d2.sum(1), c * np.abs(d2).sum(1)
        lam_g = np.array([lam.reshape(len(counts), group_rows)[k][v.reshape(len(counts), group_rows)[k]][0] if counts[k] else 0.0
                          for k in range(len(counts))])
        assert (np.abs(lam_g - own) <= 10 * 2.0 ** -24 * own_abs + 1e-30).all()
        for k in range(len(counts)):                                           # every valid row of a group carries its values
            rows_k = np.arange(k * group_rows, (k + 1) * group_rows)[v[k * group_rows:(k + 1) * group_rows]]
            assert len(set(lam[rows_k])) <= 1 and len(set(w[rows_k])) <= 1
    dl = base.float().cpu()
    assert (dl[:, n:] == poisoned((1,), torch.bfloat16).float().item()).all()     # the padding columns: untouched
    dl = dl[:, :n]
    assert torch.isfinite(dl).all()
    grad_close(dl, torch.from_numpy(want.dlogits), "dlogits", 1e-2)
    assert (dl.numpy()[~v] == 0).all() and (dl.numpy()[v] != 0).any()
    if rng is not None:                                    # finite values outside the range instead of NaN / inf: nothing changes
        outside = torch.ones(full.shape[1], dtype=torch.bool)
        outside[rng[0]:rng[0] + rng[1]] = False
        assert (dl.numpy()[:, outside.numpy()[:n]] == 0).all()
        tame = full.clone()
        tame[:, outside] = 0.5
        again = run_is(dev, tame, n, tgt, A, q, mu, ref, cfg, group_rows)
        assert all(torch.equal(x, y) for x, y in zip((row_stats, stats, group_stats, base, is_rows, is_stats), again))


@pytest.mark.parametrize("cap", [1.0, float("inf")])
@pytest.mark.parametrize("n,rng", SHAPES)
@pytest.mark.parametrize("name,level,norm", LEVELS)
def test_weight_one_is_the_uncorrected_kernels_bit_for_bit(dev, name, level, norm, n, rng, cap):
    """μ = q bit for bit, cap >= 1, no mask: w = 1, and everything the uncorrected entry point of the level writes — and
    the backward's dlogits — has the same bits."""
    base_cfg = dict(temperature=0.7, entropy_coef=0.01, kl_coef=0.1, token_range=rng or (0, n), ratio_level=level, ratio_norm=norm, **CLIP)
    full, tgt, A, q, _, ref, group_rows = make_case(name, n, rng, 0.7, level, norm, True)
    plain = run_plain(dev, full, n, tgt, A, q, ref, PolicyLossConfig(**base_cfg), group_rows)
    got = run_is(dev, full, n, tgt, A, q, q.clone(), ref, PolicyLossConfig(rollout_is_cap=cap, **base_cfg), group_rows)
    v = (tgt != IGNORE_INDEX).to(dev)
    clipped = plain[0][v, 4]
    assert bool((clipped == 1).any()) and bool((clipped == 0).any())            # a case that exercises the clip
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(got[3], plain[3])
    if level == "action":
        assert torch.equal(got[2], plain[2])
    is_rows, is_stats = got[4].cpu(), got[5].cpu()
    assert (is_rows[v.cpu(), 0] == 0).all() and (is_rows[v.cpu(), 1] == 1).all() and (is_rows[~v.cpu()] == 0).all()
    assert is_stats.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("given", [True, False], ids=["given", "self"])
@pytest.mark.parametrize("norm", ["sum", "mean"])
@pytest.mark.parametrize("n,rng", SHAPES)
def test_groups_of_one_row_are_the_token_level_form_bit_for_bit(dev, n, rng, norm, given):
    base_cfg = dict(temperature=0.7, entropy_coef=0.01, kl_coef=0.1, token_range=rng, rollout_is_cap=CAP, rollout_is_mask=MASK, **CLIP)
    full, tgt, A, q, mu, ref, group_rows = make_case("5x24", n, rng, 0.7, "action", norm, given, counts=(1, 1, 1, 1, 1, 1))
    rows = full.shape[0]
    assert rows == 144 and int((tgt != IGNORE_INDEX).sum()) == 6
    want = policy_loss(full.numpy()[:, :n], tgt.numpy(), A.numpy(), None if q is None else q.numpy(), ref.numpy(),
                       PolicyLossConfig(**base_cfg), behaviour_logprobs=mu.numpy())
    check_clear_and_mixed(want, PolicyLossConfig(**base_cfg))
    grouped = run_is(dev, full, n, tgt, A, q, mu, ref, PolicyLossConfig(ratio_level="action", ratio_norm=norm, **base_cfg), group_rows)
    token = run_is(dev, full, n, tgt, A, q, mu, ref, PolicyLossConfig(**base_cfg), group_rows)
    for i in (0, 1, 3, 4, 5):
        assert torch.equal(grouped[i], token[i]), i
    v = (tgt != IGNORE_INDEX).to(dev)
    w = token[4][v, 1]
    assert bool((w == 0).any()) and bool((w == CAP).any()) and bool(((w != 0) & (w != CAP)).any())


@pytest.mark.parametrize("name,level,norm", [("24", "token", "sum"), ("3x96", "action", "sum"), ("3x96", "action", "mean")])
def test_two_runs_are_bit_identical(dev, name, level, norm):
    n, rng = 2056, (1792, 256)
    cfg = PolicyLossConfig(temperature=0.7, entropy_coef=0.01, kl_coef=0.1, token_range=rng, ratio_level=level, ratio_norm=norm,
                           rollout_is_cap=CAP, rollout_is_mask=MASK, **CLIP)
    full, tgt, A, q, mu, ref, group_rows = make_case(name, n, rng, 0.7, level, norm, True)
    check_clear_and_mixed(policy_loss(full.numpy()[:, :n], tgt.numpy(), A.numpy(), q.numpy(), ref.numpy(), cfg, group_rows=group_rows,
                                      behaviour_logprobs=mu.numpy()), cfg)
    a = run_is(dev, full, n, tgt, A, q, mu, ref, cfg, group_rows)
    b = run_is(dev, full, n, tgt, A, q, mu, ref, cfg, group_rows)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[4]).all()) and not torch.equal(a[4], poisoned(tuple(a[4].shape), dev=dev))


def test_argument_checks(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n = 4, 64
    L = torch.zeros(rows * n + 8, device=dev)
    tg = torch.full((rows,), 20, dtype=torch.int64, device=dev)
    f = torch.zeros(rows, device=dev)
    mu = torch.full((rows,), float(-np.log(8.0)) - float(np.log(2.0)), device=dev)      # ρ = 2 under the uniform policy over 8 tokens
    rs, st, gs, _, ir, ist = out_buffers(dev, rows, rows, n)
    keep = [t.clone() for t in (rs, st, gs, ir, ist)]
    s = torch.cuda.current_stream().cuda_stream
    inf = float("inf")

    def fwd(group_rows=2, norm=0, first=16, count=8, ptr=L.data_ptr(), n_=n, temperature=1.0, gsp=gs.data_ptr(), ld=n, old=None,
            mup=mu.data_ptr(), cap=1.5, low=0.0, high=inf, irp=ir.data_ptr(), istp=ist.data_ptr()):
        return lib.bl_policy_loss_is_f32(ptr, ld, rows, n_, tg.data_ptr(), -100, f.data_ptr(), old, mup, None, temperature, 0.2, 0.2,
                                         0.0, 0.0, rs.data_ptr(), st.data_ptr(), first, count, group_rows, norm, gsp, cap, low, high,
                                         irp, istp, s)
    assert fwd(mup=None) == _lib.BL_E_ARG and fwd(irp=None) == _lib.BL_E_ARG and fwd(istp=None) == _lib.BL_E_ARG
    assert fwd(gsp=None) == _lib.BL_E_ARG and fwd(group_rows=0) == _lib.BL_E_ARG        # group_stats iff group_rows > 0
    for cap in (0.0, -1.0, float("nan")):
        assert fwd(cap=cap) == _lib.BL_E_ARG, cap
    for low, high in ((-0.5, 2.0), (2.0, 2.0), (3.0, 2.0), (float("nan"), 2.0), (0.5, float("nan"))):
        assert fwd(low=low, high=high) == _lib.BL_E_ARG, (low, high)
    for group_rows in (-2, 3, 8):
        assert fwd(group_rows=group_rows) == _lib.BL_E_SHAPE, group_rows
    assert fwd(norm=2) == _lib.BL_E_SHAPE and fwd(norm=-1) == _lib.BL_E_SHAPE
    # the existing forward's checks
    for first, count in ((12, 8), (16, 12), (60, 8), (64, 8), (-8, 16), (16, 0), (16, -8)):
        assert fwd(first=first, count=count) == _lib.BL_E_SHAPE, (first, count)
    assert fwd(n_=60) == _lib.BL_E_SHAPE and fwd(ld=n + 2) == _lib.BL_E_SHAPE
    assert fwd(ptr=None) == _lib.BL_E_ARG and fwd(temperature=0.0) == _lib.BL_E_ARG
    assert fwd(ptr=L.data_ptr() + 4) == _lib.BL_E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((rs, st, gs, ir, ist), keep))  # nothing was launched
    for group_rows, norm in ((2, 0), (1, 1), (2, 1)):
        assert fwd(group_rows=group_rows, norm=norm) == _lib.BL_OK
    assert fwd(group_rows=0, gsp=None) == _lib.BL_OK and fwd(old=f.data_ptr(), cap=inf, low=0.5, high=3.0) == _lib.BL_OK
    assert fwd(first=0, count=n) == _lib.BL_OK and fwd(group_rows=4, norm=1) == _lib.BL_OK
    torch.cuda.synchronize()
    # one group of four uniform rows over the 8 tokens of the range, self-proximal, mean norm: λ_G = log 2, w = min(2, 1.5)
    got, rows_got, stats_got = gs.cpu().numpy()[0], ir.cpu().numpy(), ist.cpu().numpy()
    assert got[2] == 4 and got[0] == 0 and got[1] == 1 and np.allclose(got[3], -4 * np.log(8.0), rtol=1e-5)
    assert np.allclose(rows_got[:, 0], np.log(2.0), rtol=1e-5) and (rows_got[:, 1] == 1.5).all()
    assert np.allclose(stats_got[:6], [1.5, 2.0, 1.0, 0.0, 1.0 - np.log(2.0), -np.log(2.0)], rtol=1e-4) and (stats_got[6:] == 0).all()
