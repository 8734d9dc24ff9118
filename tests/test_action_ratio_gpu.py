"""bl_policy_loss_grouped_f32 (the action-level importance ratio) against its fp64 specification (training/policy_loss.py with
ratio_level="action"), against the token-level kernels where the two coincide bit for bit, and its determinism and argument
checks. Bounds are those of tests/test_policy_loss_gpu.py (helpers copied, not imported)."""
import functools

import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import (GROUP_STAT_NAMES, IGNORE_INDEX, ROW_STAT_NAMES, PolicyLossConfig, policy_loss)

pytestmark = pytest.mark.gpu

PAD = 8                                                    # the padded leading dimension: ld = n + PAD
# (group_rows, valid rows per sequence, ratio_G wanted per sequence): five sequences in two workgroups of the group kernel,
# and sequences longer than a wave so that lanes stride
CASES = {"5x24": (24, (0, 1, 2, 7, 23), (1.0, 0.5, 1.6, 1.1, 0.7)),
         "2x96": (96, (70, 3), (1.5, 0.6))}
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
    """row_stats, stats, group_stats and the padded dlogits, all poisoned."""
    return (poisoned((rows, 8), dev=dev), poisoned((8,), dev=dev), poisoned((groups, 4), dev=dev),
            poisoned((rows, n + PAD), torch.bfloat16, dev=dev))


@functools.lru_cache(maxsize=None)
def make_case(name, n, rng, T, norm, counts=None):
    """Sequences of group_rows rows whose valid rows sit at scattered positions; targets reach both ends of the policy's
    columns; every group of three or more has advantages of both signs and a zero; q is placed from the specification's
    on-policy logp so that group k's ratio is the wanted one. Everything outside a token range is NaN / +inf. All inputs
    are fp32 values, so specification and kernel read the same."""
    group_rows, cnts, want = CASES[name]
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
    members = []
    for k, c in enumerate(cnts):
        pos = torch.randperm(group_rows, generator=g)[:c].sort().values + k * group_rows
        members.append(pos)
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
    for k, pos in enumerate(members):
        if len(pos):
            q[pos] -= float(np.log(want[k % len(want)])) / (1 if norm == "mean" else len(pos))
    ref = torch.from_numpy(on).float() + torch.randn(rows, generator=g) * 0.3
    return full, tgt, A, q, ref, group_rows


def run_grouped(dev, full, n, tgt, A, q, ref, cfg, group_rows, backward=True):
    from bridgelang_amd import train_ops as T
    rows = full.shape[0]
    L = full.to(dev)[:, :n]
    to = lambda t: None if t is None else t.to(dev).contiguous()
    row_stats, stats, group_stats, base = out_buffers(dev, rows, rows // group_rows, n)
    op = T.policy_loss(L, tgt.to(dev), to(A), to(q), to(ref), row_stats, stats, cfg, group_rows=group_rows, group_stats=group_stats)
    assert op.name == "bl_policy_loss_grouped_f32"
    if backward:
        T.policy_loss_backward(L, tgt.to(dev), row_stats, stats, base[:, :n], cfg)
    return row_stats, stats, group_stats, base


@pytest.mark.parametrize("T,ent,klc", [(1.0, 0.0, 0.0), (0.7, 0.01, 0.1)])
@pytest.mark.parametrize("norm", ["sum", "mean"])
@pytest.mark.parametrize("n,rng", SHAPES)
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_specification(dev, name, n, rng, norm, T, ent, klc):
    cfg = PolicyLossConfig(temperature=T, entropy_coef=ent, kl_coef=klc, token_range=rng, ratio_level="action", ratio_norm=norm, **CLIP)
    full, tgt, A, q, ref, group_rows = make_case(name, n, rng, T, norm)
    _, counts, wanted = CASES[name]
    ref = ref if klc else None
    want = policy_loss(full.numpy()[:, :n], tgt.numpy(), A.numpy(), q.numpy(), None if ref is None else ref.numpy(), cfg,
                       group_rows=group_rows)
    # the reference alone: the groups are the wanted ones, no ratio within reach of a boundary, both outcomes occur
    v, gs_want = want.valid, want.group_stats
    lo, hi = 1 - cfg.clip_low, 1 + cfg.clip_high
    full_g = np.array(counts) > 0
    assert np.array_equal(gs_want[:, 2], counts) and np.allclose(gs_want[full_g, 1], np.array(wanted)[full_g], rtol=1e-3)
    r = gs_want[full_g, 1]
    assert (np.abs(r - lo) >= 1e-3).all() and (np.abs(r - hi) >= 1e-3).all()
    assert want.clipped.any() and (v & ~want.clipped).any() and (r > hi).any() and (r < lo).any()
    a = A.numpy()[v]
    assert (a > 0).any() and (a < 0).any() and (a == 0).any()
    assert np.array_equal(want.ratio[v], np.repeat(gs_want[:, 1], group_rows)[v])

    row_stats, stats, group_stats, base = run_grouped(dev, full, n, tgt, A, q, ref, cfg, group_rows)
    rs, st, gs = row_stats.cpu().numpy(), stats.cpu().numpy(), group_stats.cpu().numpy()
    col = {k: rs[:, i] for i, k in enumerate(ROW_STAT_NAMES)}
    gcol = {k: gs[:, i] for i, k in enumerate(GROUP_STAT_NAMES)}
    # the group pass alone: the specification's s_G over the KERNEL's logp column (fp64 sums of the fp32 differences)
    delta = np.where(v, (col["logp"] - q.numpy()).astype(np.float64), 0.0).reshape(len(counts), group_rows)
    c = 1.0 / np.maximum(np.array(counts), 1) if norm == "mean" else np.ones(len(counts))
    own, own_abs = c * delta.sum(1), c * np.abs(delta).sum(1)
    print(f"[{name} n={n} range={rng} {norm} T={T}] loss {st[0]:.6f} vs {want.loss:.6f}; max |logp err| "
          f"{np.abs(col['logp'] - want.logp).max():.3g}; max |s_G err| {np.abs(gcol['log_ratio'] - gs_want[:, 0]).max():.3g} "
          f"(vs the specification on the kernel's logp: {np.abs(gcol['log_ratio'] - own).max():.3g}); "
          f"max ratio rel err {np.abs(gcol['ratio'] / np.where(full_g, gs_want[:, 1], 1) - full_g).max():.3g}")
    assert np.isfinite(rs).all() and np.isfinite(st).all() and np.isfinite(gs).all()
    for k, ref_v in (("logp", want.logp), ("entropy", want.entropy), ("ratio", want.ratio), ("row_loss", want.row_loss), ("g", want.g)):
        scalars_close(col[k], ref_v, k)
    assert np.array_equal(col["clipped"], want.clipped.astype(np.float32))
    assert np.array_equal(gcol["n"], np.array(counts, dtype=np.float32))
    for i, k in enumerate(GROUP_STAT_NAMES):
        scalars_close(gcol[k], gs_want[:, i], f"group {k}")
    # a lane adds at most two terms, the butterfly six more levels, then the product with c (and 1 / n_G itself): at most
    # 10 roundings of 2^-24 relative to a partial sum that never exceeds c·Σ|δ|
    assert (np.abs(gcol["log_ratio"] - own) <= 10 * 2.0 ** -24 * own_abs + 1e-30).all()
    assert (rs[~v] == 0).all() and (gs[~full_g] == 0).all() and st[1] == v.sum()
    scalars_close(st, want.stats, "step statistics")
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
        again = run_grouped(dev, tame, n, tgt, A, q, ref, cfg, group_rows)
        assert all(torch.equal(x, y) for x, y in zip((row_stats, stats, group_stats, base), again))


@pytest.mark.parametrize("norm", ["sum", "mean"])
@pytest.mark.parametrize("n,rng", SHAPES)
def test_groups_of_one_row_are_the_token_level_kernels_bit_for_bit(dev, n, rng, norm):
    from bridgelang_amd import train_ops as T
    base_cfg = dict(temperature=0.7, entropy_coef=0.01, kl_coef=0.1, token_range=rng, **CLIP)
    full, tgt, A, q, ref, group_rows = make_case("5x24", n, rng, 0.7, norm, counts=(1, 1, 1, 1, 1, 1))    # six sequences: 4 + 2
    rows = full.shape[0]
    assert rows == 144 and int((tgt != IGNORE_INDEX).sum()) == 6
    grouped = run_grouped(dev, full, n, tgt, A, q, ref, PolicyLossConfig(ratio_level="action", ratio_norm=norm, **base_cfg), group_rows)
    cfg = PolicyLossConfig(**base_cfg)
    L = full.to(dev)[:, :n]
    row_stats, stats, _, dl = out_buffers(dev, rows, rows // group_rows, n)
    op = T.policy_loss(L, tgt.to(dev), A.to(dev), q.to(dev), ref.to(dev), row_stats, stats, cfg)
    assert op.name == ("bl_policy_loss_f32" if rng is None else "bl_policy_loss_range_f32")
    T.policy_loss_backward(L, tgt.to(dev), row_stats, stats, dl[:, :n], cfg)
    v = (tgt != IGNORE_INDEX).to(dev)
    clipped = row_stats[v, 4]
    assert bool((clipped == 1).any()) and bool((clipped == 0).any())            # a case that exercises the clip
    assert torch.equal(grouped[0], row_stats) and torch.equal(grouped[1], stats) and torch.equal(grouped[3], dl)
    gs = grouped[2]
    assert torch.equal(gs[:, 1], row_stats[v, 2]) and torch.equal(gs[:, 3], row_stats[v, 0]) and bool((gs[:, 2] == 1).all())


@pytest.mark.parametrize("norm", ["sum", "mean"])
def test_two_runs_are_bit_identical(dev, norm):
    n, rng = 2056, (1792, 256)
    cfg = PolicyLossConfig(temperature=0.7, entropy_coef=0.01, kl_coef=0.1, token_range=rng, ratio_level="action", ratio_norm=norm, **CLIP)
    full, tgt, A, q, ref, group_rows = make_case("2x96", n, rng, 0.7, norm)
    a = run_grouped(dev, full, n, tgt, A, q, ref, cfg, group_rows)
    b = run_grouped(dev, full, n, tgt, A, q, ref, cfg, group_rows)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert bool(torch.isfinite(a[0]).all()) and not torch.equal(a[0], poisoned((192, 32), dev=dev))


def test_argument_checks(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    rows, n = 4, 64
    L = torch.zeros(rows * n + 8, device=dev)
    tg = torch.full((rows,), 20, dtype=torch.int64, device=dev)
    f = torch.zeros(rows, device=dev)
    rs, st, gs, _ = out_buffers(dev, rows, rows, n)
    keep = [t.clone() for t in (rs, st, gs)]
    s = torch.cuda.current_stream().cuda_stream

    def fwd(group_rows=2, norm=0, first=16, count=8, ptr=L.data_ptr(), n_=n, temperature=1.0, gsp=gs.data_ptr(), ld=n):
        return lib.bl_policy_loss_grouped_f32(ptr, ld, rows, n_, tg.data_ptr(), -100, f.data_ptr(), f.data_ptr(), None, temperature, 0.2,
                                              0.2, 0.0, 0.0, rs.data_ptr(), st.data_ptr(), first, count, group_rows, norm, gsp, s)
    assert fwd(gsp=None) == _lib.BL_E_ARG
    for group_rows in (0, -2, 3, 8):
        assert fwd(group_rows=group_rows) == _lib.BL_E_SHAPE, group_rows
    assert fwd(norm=2) == _lib.BL_E_SHAPE and fwd(norm=-1) == _lib.BL_E_SHAPE
    # the existing forward's checks
    for first, count in ((12, 8), (16, 12), (60, 8), (64, 8), (-8, 16), (16, 0), (16, -8)):
        assert fwd(first=first, count=count) == _lib.BL_E_SHAPE, (first, count)
    assert fwd(n_=60) == _lib.BL_E_SHAPE and fwd(ld=n + 2) == _lib.BL_E_SHAPE
    assert fwd(ptr=None) == _lib.BL_E_ARG and fwd(temperature=0.0) == _lib.BL_E_ARG
    assert fwd(ptr=L.data_ptr() + 4) == _lib.BL_E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((rs, st, gs), keep))              # nothing was launched
    for group_rows, norm in ((2, 0), (1, 1), (2, 1)):
        assert fwd(group_rows=group_rows, norm=norm) == _lib.BL_OK
    assert fwd(first=0, count=n) == _lib.BL_OK and fwd(group_rows=4, norm=1) == _lib.BL_OK
    torch.cuda.synchronize()
    got = gs.cpu().numpy()[0]                              # one group of four uniform rows over the 8 tokens of the range, q = 0
    assert got[2] == 4 and np.allclose(got[[0, 1, 3]], [-np.log(8.0), 1 / 8, -4 * np.log(8.0)], rtol=1e-5)
