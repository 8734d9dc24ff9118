"""The action-level importance ratio of the policy loss (PolicyLossConfig.ratio_level = "action"), host side: the fp64
specification against torch.autograd over an independent restatement, the cases where it must equal the token-level loss
exactly, the validation of the new settings, and the new entry point in header, ctypes table and built library."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import (GROUP_STAT_NAMES, IGNORE_INDEX, STAT_NAMES, PolicyLossConfig, policy_loss)

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("logp", "entropy", "ratio", "pg", "kl", "row_loss", "clipped", "valid", "g", "stats", "dlogits")


def restated(logits, tg, A, q, ref, cfg, group_rows):
    """The action-level loss in torch fp64, written from the formulas and not from the numpy code: a loop over the
    sequences, log_softmax, minimum and clamp. → (loss, stats dict, group statistics list)."""
    lo, hi = 1 - cfg.clip_low, 1 + cfg.clip_high
    lsm = torch.log_softmax(logits / cfg.temperature, dim=-1)
    H = -(lsm.exp() * lsm).sum(-1)
    total = 0.0
    acc = dict(pg=0.0, entropy=0.0, kl=0.0, clip_frac=0.0, approx_kl=0.0, ratio=0.0)
    nv, groups = 0, []
    for k in range(logits.shape[0] // group_rows):
        idx = [r for r in range(k * group_rows, (k + 1) * group_rows) if int(tg[r]) != IGNORE_INDEX]
        if not idx:
            groups.append((0.0, 0.0, 0, 0.0))
            continue
        i = torch.tensor(idx)
        logp = lsm[i, tg[i]]
        s = (logp - q[i]).sum() * (1.0 / len(idx) if cfg.ratio_norm == "mean" else 1.0)
        ratio = torch.exp(s)
        pg = -torch.minimum(ratio * A[i], ratio.clamp(lo, hi) * A[i])
        d = ref[i] - logp
        kl = torch.exp(d) - d - 1
        total = total + (pg - cfg.entropy_coef * H[i] + cfg.kl_coef * kl).sum()
        active = ((A[i] >= 0) & (ratio <= hi)) | ((A[i] < 0) & (ratio >= lo))
        for name, v in (("pg", pg.sum()), ("entropy", H[i].sum()), ("kl", kl.sum()), ("clip_frac", (~active).double().sum()),
                        ("approx_kl", (torch.expm1(s) - s) * len(idx)), ("ratio", ratio * len(idx))):
            acc[name] = acc[name] + v
        nv += len(idx)
        groups.append((s.item(), ratio.item(), len(idx), logp.sum().item()))
    loss = total / nv
    stats = dict(loss=loss, n_valid=nv, **{k: v / nv for k, v in acc.items()})
    return loss, stats, groups


def small_case(seed, rows, n, group_rows, counts):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, n, generator=g, dtype=torch.float64) * 2
    tg = torch.full((rows,), IGNORE_INDEX, dtype=torch.int64)
    for k, c in enumerate(counts):                     # the labelled rows of a sequence: a run that ends before its last row
        start = k * group_rows + (group_rows - 1 - c) // 2
        tg[start:start + c] = torch.randint(0, n, (c,), generator=g)
    A = torch.randn(rows, generator=g, dtype=torch.float64)
    q = -2.0 + 0.05 * torch.randn(rows, generator=g, dtype=torch.float64)
    ref = -2.0 + 0.3 * torch.randn(rows, generator=g, dtype=torch.float64)
    return logits, tg, A, q, ref


@pytest.mark.parametrize("norm", ["sum", "mean"])
def test_specification_matches_autograd(norm):
    group_rows, n = 12, 16
    counts = (7, 0, 1, 11, 4)
    cfg = PolicyLossConfig(temperature=0.8, clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.1, ratio_level="action",
                           ratio_norm=norm)
    logits, tg, A, q, ref = small_case(5, 5 * group_rows, n, group_rows, counts)
    # place q from the on-policy logp so that the group ratios sit on both clipped sides and inside, away from the boundaries
    on = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), np.zeros(len(tg)), None, PolicyLossConfig(temperature=0.8)).logp
    want_ratio = {0: 1.6, 2: 0.5, 3: 1.1, 4: 0.9}
    q = torch.from_numpy(on.copy())
    for k, r in want_ratio.items():
        rows_k = [i for i in range(k * group_rows, (k + 1) * group_rows) if int(tg[i]) != IGNORE_INDEX]
        q[rows_k] -= np.log(r) / (1 if norm == "mean" else len(rows_k))
    got = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), q.numpy(), ref.numpy(), cfg, group_rows=group_rows)
    assert got.clipped.any() and (got.valid & ~got.clipped).any()
    leaf = logits.clone().requires_grad_(True)
    loss, stats, groups = restated(leaf, tg, A, q, ref, cfg, group_rows)
    (grad,) = torch.autograd.grad(loss, leaf)
    scale = grad.abs().max().item()
    assert scale > 0 and np.abs(got.dlogits - grad.numpy()).max() <= 1e-9 * scale
    assert abs(got.loss - loss.item()) <= 1e-12 * max(abs(loss.item()), 1.0)
    for i, name in enumerate(STAT_NAMES):
        assert abs(got.stats[i] - float(stats[name])) <= 1e-12 * max(abs(float(stats[name])), 1.0), name
    want_groups = np.array(groups, dtype=np.float64)
    assert got.group_stats.shape == (5, len(GROUP_STAT_NAMES)) and np.array_equal(got.group_stats[:, 2], counts)
    assert np.abs(got.group_stats - want_groups).max() <= 1e-12 * max(np.abs(want_groups).max(), 1.0)
    for k, r in want_ratio.items():
        assert got.group_stats[k, 1] == pytest.approx(r, rel=1e-9)
    assert (got.group_stats[1] == 0).all()                                     # the empty sequence
    v = got.valid
    assert np.array_equal(got.ratio[v], np.repeat(got.group_stats[:, 1], group_rows)[v]) and (got.ratio[~v] == 0).all()
    assert (got.dlogits[~v] == 0).all() and np.isfinite(got.dlogits).all()


@pytest.mark.parametrize("norm", ["sum", "mean"])
@pytest.mark.parametrize("token_range", [None, (8, 8)])
def test_groups_of_at_most_one_row_are_the_token_level_loss(norm, token_range):
    rows, n, group_rows = 24, 16, 4
    logits, tg, A, q, ref = small_case(7, rows, n, group_rows, (1, 0, 1, 1, 0, 1))
    if token_range is not None:
        tg = torch.where(tg != IGNORE_INDEX, tg % 8 + 8, tg)
    base = dict(temperature=0.7, clip_low=0.02, clip_high=0.03, entropy_coef=0.01, kl_coef=0.1, token_range=token_range)
    args = (logits.numpy(), tg.numpy(), A.numpy(), q.numpy(), ref.numpy())
    token = policy_loss(*args, PolicyLossConfig(**base))
    token_ignoring = policy_loss(*args, PolicyLossConfig(**base), group_rows=5)           # ignored at token level
    action = policy_loss(*args, PolicyLossConfig(ratio_level="action", ratio_norm=norm, **base), group_rows=group_rows)
    assert token.clipped.any() and (token.valid & ~token.clipped).any() and token.group_stats is None
    for name in FIELDS:
        assert np.array_equal(getattr(action, name), getattr(token, name)), name
        assert np.array_equal(getattr(token_ignoring, name), getattr(token, name)), name
    assert action.loss == token.loss
    # group_rows = 1: every row its own sequence
    single = policy_loss(*args, PolicyLossConfig(ratio_level="action", ratio_norm=norm, **base), group_rows=1)
    for name in FIELDS:
        assert np.array_equal(getattr(single, name), getattr(token, name)), name
    assert np.array_equal(single.group_stats[:, 2], token.valid.astype(np.float64))
    assert np.array_equal(single.group_stats[:, 3], token.logp) and np.array_equal(single.group_stats[:, 1], token.ratio)


def test_mean_of_equal_log_ratios_is_the_token_ratio():
    rows, n = 12, 16
    logits, tg, A, q, ref = small_case(3, rows, n, rows, (7,))
    on = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), np.zeros(rows), None).logp
    q = on - 0.125                                                              # every δ = 0.125
    token = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), q, None, PolicyLossConfig())
    mean = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), q, None, PolicyLossConfig(ratio_level="action", ratio_norm="mean"),
                       group_rows=rows)
    total = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), q, None, PolicyLossConfig(ratio_level="action"), group_rows=rows)
    v = token.valid
    assert v.sum() == 7 and mean.group_stats[0, 2] == 7
    assert np.allclose(mean.ratio[v], token.ratio[v], rtol=1e-14, atol=0) and np.allclose(mean.ratio[v], np.exp(0.125), rtol=1e-14, atol=0)
    assert np.allclose(mean.pg[v], token.pg[v], rtol=1e-14, atol=0)
    assert np.allclose(total.ratio[v], np.exp(7 * 0.125), rtol=1e-13, atol=0)


def test_config_and_group_rows_validation():
    for bad in (dict(ratio_level="sequence"), dict(ratio_level="action", ratio_norm="geometric"), dict(ratio_norm="mean"),
                dict(ratio_level="token", ratio_norm="mean")):
        with pytest.raises(ValueError):
            PolicyLossConfig(**bad)
    assert PolicyLossConfig().ratio_level == "token" and PolicyLossConfig().ratio_norm == "sum"
    logits, tg, A, q, ref = small_case(1, 12, 16, 4, (2, 1, 3))
    args = (logits.numpy(), tg.numpy(), A.numpy(), q.numpy())
    for norm in ("sum", "mean"):
        cfg = PolicyLossConfig(ratio_level="action", ratio_norm=norm)
        for bad in (None, 5, 0, -4, 24):
            with pytest.raises(ValueError):
                policy_loss(*args, None, cfg, group_rows=bad)
        with pytest.raises(ValueError):
            policy_loss(*args, None, PolicyLossConfig(ratio_level="action", ratio_norm=norm, token_range=(0, 16)))
        assert policy_loss(*args, None, cfg, group_rows=4).group_stats.shape == (3, 4)


def test_grouped_entry_point_is_declared_bound_and_exported():
    from bridgelang_amd import _lib
    name = "bl_policy_loss_grouped_f32"
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    declared = set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", header))
    assert name in declared and f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == 22                                 # the ranged forward's 19, then 3 (stream last)
    assert _lib.SIGNATURES[name][1][:18] == _lib.SIGNATURES["bl_policy_loss_range_f32"][1][:18]
    lib = _lib.load()
    assert hasattr(lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"bl_[a-z0-9_]+", line.split()[-1])}
    assert name in exported
    assert declared == set(_lib.SIGNATURES) == exported, (declared ^ exported, declared ^ set(_lib.SIGNATURES))
