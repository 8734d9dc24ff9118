"""The rollout correction of the policy loss (PolicyLossConfig.rollout_is_cap / rollout_is_mask: a truncated importance weight
between the proximal policy and the policy that drew the tokens), host side: the fp64 specification against torch.autograd
over an independent restatement at both ratio levels, in both proximal modes, with and without mask and token range; the
cases where it must equal the uncorrected loss exactly; the self-proximal form; validation; `rl.policy_batch`; and the new
entry point in header, ctypes table and built library."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import (IGNORE_INDEX, IS_STAT_NAMES, STAT_NAMES, PolicyLossConfig, policy_loss)
from bridgelang_amd.training.rl import policy_batch

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("logp", "entropy", "ratio", "pg", "kl", "row_loss", "clipped", "valid", "g", "stats", "dlogits")
GROUP_ROWS, COUNTS, N = 12, (7, 0, 1, 11, 4, 3), 16
# per sequence: the ratio π_θ/π_prox wanted (given proximal only) and ρ = π_prox/μ wanted — with cap 1.5 and mask (0.5, 3):
# untouched, truncated, masked above, masked below, untouched
WANT_RATIO = {0: 1.6, 2: 0.5, 3: 1.1, 4: 0.9, 5: 1.0}
WANT_RHO = {0: 2.0, 2: 4.0, 3: 0.8, 4: 0.3, 5: 1.2}
CAP, MASK = 1.5, (0.5, 3.0)


def units_of(tg, level):
    """The index lists the ratio and the weight are formed over: every valid row at token level, a sequence's valid rows at
    action level."""
    valid = [r for r in range(len(tg)) if int(tg[r]) != IGNORE_INDEX]
    if level == "token":
        return [[r] for r in valid]
    return [u for u in ([r for r in valid if r // GROUP_ROWS == k] for k in range(len(tg) // GROUP_ROWS)) if u]


def restated(logits, tg, A, q, mu, ref, cfg):
    """The corrected loss in torch fp64, written from the formulas and not from the numpy code: a loop over the units,
    log_softmax over the token range, minimum and clamp, detach() on w and on the self-proximal q. → (loss, statistics,
    rollout statistics, λ per row, w per row)."""
    lo, hi = 1 - cfg.clip_low, 1 + cfg.clip_high
    first, count = cfg.token_range or (0, logits.shape[1])
    low, high = cfg.rollout_is_mask or (0.0, float("inf"))
    lsm = torch.log_softmax(logits[:, first:first + count] / cfg.temperature, dim=-1)
    H = -(lsm.exp() * lsm).sum(-1)
    total, nv = 0.0, 0
    acc = dict(pg=0.0, entropy=0.0, kl=0.0, clip_frac=0.0, approx_kl=0.0, ratio=0.0)
    isacc = dict.fromkeys(IS_STAT_NAMES, 0.0)
    lam_rows, w_rows = torch.zeros(len(tg), dtype=torch.float64), torch.zeros(len(tg), dtype=torch.float64)
    for idx in units_of(tg, cfg.ratio_level):
        i, k = torch.tensor(idx), len(idx)
        logp = lsm[i, tg[i] - first]
        prox = logp.detach() if q is None else q[i]
        c = 1.0 / k if cfg.ratio_norm == "mean" else 1.0
        s = c * (logp - prox).sum()
        lam = (c * (prox - mu[i]).sum()).detach()
        rho = torch.exp(lam)
        masked = bool(rho < low or rho > high)
        w = torch.zeros((), dtype=torch.float64) if masked else rho.clamp(max=cfg.rollout_is_cap)
        ratio = torch.exp(s)
        pg = w * -torch.minimum(ratio * A[i], ratio.clamp(lo, hi) * A[i])
        kl = torch.zeros(k, dtype=torch.float64)
        if ref is not None:
            d = ref[i] - logp
            kl = torch.exp(d) - d - 1
        total = total + (pg - cfg.entropy_coef * H[i] + cfg.kl_coef * kl).sum()
        active = ((A[i] >= 0) & (ratio <= hi)) | ((A[i] < 0) & (ratio >= lo))
        for name, v in (("pg", pg.sum()), ("entropy", H[i].sum()), ("kl", kl.sum()), ("clip_frac", (~active).double().sum()),
                        ("approx_kl", (torch.expm1(s) - s) * k), ("ratio", ratio * k)):
            acc[name] = acc[name] + v
        for name, v in (("weight", w), ("rho", rho), ("trunc_frac", float(not masked and rho > cfg.rollout_is_cap)),
                        ("mask_frac", float(masked)), ("rollout_kl", rho - 1 - lam), ("rollout_k1", -lam)):
            isacc[name] = isacc[name] + v * k
        lam_rows[i], w_rows[i] = lam, w
        nv += k
    loss = total / nv
    return (loss, dict(loss=loss, n_valid=nv, **{k: v / nv for k, v in acc.items()}), {k: v / nv for k, v in isacc.items()},
            lam_rows, w_rows)


def small_case(seed, token_range=None):
    rows = GROUP_ROWS * len(COUNTS)
    first, count = token_range or (0, N)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, N, generator=g, dtype=torch.float64) * 2
    tg = torch.full((rows,), IGNORE_INDEX, dtype=torch.int64)
    for k, c in enumerate(COUNTS):                     # the labelled rows of a sequence: a run that ends before its last row
        start = k * GROUP_ROWS + (GROUP_ROWS - 1 - c) // 2
        tg[start:start + c] = first + torch.randint(0, count, (c,), generator=g)
    A = torch.randn(rows, generator=g, dtype=torch.float64)
    ref = -2.0 + 0.3 * torch.randn(rows, generator=g, dtype=torch.float64)
    return logits, tg, A, ref


def place(on, tg, level, norm, given):
    """q and μ from the specification's own on-policy logp, so that every unit of sequence k has the ratio and the ρ wanted
    for k. Self-proximal (`given` False): q is None and μ is placed from logp itself."""
    q, mu = torch.from_numpy(on.copy()), torch.from_numpy(on.copy())
    for idx in units_of(tg, level):
        k, share = idx[0] // GROUP_ROWS, (1 if norm == "mean" or level == "token" else len(idx))
        if given:
            q[idx] -= np.log(WANT_RATIO[k]) / share
        mu[idx] = q[idx] - np.log(WANT_RHO[k]) / share
    return (q if given else None), mu


def check_clear_and_mixed(res, cfg):
    """On the specification alone: no ρ within 1e-3 (relative) of cap, low or high, so that the flags are well defined, and
    truncated, masked (when there is a mask) and untouched rows all occur."""
    v = res.valid
    rho = np.exp(res.log_rho[v])
    for bound in (cfg.rollout_is_cap,) + tuple(cfg.rollout_is_mask or ()):
        if 0 < bound < np.inf:
            assert (np.abs(rho / bound - 1) >= 1e-3).all(), bound
    untouched = v & ~res.masked & ~res.truncated
    assert res.truncated.any() and untouched.any() and res.masked.any() == (cfg.rollout_is_mask is not None)
    assert (res.weight[res.masked] == 0).all() and (res.weight[res.truncated] == cfg.rollout_is_cap).all()
    assert np.array_equal(res.weight[untouched], np.exp(res.log_rho[untouched]))


@pytest.mark.parametrize("token_range", [None, (8, 8)])
@pytest.mark.parametrize("mask", [None, MASK])
@pytest.mark.parametrize("given", [True, False], ids=["given", "self"])
@pytest.mark.parametrize("level,norm", [("token", "sum"), ("action", "sum"), ("action", "mean")])
def test_specification_matches_autograd(level, norm, given, mask, token_range):
    cfg = PolicyLossConfig(temperature=0.8, clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.1, ratio_level=level,
                           ratio_norm=norm, token_range=token_range, rollout_is_cap=CAP, rollout_is_mask=mask)
    logits, tg, A, ref = small_case(5, token_range)
    rows = len(tg)
    on = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), np.zeros(rows), None,
                     PolicyLossConfig(temperature=0.8, token_range=token_range)).logp
    q, mu = place(on, tg, level, norm, given)
    got = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), None if q is None else q.numpy(), ref.numpy(), cfg,
                      group_rows=GROUP_ROWS, behaviour_logprobs=mu.numpy())
    check_clear_and_mixed(got, cfg)
    if given:
        assert got.clipped.any() and (got.valid & ~got.clipped).any()
    leaf = logits.clone().requires_grad_(True)
    loss, stats, is_stats, lam, w = restated(leaf, tg, A, q, mu, ref, cfg)
    (grad,) = torch.autograd.grad(loss, leaf)
    scale = grad.abs().max().item()
    assert scale > 0 and np.abs(got.dlogits - grad.numpy()).max() <= 1e-9 * scale
    assert abs(got.loss - loss.item()) <= 1e-12 * max(abs(loss.item()), 1.0)
    for i, name in enumerate(STAT_NAMES):
        assert abs(got.stats[i] - float(stats[name])) <= 1e-12 * max(abs(float(stats[name])), 1.0), name
    assert got.is_stats.shape == (8,) and (got.is_stats[6:] == 0).all()
    for i, name in enumerate(IS_STAT_NAMES):
        assert abs(got.is_stats[i] - float(is_stats[name])) <= 1e-12 * max(abs(float(is_stats[name])), 1.0), name
    assert np.abs(got.log_rho - lam.numpy()).max() <= 1e-12 and np.abs(got.weight - w.numpy()).max() <= 1e-12
    v = got.valid
    assert (got.log_rho[~v] == 0).all() and (got.weight[~v] == 0).all() and not got.masked[~v].any() and not got.truncated[~v].any()
    assert got.stats[1] == v.sum() == sum(COUNTS)                              # a masked row still counts
    if token_range is not None:
        outside = np.ones(N, dtype=bool)
        outside[token_range[0]:token_range[0] + token_range[1]] = False
        assert (got.dlogits[:, outside] == 0).all()
    if level == "action":                                                      # every valid row of a group carries the group's values
        for idx in units_of(tg, "action"):
            assert len(set(got.log_rho[idx])) == 1 and len(set(got.weight[idx])) == 1
            assert np.exp(got.log_rho[idx[0]]) == pytest.approx(WANT_RHO[idx[0] // GROUP_ROWS], rel=1e-9)


@pytest.mark.parametrize("cap", [1.0, 7.5, float("inf")])
@pytest.mark.parametrize("level,norm", [("token", "sum"), ("action", "sum"), ("action", "mean")])
def test_behaviour_equal_to_proximal_is_the_uncorrected_loss_exactly(level, norm, cap):
    base = dict(temperature=0.7, clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.1, ratio_level=level, ratio_norm=norm)
    logits, tg, A, ref = small_case(9)
    on = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), np.zeros(len(tg)), None, PolicyLossConfig(temperature=0.7)).logp
    q, _ = place(on, tg, level, norm, True)
    args = (logits.numpy(), tg.numpy(), A.numpy(), q.numpy(), ref.numpy())
    plain = policy_loss(*args, PolicyLossConfig(**base), group_rows=GROUP_ROWS)
    same = policy_loss(*args, PolicyLossConfig(rollout_is_cap=cap, **base), group_rows=GROUP_ROWS, behaviour_logprobs=q.numpy())
    assert plain.clipped.any() and (plain.valid & ~plain.clipped).any() and plain.weight is None and plain.is_stats is None
    for name in FIELDS:
        assert np.array_equal(getattr(same, name), getattr(plain, name)), name
    if level == "action":
        assert np.array_equal(same.group_stats, plain.group_stats)
    v = same.valid
    assert (same.log_rho == 0).all() and np.array_equal(same.weight, v.astype(np.float64))
    assert np.array_equal(same.is_stats, [1, 1, 0, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("level,norm", [("token", "sum"), ("action", "sum"), ("action", "mean")])
def test_self_proximal_has_ratio_one_and_the_weighted_advantage_as_gradient(level, norm):
    cfg = PolicyLossConfig(temperature=0.8, clip_low=0.02, clip_high=0.03, kl_coef=0.1, ratio_level=level, ratio_norm=norm,
                           rollout_is_cap=CAP, rollout_is_mask=MASK)
    logits, tg, A, ref = small_case(11)
    on = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), np.zeros(len(tg)), None, PolicyLossConfig(temperature=0.8)).logp
    _, mu = place(on, tg, level, norm, False)
    got = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), None, ref.numpy(), cfg, group_rows=GROUP_ROWS,
                      behaviour_logprobs=mu.numpy())
    check_clear_and_mixed(got, cfg)
    v = got.valid
    assert (got.ratio[v] == 1).all() and not got.clipped.any()                 # however tight the clip
    assert got.stats[STAT_NAMES.index("ratio")] == 1 and got.stats[STAT_NAMES.index("clip_frac")] == 0
    assert got.stats[STAT_NAMES.index("approx_kl")] == 0
    kl_share = -cfg.kl_coef * np.expm1(ref.numpy() - got.logp)
    want = np.zeros(len(tg))
    for idx in units_of(tg, level):
        c = 1.0 / len(idx) if norm == "mean" else 1.0
        want[idx] = c * sum(got.weight[idx[0]] * -A.numpy()[j] for j in idx)
    assert np.abs(got.g[v] - (want + kl_share)[v]).max() <= 1e-14
    assert np.array_equal(got.pg[v], (got.weight * -A.numpy())[v])
    # the same numbers as an explicit proximal policy equal to this forward's logp
    explicit = policy_loss(logits.numpy(), tg.numpy(), A.numpy(), got.logp, ref.numpy(), cfg, group_rows=GROUP_ROWS,
                           behaviour_logprobs=mu.numpy())
    assert np.array_equal(explicit.weight, got.weight) and np.array_equal(explicit.dlogits, got.dlogits)


def test_config_and_argument_validation():
    for bad in (dict(rollout_is_cap=0.0), dict(rollout_is_cap=-1.0), dict(rollout_is_cap=float("nan")),
                dict(rollout_is_mask=(0.5, 2.0)), dict(rollout_is_cap=2.0, rollout_is_mask=(1.0, 1.0)),
                dict(rollout_is_cap=2.0, rollout_is_mask=(-0.1, 2.0)), dict(rollout_is_cap=2.0, rollout_is_mask=(2.0, 1.0)),
                dict(rollout_is_cap=2.0, rollout_is_mask=(float("nan"), 1.0)), dict(rollout_is_cap=2.0, rollout_is_mask=(0.5,)),
                dict(rollout_is_cap=2.0, rollout_is_mask=0.5), dict(rollout_is_cap=2.0, rollout_is_mask=(0.5, float("nan")))):
        with pytest.raises(ValueError):
            PolicyLossConfig(**bad)
    d = PolicyLossConfig()
    assert d.rollout_is_cap is None and d.rollout_is_mask is None
    ok = PolicyLossConfig(rollout_is_cap=float("inf"), rollout_is_mask=(0, float("inf")))
    assert ok.rollout_is_cap == float("inf") and ok.rollout_is_mask == (0.0, float("inf"))
    logits, tg, A, ref = small_case(1)
    rows = len(tg)
    q = mu = np.full(rows, -2.0)
    args = (logits.numpy(), tg.numpy(), A.numpy())
    on, off = PolicyLossConfig(rollout_is_cap=2.0), PolicyLossConfig()
    with pytest.raises(ValueError):
        policy_loss(*args, q, None, off, behaviour_logprobs=mu)                # μ without the correction
    with pytest.raises(ValueError):
        policy_loss(*args, None, None, off)                                    # self-proximal without the correction
    with pytest.raises(ValueError):
        policy_loss(*args, q, None, on)                                        # the correction without μ
    with pytest.raises(ValueError):
        policy_loss(*args, q, None, on, behaviour_logprobs=mu[:-1])
    valid = tg.numpy() != IGNORE_INDEX
    for poison in (-np.inf, np.nan, np.inf):
        bad = mu.copy()
        bad[np.argmax(valid)] = poison
        with pytest.raises(ValueError, match="behaviour_logprobs"):
            policy_loss(*args, q, None, on, behaviour_logprobs=bad)
        with pytest.raises(ValueError, match="behaviour_logprobs"):
            policy_loss(*args, None, None, PolicyLossConfig(rollout_is_cap=2.0, token_range=(0, 16)), behaviour_logprobs=bad)
        fine = mu.copy()
        fine[~valid] = poison                                                  # never read on ignored rows
        a, b = policy_loss(*args, q, None, on, behaviour_logprobs=fine), policy_loss(*args, q, None, on, behaviour_logprobs=mu)
        assert np.array_equal(a.dlogits, b.dlogits) and np.array_equal(a.is_stats, b.is_stats)


def test_policy_batch_keys():
    prompt = torch.tensor([[1, 5, 6, 29871], [1, 7, 29871, 32000]])
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 1, 0]])
    tok = torch.tensor([[31800, 31801], [31900, 31901]])
    lp = torch.tensor([[-1.0, -2.0], [-3.0, -4.0]])
    prox = lp + 0.25
    adv = torch.tensor([0.5, -0.5])
    plain = policy_batch(prompt, mask, tok, lp, adv)
    assert list(plain) == ["input_ids", "attention_mask", "labels", "advantages", "old_logprobs"]
    again = policy_batch(prompt, mask, tok, lp, adv, rollout_is=False, proximal_logprobs=None)
    assert list(again) == list(plain) and all(torch.equal(again[k], plain[k]) for k in plain)
    self_prox = policy_batch(prompt, mask, tok, lp, adv, rollout_is=True)
    assert list(self_prox) == ["input_ids", "attention_mask", "labels", "advantages", "behaviour_logprobs"]
    assert torch.equal(self_prox["behaviour_logprobs"], plain["old_logprobs"])
    assert all(torch.equal(self_prox[k], plain[k]) for k in ("input_ids", "attention_mask", "labels", "advantages"))
    given = policy_batch(prompt, mask, tok, lp, adv, rollout_is=True, proximal_logprobs=prox, values=torch.tensor([0.1, 0.2]))
    assert set(given) == {"input_ids", "attention_mask", "labels", "advantages", "old_logprobs", "behaviour_logprobs", "old_values"}
    assert torch.equal(given["behaviour_logprobs"], plain["old_logprobs"])
    lab = given["labels"] != IGNORE_INDEX
    assert torch.equal(given["old_logprobs"][lab], prox.reshape(-1)) and (given["old_logprobs"][~lab] == 0).all()
    with pytest.raises(ValueError):
        policy_batch(prompt, mask, tok, lp, adv, proximal_logprobs=prox)       # a proximal policy without the correction
    with pytest.raises(ValueError):
        policy_batch(prompt, mask, tok, lp, adv, rollout_is=True, proximal_logprobs=prox[:, :1])
    with pytest.raises(ValueError):
        policy_batch(prompt, mask, tok, lp, adv, rollout_is=True, proximal_logprobs=torch.full((2, 2), float("-inf")))


def test_entry_point_is_declared_bound_and_exported():
    from bridgelang_amd import _lib
    name = "bl_policy_loss_is_f32"
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    proto = re.search(rf"\bint {name}\(([^;]*)\);", header)
    assert proto is not None and name in _lib.SIGNATURES
    params = [p.strip() for p in proto.group(1).split(",")]
    argtypes = _lib.SIGNATURES[name][1]
    assert len(params) == len(argtypes) == 28                                  # the grouped forward's 22, then μ, 3 + 2 more
    assert [p.split()[-1] for p in params[7:10]] == ["old_logprob", "behaviour_logprob", "ref_logprob"]
    assert [p.split()[-1] for p in params[-6:]] == ["is_cap", "is_mask_low", "is_mask_high", "is_rows", "is_stats", "stream"]
    grouped = _lib.SIGNATURES["bl_policy_loss_grouped_f32"][1]
    assert argtypes[:8] == grouped[:8] and argtypes[9:22] == grouped[8:21]     # μ is inserted behind old_logprob
    pointer = lambda p: "*" in p
    assert [pointer(p) for p in params] == [t is _lib.SIGNATURES[name][1][0] for t in argtypes]      # pointers where c_void_p is
    lib = _lib.load()
    assert hasattr(lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    assert name in {line.split()[-1] for line in out.splitlines()}
