"""The clipped-surrogate policy-gradient loss of the training step: the host SPECIFICATION (numpy, fp64) of
`bl_policy_loss_f32` / `bl_policy_loss_backward_f32` (csrc/policy.hip).

The host file is the definition and the kernels are its twin, as `sampling.py` ↔ `bl_sample_f32`; here the twin holds to a
tolerance, not bit for bit, because the kernels use `expf` / `logf` as the cross-entropy kernels do.

Rows are the step's logits rows (bf16-rounded fp32), with cross-entropy's row convention: `targets[r]` is the token of
the NEXT position, `IGNORE_INDEX` rows contribute nothing. Per valid row r with logits l[0..n), token a, advantage A,
behaviour log-probability q and (optionally) a reference policy's log-probability ref:

    z_i    = l_i / T                     m = max z      S = Σ exp(z_i − m)
    logp_i = z_i − m − log S             logp = logp_a  p_i = exp(logp_i)
    H      = −Σ p_i · logp_i             (full row; a term with p_i = 0 is 0)
    ratio  = exp(logp − q)
    pg     = −min(ratio·A, clip(ratio, 1 − clip_low, 1 + clip_high)·A)
    active = (A ≥ 0 and ratio ≤ 1 + clip_high) or (A < 0 and ratio ≥ 1 − clip_low)
    kl     = exp(ref − logp) − (ref − logp) − 1                      (the k3 estimator; 0 without ref)
    row_loss = pg − entropy_coef·H + kl_coef·kl
    loss   = Σ_valid row_loss / n_valid
    g      = ∂row_loss/∂logp = −A·ratio·[active] + kl_coef·(1 − exp(ref − logp))
    dlogits_i = [ g·(δ_ia − p_i) + entropy_coef·p_i·(logp_i + H) ] / (T · n_valid)

`active` is where the surrogate still has a gradient: `clamp` passes its gradient at the boundary, as torch does, and
`min` of two equal values takes either (they have the same gradient there unless the ratio sits exactly on a boundary).

Preconditions: finite logits; on valid rows finite A, q and ref — the host entry points raise ValueError otherwise. The
case that matters in practice is the -inf `score_actions` reports for a token outside a top-k / top-p support. Top-k and
top-p warping are NOT part of this loss: log π here is the temperature-only softmax, so rollouts meant for training are
drawn with temperature only (top_k = 0, top_p = 1).

A token range IS part of it. With `PolicyLossConfig.token_range = (first, count)` the policy is the softmax of
`l[first : first + count]` alone — the restricted policy of `sampling.py` (`vocab=`): the definition above on the sliced
rows with the targets shifted by `first`, so m, S, H, logp and p_i are all over the range, `dlogits` is exactly 0 in every
column outside it, and no logit outside it is read. A valid row whose target lies outside the range is an error: that
action has probability 0 and the loss is undefined. Sampler, scorer and loss must describe ONE distribution or the ratio
of an on-policy step is not 1: `temperature` and `token_range` here must be the rollout's (`action_tokens_only=True` on
`sample_actions` / `score_actions` ↔ `token_range = model.action_token_range()`).

The ratio LEVEL is part of it too. An OpenVLA action is the n consecutive action tokens of a sequence: drawn together,
rewarded together, given one advantage. With `PolicyLossConfig.ratio_level = "action"` (`bl_policy_loss_grouped_f32`) the
importance ratio is the action's, π(a)/π_old(a), clipped once, instead of one ratio per token. `group_rows` consecutive
rows are one sequence and its group G is the set of its valid rows (labels cover exactly the sampled action, and the shift
never crosses a sequence, so no index tensor is needed). With δ_r = logp_r − q_r, n_G = |G| and c = 1 (`ratio_norm =
"sum"`, PPO's action ratio) or 1 / n_G (`"mean"`, the geometric mean of the token ratios: GSPO's sequence ratio):

    s_G      = c · Σ_{r∈G} δ_r                 (summed in row order)
    ratio_G  = exp(s_G)
    for r ∈ G:
      pg_r     = −min(ratio_G·A_r, clip(ratio_G, 1 − clip_low, 1 + clip_high)·A_r)
      active_r = (A_r ≥ 0 and ratio_G ≤ 1 + clip_high) or (A_r < 0 and ratio_G ≥ 1 − clip_low)
      kl_r, H_r as above (per token)
      row_loss_r = pg_r − entropy_coef·H_r + kl_coef·kl_r
      g_r      = c · Σ_{j∈G} (−A_j · ratio_G · [active_j]) + kl_coef·(1 − exp(ref_r − logp_r))
    loss, dlogits as above (a token mean; dlogits with this g_r)

`ratio` holds ratio_G on every row of G, `clipped` is valid and not active_r, the statistics `ratio`, `approx_kl` and
`clip_frac` are means over valid rows of ratio_G, expm1(s_G) − s_G and not active_r, and `group_stats` reports
GROUP_STAT_NAMES per sequence (zeros for a sequence without a valid row, which contributes nothing). Groups of one row are
the token-level loss exactly. With `"sum"` and the token-mean loss a group's surrogate is counted n_G times: harmless when
every action has the same number of tokens (OpenVLA: 7), but with ragged groups longer actions weigh more — `"mean"`, or
advantages scaled by 1 / n_G, if that is not wanted.

The ROLLOUT CORRECTION is part of it as well (`PolicyLossConfig.rollout_is_cap`, `bl_policy_loss_is_f32`): decoupled PPO with
a truncated importance weight. The policy that DREW the tokens (the decode engine, perhaps through the e4m3 prefill) is not
the policy the learner differentiates, so a row has two log-probabilities: the behaviour one μ_r (`behaviour_logprobs`, what
the sampler reported) and the proximal one q_r the clip is centred on. q_r is `old_logprobs`, exactly as above, or with
`old_logprobs=None` (self-proximal, allowed only with the correction on) the logp_r of THIS forward taken as a constant:
the log ratio is then 0 exactly, the ratio 1 and every row active. With cap = `rollout_is_cap` (> 0, may be inf) and
(low, high) = `rollout_is_mask` (0 ≤ low < high, high may be inf; None: no mask), at token level

    λ_r = q_r − μ_r          ρ_r = exp(λ_r)
    masked_r    = ρ_r < low or ρ_r > high
    w_r         = 0 if masked_r else min(ρ_r, cap)
    truncated_r = not masked_r and ρ_r > cap
    pg_r = w_r · (−min(ratio·A, clip(ratio)·A))
    g_r  = w_r · (−A·ratio·[active]) + the unchanged KL share

and at action level the weight is formed at the level of the ratio, with its norm c: λ_G = c·Σ_{r∈G} (q_r − μ_r) in row
order, ρ_G, w_G, masked_G and truncated_G from λ_G as above on every valid row of G, and
g_r = c·Σ_{j∈G} w_G·(−A_j·ratio_G·[active_j]) + KL share. w is a CONSTANT in both modes (no gradient flows through it, nor
through the self-proximal q); the entropy and KL terms are not weighted; a masked row still counts in n_valid, so masking
shrinks the gradient instead of renormalising it. `stats` keeps its layout: `pg` and `loss` are the weighted ones, `ratio`,
`clip_frac` and `approx_kl` stay about π_θ/π_prox. `is_stats` (IS_STAT_NAMES) are means over valid rows of w, ρ, truncated,
masked, ρ − 1 − λ (the k3 estimate of KL(μ‖π_prox)) and −λ (k1), then two zero slots. μ must be finite on valid rows.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

IGNORE_INDEX = -100

# the step statistics vector (fp32 [8]); slots 0 and 1 are cross-entropy's mean_and_count
STAT_NAMES = ("loss", "n_valid", "pg", "entropy", "kl", "clip_frac", "approx_kl", "ratio")
# the per-row statistics (fp32 [rows, 8]): five reported values, then what the backward kernel needs
ROW_STAT_NAMES = ("logp", "entropy", "ratio", "row_loss", "clipped", "m", "log_s", "g")
# the per-sequence statistics of the action-level ratio (fp32 [groups, 4]): s_G, ratio_G, n_G, Σ_G logp
GROUP_STAT_NAMES = ("log_ratio", "ratio", "n", "logp")
# the step statistics of the rollout correction (fp32 [8]): means over valid rows; slots 6 and 7 are zero and have no name
IS_STAT_NAMES = ("weight", "rho", "trunc_frac", "mask_frac", "rollout_kl", "rollout_k1")


@dataclass(frozen=True)
class PolicyLossConfig:
    temperature: float = 1.0
    clip_low: float = 0.2
    clip_high: float = 0.2
    entropy_coef: float = 0.0
    kl_coef: float = 0.0
    token_range: Optional[Tuple[int, int]] = None    # (first, count): the policy is over these tokens alone
    ratio_level: str = "token"                       # "token": one ratio per token; "action": one per sequence's labelled tokens
    ratio_norm: str = "sum"                          # action level: exp(Σ δ) ("sum") or exp(Σ δ / n_G) ("mean")
    rollout_is_cap: Optional[float] = None           # set: the rollout correction is on, w = min(π_prox / μ, cap); may be inf
    rollout_is_mask: Optional[Tuple[float, float]] = None    # (low, high): w = 0 where π_prox / μ leaves [low, high]

    def __post_init__(self):
        if self.rollout_is_cap is not None:
            cap = float(self.rollout_is_cap)
            if not cap > 0:
                raise ValueError(f"PolicyLossConfig: rollout_is_cap is None or > 0 (inf: no truncation), got {self.rollout_is_cap!r}")
            object.__setattr__(self, "rollout_is_cap", cap)
        if self.rollout_is_mask is not None:
            if self.rollout_is_cap is None:
                raise ValueError("PolicyLossConfig: rollout_is_mask needs rollout_is_cap (the correction it masks)")
            try:
                low, high = (float(v) for v in self.rollout_is_mask)
            except (TypeError, ValueError):
                low, high = 1.0, 0.0
            if not 0 <= low < high:
                raise ValueError("PolicyLossConfig: rollout_is_mask is None or (low, high) with 0 <= low < high (high may be inf)")
            object.__setattr__(self, "rollout_is_mask", (low, high))
        if self.ratio_level not in ("token", "action"):
            raise ValueError(f"PolicyLossConfig: ratio_level is 'token' or 'action', got {self.ratio_level!r}")
        if self.ratio_norm not in ("sum", "mean"):
            raise ValueError(f"PolicyLossConfig: ratio_norm is 'sum' or 'mean', got {self.ratio_norm!r}")
        if self.ratio_norm == "mean" and self.ratio_level != "action":
            raise ValueError("PolicyLossConfig: ratio_norm='mean' goes with ratio_level='action' (a token is its own mean)")
        if self.token_range is not None:
            try:
                first, count = (int(v) for v in self.token_range)
                exact = (first, count) == tuple(self.token_range)
            except (TypeError, ValueError):
                exact = False
            if not exact or first < 0 or count < 1:
                raise ValueError("PolicyLossConfig: token_range is None or (first, count) with first >= 0 and count >= 1")
            object.__setattr__(self, "token_range", (first, count))
        if not (np.isfinite(self.temperature) and self.temperature > 0):
            raise ValueError("PolicyLossConfig: temperature must be > 0 (a greedy rollout has no policy gradient)")
        if not (0 <= self.clip_low < 1 and 0 <= self.clip_high and np.isfinite(self.clip_high)):
            raise ValueError("PolicyLossConfig: 0 <= clip_low < 1 and 0 <= clip_high")
        if not (np.isfinite(self.entropy_coef) and np.isfinite(self.kl_coef)):
            raise ValueError("PolicyLossConfig: entropy_coef and kl_coef must be finite")


def check_finite(valid, **named) -> None:
    """ValueError if any named array (None is skipped) is not finite where `valid` is set."""
    valid = np.asarray(valid, dtype=bool)
    for name, v in named.items():
        if v is None:
            continue
        v = np.asarray(v, dtype=np.float64)
        if v.shape != valid.shape:
            raise ValueError(f"{name}: shape {v.shape}, expected {valid.shape}")
        bad = valid & ~np.isfinite(v)
        if bad.any():
            raise ValueError(f"{name}: {int(bad.sum())} non-finite value(s) on labelled positions (first at {tuple(np.argwhere(bad)[0])}): "
                             "a token outside the rollout's top-k / top-p support scores -inf — draw training rollouts with temperature only")


@dataclass
class PolicyLossResult:
    logp: np.ndarray          # [rows]  log π(a); 0 on ignored rows, as every per-row array
    entropy: np.ndarray       # [rows]  H
    ratio: np.ndarray
    pg: np.ndarray
    kl: np.ndarray
    row_loss: np.ndarray
    clipped: np.ndarray       # [rows]  bool: valid and not active
    valid: np.ndarray         # [rows]  bool
    g: np.ndarray
    loss: float
    stats: np.ndarray         # [8] fp64, STAT_NAMES
    dlogits: np.ndarray       # [rows, n] fp64
    group_stats: Optional[np.ndarray] = None      # [groups, 4] fp64, GROUP_STAT_NAMES (action level only)
    log_rho: Optional[np.ndarray] = None          # [rows]  λ = q − μ (the group's at action level); these five with the
    weight: Optional[np.ndarray] = None           # [rows]  w                                        rollout correction only
    masked: Optional[np.ndarray] = None           # [rows]  bool
    truncated: Optional[np.ndarray] = None        # [rows]  bool
    is_stats: Optional[np.ndarray] = None         # [8] fp64, IS_STAT_NAMES


def _group_sums(v, valid, group_rows: int):
    """[rows] → ([groups] sums of v over each group's valid rows, accumulated in row order; [groups] valid counts)."""
    groups = v.shape[0] // group_rows
    sums, counts = np.zeros(groups), np.zeros(groups, dtype=np.int64)
    for k in range(groups):
        sl = slice(k * group_rows, (k + 1) * group_rows)
        vk = v[sl][valid[sl]]
        counts[k] = vk.size
        if vk.size:
            sums[k] = np.add.accumulate(vk)[-1]
    return sums, counts


def row_softmax(l, T: float):
    """z = l / T → (logp_i [rows, n], p_i [rows, n], H [rows]) of the definition above, for every row of fp64 `l`."""
    z = l / T
    m = z.max(axis=1, keepdims=True)
    S = np.exp(z - m).sum(axis=1, keepdims=True)
    logp_all = z - m - np.log(S)
    p = np.exp(logp_all)
    H = -(p * logp_all).sum(axis=1)               # p = 0 (underflow) times a finite logp is 0
    return logp_all, p, H


def slice_range(logits, targets, token_range, ignore_index: int, what: str):
    """The rows restricted to token_range = (first, count): (logits[:, first : first + count], targets shifted by first).
    ValueError if the range leaves the row or a valid target lies outside it."""
    first, count = token_range
    n = np.shape(logits)[1]
    if first + count > n:
        raise ValueError(f"{what}: token_range [{first}, {first + count}) leaves [0, {n})")
    tg = np.asarray(targets, dtype=np.int64)
    valid = tg != ignore_index
    outside = valid & ((tg < first) | (tg >= first + count))
    if outside.any():
        raise ValueError(f"{what}: {int(outside.sum())} target(s) outside token_range [{first}, {first + count}) "
                         f"(first at row {int(np.argmax(outside))}): that action has probability 0 under the restricted policy")
    return np.asarray(logits)[:, first:first + count], np.where(valid, tg - first, ignore_index)


def policy_loss(logits, targets, advantages, old_logprobs, ref_logprobs=None, cfg: Optional[PolicyLossConfig] = None,
                ignore_index: int = IGNORE_INDEX, group_rows: Optional[int] = None, behaviour_logprobs=None) -> PolicyLossResult:
    """`group_rows`: rows per sequence, needed (and dividing the row count) with cfg.ratio_level == "action"; ignored at
    token level. `behaviour_logprobs`: μ of the rollout correction, given iff cfg.rollout_is_cap is set; `old_logprobs` may
    then be None (self-proximal)."""
    cfg = cfg or PolicyLossConfig()
    by_action = cfg.ratio_level == "action"
    corrected = cfg.rollout_is_cap is not None
    if corrected != (behaviour_logprobs is not None):
        raise ValueError("policy_loss: behaviour_logprobs goes together with cfg.rollout_is_cap")
    if old_logprobs is None and not corrected:
        raise ValueError("policy_loss: old_logprobs=None (self-proximal) needs the rollout correction (cfg.rollout_is_cap)")
    if by_action:
        rows = np.shape(logits)[0]
        if group_rows is None or int(group_rows) != group_rows or group_rows < 1 or rows % int(group_rows):
            raise ValueError(f"policy_loss: ratio_level='action' needs group_rows >= 1 dividing the {rows} rows, got {group_rows!r}")
        group_rows = int(group_rows)
    if cfg.token_range is not None:
        return _policy_loss_range(logits, targets, advantages, old_logprobs, ref_logprobs, cfg, ignore_index, group_rows,
                                  behaviour_logprobs)
    l = np.asarray(logits, dtype=np.float64)
    tg = np.asarray(targets, dtype=np.int64)
    rows, n = l.shape
    valid = tg != ignore_index
    if not np.isfinite(l).all():
        raise ValueError("policy_loss: logits must be finite")
    if valid.any() and (tg[valid].min() < 0 or tg[valid].max() >= n):
        raise ValueError(f"policy_loss: targets must lie in [0, {n}) or be {ignore_index}")
    check_finite(valid, advantages=advantages, old_logprobs=old_logprobs, ref_logprobs=ref_logprobs,
                 behaviour_logprobs=behaviour_logprobs)
    A = np.where(valid, np.asarray(advantages, dtype=np.float64), 0.0)
    ref = None if ref_logprobs is None else np.where(valid, np.asarray(ref_logprobs, dtype=np.float64), 0.0)
    T = float(cfg.temperature)
    logp_all, p, H = row_softmax(l, T)
    a = np.where(valid, tg, 0)
    logp = logp_all[np.arange(rows), a]
    q = np.where(valid, logp if old_logprobs is None else np.asarray(old_logprobs, dtype=np.float64), 0.0)   # self-proximal: a constant
    lr = np.where(valid, logp, 0.0) - q
    lam = np.where(valid, q - np.asarray(behaviour_logprobs, dtype=np.float64), 0.0) if corrected else None
    group_stats = None
    if by_action:                                 # every valid row takes its group's log-ratio s_G = c·Σ δ
        sums, n_g = _group_sums(lr, valid, group_rows)
        c_g = 1.0 / np.maximum(n_g, 1) if cfg.ratio_norm == "mean" else np.ones(len(n_g))
        s_g = c_g * sums
        lr = np.where(valid, np.repeat(s_g, group_rows), 0.0)
        group_stats = np.stack([s_g, np.where(n_g > 0, np.exp(s_g), 0.0), n_g.astype(np.float64),
                                _group_sums(logp, valid, group_rows)[0]], axis=1)
        if corrected:                             # … and, with the correction, its group's λ_G = c·Σ (q − μ)
            lam = np.where(valid, np.repeat(c_g * _group_sums(lam, valid, group_rows)[0], group_rows), 0.0)
    w = np.ones(rows)
    if corrected:
        low, high = cfg.rollout_is_mask or (0.0, np.inf)
        rho = np.exp(lam)
        masked = valid & ((rho < low) | (rho > high))
        truncated = valid & ~masked & (rho > cfg.rollout_is_cap)
        w = np.where(masked, 0.0, np.minimum(rho, cfg.rollout_is_cap))
    ratio = np.exp(lr)
    lo, hi = 1.0 - cfg.clip_low, 1.0 + cfg.clip_high
    pg = -np.minimum(ratio * A, np.clip(ratio, lo, hi) * A)
    active = ((A >= 0) & (ratio <= hi)) | ((A < 0) & (ratio >= lo))
    g = np.where(active, -A * ratio, 0.0)
    if corrected:                                 # w is a constant factor of the surrogate (a group's rows share w_G)
        pg, g = w * pg, w * g
    if by_action:                                 # … and its group's surrogate gradient c·Σ_j −A_j·ratio_G·[active_j]
        g = np.repeat(c_g * _group_sums(g, valid, group_rows)[0], group_rows)
    kl = np.zeros(rows)
    if ref is not None:
        d = ref - logp
        kl = np.expm1(d) - d
        g = g - cfg.kl_coef * np.expm1(d)
    row_loss = pg - cfg.entropy_coef * H + cfg.kl_coef * kl
    nv = int(valid.sum())
    onehot = np.zeros_like(l)
    onehot[np.arange(rows), a] = 1.0
    dl = np.zeros_like(l)
    if nv:
        dl = (g[:, None] * (onehot - p) + cfg.entropy_coef * p * (logp_all + H[:, None])) / (T * nv)
        dl[~valid] = 0.0
    zero = lambda v: np.where(valid, v, 0.0)
    mean = lambda v: float(v[valid].sum() / nv) if nv else 0.0
    stats = np.array([mean(row_loss), nv, mean(pg), mean(H), mean(kl), mean((~active).astype(np.float64)),
                      mean(np.expm1(lr) - lr), mean(ratio)], dtype=np.float64)
    res = PolicyLossResult(logp=zero(logp), entropy=zero(H), ratio=zero(ratio), pg=zero(pg), kl=zero(kl), row_loss=zero(row_loss),
                           clipped=valid & ~active, valid=valid, g=zero(g), loss=stats[0], stats=stats, dlogits=dl,
                           group_stats=group_stats)
    if corrected:
        res.log_rho, res.weight, res.masked, res.truncated = zero(lam), zero(w), masked, truncated
        res.is_stats = np.array([mean(w), mean(rho), mean(truncated.astype(np.float64)), mean(masked.astype(np.float64)),
                                 mean(np.expm1(lam) - lam), mean(-lam), 0.0, 0.0], dtype=np.float64)
    return res


def _policy_loss_range(logits, targets, advantages, old_logprobs, ref_logprobs, cfg: PolicyLossConfig, ignore_index: int,
                       group_rows: Optional[int] = None, behaviour_logprobs=None) -> PolicyLossResult:
    """`policy_loss` on logits[:, first : first + count] with the targets shifted by `first`; dlogits widened with zeros."""
    import dataclasses
    first, count = cfg.token_range
    n = np.shape(logits)[1]
    sliced, shifted = slice_range(logits, targets, cfg.token_range, ignore_index, "policy_loss")     # only the range is looked at
    res = policy_loss(sliced, shifted, advantages, old_logprobs, ref_logprobs,
                      dataclasses.replace(cfg, token_range=None), ignore_index, group_rows, behaviour_logprobs)
    dl = np.zeros((sliced.shape[0], n), dtype=np.float64)
    dl[:, first:first + count] = res.dlogits
    res.dlogits = dl
    return res
