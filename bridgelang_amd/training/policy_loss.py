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


@dataclass(frozen=True)
class PolicyLossConfig:
    temperature: float = 1.0
    clip_low: float = 0.2
    clip_high: float = 0.2
    entropy_coef: float = 0.0
    kl_coef: float = 0.0
    token_range: Optional[Tuple[int, int]] = None    # (first, count): the policy is over these tokens alone

    def __post_init__(self):
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


def policy_loss(logits, targets, advantages, old_logprobs, ref_logprobs=None, cfg: Optional[PolicyLossConfig] = None,
                ignore_index: int = IGNORE_INDEX) -> PolicyLossResult:
    cfg = cfg or PolicyLossConfig()
    if cfg.token_range is not None:
        return _policy_loss_range(logits, targets, advantages, old_logprobs, ref_logprobs, cfg, ignore_index)
    l = np.asarray(logits, dtype=np.float64)
    tg = np.asarray(targets, dtype=np.int64)
    rows, n = l.shape
    valid = tg != ignore_index
    if not np.isfinite(l).all():
        raise ValueError("policy_loss: logits must be finite")
    if valid.any() and (tg[valid].min() < 0 or tg[valid].max() >= n):
        raise ValueError(f"policy_loss: targets must lie in [0, {n}) or be {ignore_index}")
    check_finite(valid, advantages=advantages, old_logprobs=old_logprobs, ref_logprobs=ref_logprobs)
    A = np.where(valid, np.asarray(advantages, dtype=np.float64), 0.0)
    q = np.where(valid, np.asarray(old_logprobs, dtype=np.float64), 0.0)
    ref = None if ref_logprobs is None else np.where(valid, np.asarray(ref_logprobs, dtype=np.float64), 0.0)
    T = float(cfg.temperature)
    z = l / T
    m = z.max(axis=1, keepdims=True)
    S = np.exp(z - m).sum(axis=1, keepdims=True)
    logp_all = z - m - np.log(S)
    p = np.exp(logp_all)
    H = -(p * logp_all).sum(axis=1)               # p = 0 (underflow) times a finite logp is 0
    a = np.where(valid, tg, 0)
    logp = logp_all[np.arange(rows), a]
    ratio = np.exp(logp - q)
    lo, hi = 1.0 - cfg.clip_low, 1.0 + cfg.clip_high
    pg = -np.minimum(ratio * A, np.clip(ratio, lo, hi) * A)
    active = ((A >= 0) & (ratio <= hi)) | ((A < 0) & (ratio >= lo))
    g = np.where(active, -A * ratio, 0.0)
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
    lr = logp - q
    stats = np.array([mean(row_loss), nv, mean(pg), mean(H), mean(kl), mean((~active).astype(np.float64)),
                      mean(np.expm1(lr) - lr), mean(ratio)], dtype=np.float64)
    return PolicyLossResult(logp=zero(logp), entropy=zero(H), ratio=zero(ratio), pg=zero(pg), kl=zero(kl), row_loss=zero(row_loss),
                            clipped=valid & ~active, valid=valid, g=zero(g), loss=stats[0], stats=stats, dlogits=dl)


def _policy_loss_range(logits, targets, advantages, old_logprobs, ref_logprobs, cfg: PolicyLossConfig, ignore_index: int) -> PolicyLossResult:
    """`policy_loss` on logits[:, first : first + count] with the targets shifted by `first`; dlogits widened with zeros."""
    import dataclasses
    first, count = cfg.token_range
    n = np.shape(logits)[1]
    if first + count > n:
        raise ValueError(f"policy_loss: token_range [{first}, {first + count}) leaves [0, {n})")
    tg = np.asarray(targets, dtype=np.int64)
    valid = tg != ignore_index
    outside = valid & ((tg < first) | (tg >= first + count))
    if outside.any():
        raise ValueError(f"policy_loss: {int(outside.sum())} target(s) outside token_range [{first}, {first + count}) "
                         f"(first at row {int(np.argmax(outside))}): that action has probability 0 under the restricted policy")
    sliced = np.asarray(logits)[:, first:first + count]           # only the range is looked at, also by the finiteness check
    res = policy_loss(sliced, np.where(valid, tg - first, ignore_index), advantages, old_logprobs, ref_logprobs,
                      dataclasses.replace(cfg, token_range=None), ignore_index)
    dl = np.zeros((sliced.shape[0], n), dtype=np.float64)
    dl[:, first:first + count] = res.dlogits
    res.dlogits = dl
    return res
