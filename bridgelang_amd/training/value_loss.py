"""The critic of the policy training step: a linear value head on the final-norm output and PPO's clipped value loss — the
host SPECIFICATION (numpy, fp64) of `bl_value_head_f32` / `bl_value_head_backward_f32` (csrc/value.hip).

The host file is the definition and the kernels are its twin to a tolerance (fp32 sums in a documented order), as
`policy_loss.py` ↔ csrc/policy.hip.

Rows are the step's rows, with cross-entropy's convention: `targets[r]` is the token of the NEXT position and `group_rows`
consecutive rows are one sequence. The VALUE ROWS depend on `ValueLossConfig.level`:

    "token"   every valid row (targets[r] != IGNORE_INDEX)
    "action"  the first valid row of each sequence: the position that has seen image and instruction and predicts the first
              action token, i.e. V(s). A sequence without a valid row has none; a sequence with two separate labelled runs
              has one, the first row of its first run.

Per value row r, with hn[r] the (bf16) final-norm output, the head w [D] and b (bf16 values), the return R_r and the value
vo_r the behaviour critic gave the state:

    v   = Σ_k hn[r,k]·w[k] + b
    e   = v − R              vc = vo + clip(v − vo, −c, +c)        ec = vc − R
    l   = ½·max(e², ec²)     (clip None: ½·e²)
    ∂l/∂v = e  if e² ≥ ec²  else 0        clipped = not (e² ≥ ec²)

Inside the clip range vc = v, so the two branches tie and have the same gradient; where the clipped branch is selected,
`clamp` passes no gradient. The tie is taken as exact: for |v − vo| ≤ c, ec is e itself and not vo + (v − vo) − R, whose
rounding could select the clipped branch and its zero gradient (here and in the kernels alike). With n_v the number of
value rows:

    value_loss = Σ l / n_v        total = policy_loss + coef·value_loss
    dv_r  = coef · ∂l/∂v / n_v
    dw[k] = Σ_r dv_r·hn[r,k]      (ascending r)
    db    = Σ_r dv_r
    dhn[r,k] += dv_r·w[k]         (value rows only; nothing with `detach`: the critic then trains on the trunk's features
                                   without shaping them)

n_v = 0 gives loss 0 and every gradient 0 (no division by zero). Values of R and vo on other rows are never read; a
non-finite R or vo on a value row raises ValueError from the host entry points. `inv_world` scales dv (the mean over
data-parallel ranks, which the policy path gets from its n_valid).

Critic warm-up needs no mode of its own: advantages of 0 with entropy_coef = kl_coef = 0 make the policy loss's dlogits
exactly 0, so every trunk gradient is the value path's.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .policy_loss import IGNORE_INDEX, check_finite

# the step statistics vector of the value loss (fp32 [8])
VALUE_STAT_NAMES = ("value_loss", "n", "clip_frac", "value", "return", "explained_var", "abs_err", "total")
# the per-row outputs (fp32 [rows, 4]), zero on rows that are not value rows; `dv` is what the backward kernel reads
VALUE_ROW_NAMES = ("value", "loss", "clipped", "dv")
LEVELS = ("token", "action")


@dataclass(frozen=True)
class ValueLossConfig:
    coef: float = 0.5
    clip: Optional[float] = 0.2        # None: the unclipped ½·(v − R)²
    level: str = "action"              # "action": one value per sequence (its first labelled row); "token": one per labelled row
    detach: bool = False               # True: no gradient from the value loss into the trunk

    def __post_init__(self):
        if self.level not in LEVELS:
            raise ValueError(f"ValueLossConfig: level is 'action' or 'token', got {self.level!r}")
        if not (np.isfinite(self.coef) and self.coef >= 0):
            raise ValueError("ValueLossConfig: coef must be finite and >= 0")
        if self.clip is not None and not (np.isfinite(self.clip) and self.clip > 0):
            raise ValueError("ValueLossConfig: clip is None (unclipped) or a finite value > 0")
        if not isinstance(self.detach, (bool, np.bool_)):
            raise ValueError("ValueLossConfig: detach is a bool")


def value_row_index(targets, level: str, group_rows: Optional[int] = None, ignore_index: int = IGNORE_INDEX) -> np.ndarray:
    """The ascending list (int64) of the value rows of `targets` [rows] at `level`."""
    tg = np.asarray(targets, dtype=np.int64).reshape(-1)
    valid = tg != ignore_index
    if level == "token":
        return np.flatnonzero(valid)
    if level != "action":
        raise ValueError(f"value_row_index: level is 'action' or 'token', got {level!r}")
    rows = tg.shape[0]
    if group_rows is None or int(group_rows) != group_rows or group_rows < 1 or rows % int(group_rows):
        raise ValueError(f"value_row_index: level='action' needs group_rows >= 1 dividing the {rows} rows, got {group_rows!r}")
    v = valid.reshape(-1, int(group_rows))
    has = v.any(axis=1)
    return (np.flatnonzero(has) * int(group_rows) + v.argmax(axis=1)[has]).astype(np.int64)


@dataclass
class ValueLossResult:
    index: np.ndarray         # [n_v] int64: the value rows, ascending
    value: np.ndarray         # [rows] v; 0 off the value rows, as every per-row array
    loss: np.ndarray          # [rows] l
    clipped: np.ndarray       # [rows] bool
    dl_dv: np.ndarray         # [rows] ∂l/∂v
    dv: np.ndarray            # [rows] coef·∂l/∂v / n_v (· inv_world)
    rows: np.ndarray          # [rows, 4] fp64, VALUE_ROW_NAMES
    value_loss: float
    total: float
    stats: np.ndarray         # [8] fp64, VALUE_STAT_NAMES
    dw: np.ndarray            # [D]
    db: float
    dhn: np.ndarray           # [rows, D]: the value loss's own contribution (zeros with detach)


def value_loss(hn, targets, w, b, returns, old_values=None, cfg: Optional[ValueLossConfig] = None,
               group_rows: Optional[int] = None, ignore_index: int = IGNORE_INDEX, policy_loss: float = 0.0,
               inv_world: float = 1.0) -> ValueLossResult:
    """hn [rows, D], w [D], b scalar, returns / old_values [rows] (read on value rows only; old_values None only with
    cfg.clip None). `policy_loss` is the loss `total` adds to."""
    cfg = cfg or ValueLossConfig()
    h = np.asarray(hn)
    rows, D = h.shape
    idx = value_row_index(targets, cfg.level, group_rows, ignore_index)
    if cfg.clip is not None and old_values is None:
        raise ValueError("value_loss: old_values is needed unless cfg.clip is None")
    is_v = np.zeros(rows, dtype=bool)
    is_v[idx] = True
    check_finite(is_v, returns=np.asarray(returns).reshape(-1), old_values=None if old_values is None else np.asarray(old_values).reshape(-1))
    wv = np.asarray(w, dtype=np.float64).reshape(-1)
    if wv.shape[0] != D:
        raise ValueError(f"value_loss: w has {wv.shape[0]} elements, hn rows have {D}")
    bv = float(np.asarray(b, dtype=np.float64).reshape(-1)[0])
    hv = np.asarray(h[idx], dtype=np.float64)                   # rows off the list are never read
    if not np.isfinite(hv).all():
        raise ValueError("value_loss: hn must be finite on the value rows")
    R = np.asarray(returns, dtype=np.float64).reshape(-1)[idx]
    n = idx.shape[0]
    v = hv @ wv + bv
    e = v - R
    if cfg.clip is None:
        l, unclipped = 0.5 * e * e, np.ones(n, dtype=bool)
    else:
        vo = np.asarray(old_values, dtype=np.float64).reshape(-1)[idx]
        c = float(cfg.clip)
        d = v - vo
        ec = np.where(np.abs(d) <= c, e, vo + np.copysign(c, d) - R)      # inside the range vc IS v: an exact tie, in any precision
        unclipped = e * e >= ec * ec
        l = 0.5 * np.maximum(e * e, ec * ec)
    g = np.where(unclipped, e, 0.0)
    dv = cfg.coef * g / n * inv_world if n else np.zeros(0)
    mean = lambda x: float(x.sum() / n) if n else 0.0
    vl = mean(l)
    total = float(policy_loss) + cfg.coef * vl
    den = float(((R - mean(R)) ** 2).sum()) if n else 0.0
    ev = 1.0 - float(((e - mean(e)) ** 2).sum()) / den if den > 0 else 0.0
    stats = np.array([vl, n, mean((~unclipped).astype(np.float64)), mean(v), mean(R), ev, mean(np.abs(e)), total], dtype=np.float64)
    full = lambda x, dtype=np.float64: _scatter(x, idx, rows, dtype)
    dw = np.zeros(D)
    for j in range(n):                                          # ascending r
        dw += dv[j] * hv[j]
    dhn = np.zeros((rows, D))
    if not cfg.detach and n:
        dhn[idx] = dv[:, None] * wv[None, :]
    out_rows = np.stack([full(v), full(l), full((~unclipped).astype(np.float64)), full(dv)], axis=1)
    return ValueLossResult(index=idx, value=full(v), loss=full(l), clipped=full(~unclipped, bool), dl_dv=full(g), dv=full(dv),
                           rows=out_rows, value_loss=vl, total=total, stats=stats, dw=dw, db=float(dv.sum()), dhn=dhn)


def _scatter(x, idx, rows: int, dtype):
    out = np.zeros(rows, dtype=dtype)
    out[idx] = x
    return out
