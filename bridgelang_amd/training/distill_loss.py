"""The distribution-matching (distillation) loss of the training step: the host SPECIFICATION (numpy, fp64) of
`bl_distill_loss_f32` / `bl_distill_loss_backward_f32` (csrc/distill.hip).

The host file is the definition and the kernels are its fp32 twin to a tolerance, as `policy_loss.py` ↔ csrc/policy.hip.

Rows, `targets`, `IGNORE_INDEX`, `temperature` and `token_range = (first, count)` mean exactly what they mean in the policy
loss (`row_softmax` and `slice_range` are its). The loss learns from a DISTRIBUTION per row, not from one token: an OpenVLA
action token is one of 256 bins, so a teacher's whole row (`score_actions(return_bins=True)`, a Gaussian round the
demonstrated bin, an average of several policies) fits next to the 256 logits it is compared with, and the divergence is
computed exactly instead of estimated on one sampled token (the policy loss's k3 `kl_coef`). Per valid row with logits
l[0..n) over the range, target token a and a teacher row q_i >= 0 (fp32, already at whatever temperature the caller wants):

    z_i    = l_i / T                     m = max z      S = Σ exp(z_i − m)
    logp_i = z_i − m − log S             p_i = exp(logp_i)          H = −Σ p_i·logp_i
    Q      = Σ q_i                       (the teacher's mass; 1 up to rounding)

    forward_kl : D = Σ q_i·(log q_i − logp_i)                         ∂D/∂z_i = p_i·Q − q_i             c = Q
    reverse_kl : D = Σ p_i·(logp_i − log q_i)        u_i = logp_i − log q_i
    jsd (β)    : m_i = β·q_i + (1 − β)·p_i
                 D = β·Σ q_i·log(q_i / m_i) + (1 − β)·Σ p_i·log(p_i / m_i)    u_i = (1 − β)·(logp_i − log m_i)
    reverse_kl, jsd:                                                  ∂D/∂z_i = p_i·(u_i − c),  c = Σ_j p_j·u_j
    row_loss  = D + sft_coef·(−logp_a)
    loss      = Σ_valid row_loss / n_valid
    dlogits_i = [ ∂D/∂z_i + sft_coef·(p_i − δ_ia) ] / (T · n_valid)

A term whose weight (q_i or p_i) is 0 is 0. logp_i is always z_i − m − log S by arithmetic, never log(p_i), so an
underflowed p_i gives 0·finite. The derivatives are exact for any q >= 0, not only for Σ q = 1: that is why Q appears
(tests/test_distill_loss_cpu.py holds all three against central differences). For reverse_kl c = D. There is NO T² factor:
the loss is the divergence at temperature T as it stands, and its gradient carries the 1/T of z = l / T alone; a caller who
wants Hinton's T²-scaled soft-target gradient multiplies the loss weight.

Preconditions (ValueError from `distill_loss`): finite logits; on valid rows a finite teacher with q_i >= 0 and
|Q − 1| <= 1e-3; for reverse_kl q_i > 0 on the whole range of every valid row (its divergence is infinite otherwise —
`rl.distill_batch(smoothing=)` is the way out); a valid target outside the range, as in the policy loss. forward_kl and jsd
take zeros in the teacher.

`agree` is whether student and teacher share their FIRST argmax over the range. The step statistics are means over valid
rows; `bin_gap` is |Σ_i i·(p_i − q_i)| with i counted from the start of the range: the distance between the two expected
bins, in bins."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .policy_loss import IGNORE_INDEX, row_softmax, slice_range

KINDS = ("forward_kl", "reverse_kl", "jsd")
# the step statistics vector (fp32 [8]); slots 0 and 1 are cross-entropy's mean_and_count
DISTILL_STAT_NAMES = ("loss", "n_valid", "divergence", "entropy", "teacher_entropy", "agreement", "nll", "bin_gap")
# the per-row statistics (fp32 [rows, 8]): logp, m and log_s sit where policy_loss.ROW_STAT_NAMES has them
DISTILL_ROW_STAT_NAMES = ("logp", "entropy", "divergence", "row_loss", "agree", "m", "log_s", "c")
MASS_TOL = 1e-3


@dataclass(frozen=True)
class DistillLossConfig:
    kind: str = "forward_kl"
    beta: float = 0.5                                 # jsd only: the teacher's weight in the mixture m = β·q + (1 − β)·p
    temperature: float = 1.0
    sft_coef: float = 0.0                             # + sft_coef · (−log π(target))
    token_range: Optional[Tuple[int, int]] = None     # (first, count): student and teacher are over these tokens alone

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"DistillLossConfig: kind is one of {KINDS}, got {self.kind!r}")
        if not 0 < self.beta < 1:
            raise ValueError("DistillLossConfig: 0 < beta < 1 (the teacher's weight in jsd's mixture)")
        if not (np.isfinite(self.temperature) and self.temperature > 0):
            raise ValueError("DistillLossConfig: temperature must be > 0")
        if not (np.isfinite(self.sft_coef) and self.sft_coef >= 0):
            raise ValueError("DistillLossConfig: sft_coef must be >= 0")
        if self.token_range is not None:
            try:
                first, count = (int(v) for v in self.token_range)
                exact = (first, count) == tuple(self.token_range)
            except (TypeError, ValueError):
                exact = False
            if not exact or first < 0 or count < 1:
                raise ValueError("DistillLossConfig: token_range is None or (first, count) with first >= 0 and count >= 1")
            object.__setattr__(self, "token_range", (first, count))


@dataclass
class DistillLossResult:
    logp: np.ndarray          # [rows]  log π(a); 0 on ignored rows, as every per-row array
    entropy: np.ndarray       # [rows]  H
    divergence: np.ndarray    # [rows]  D
    row_loss: np.ndarray
    agree: np.ndarray         # [rows]  0/1: the first argmax of p is the first argmax of q
    m: np.ndarray             # [rows]  max z
    log_s: np.ndarray         # [rows]  log Σ exp(z − m)
    c: np.ndarray             # [rows]  Q (forward_kl) or Σ p·u
    teacher_entropy: np.ndarray
    bin_gap: np.ndarray
    valid: np.ndarray         # [rows]  bool
    loss: float
    stats: np.ndarray         # [8] fp64, DISTILL_STAT_NAMES
    dlogits: np.ndarray       # [rows, n] fp64


def check_teacher(q, valid, kind: str, what: str = "distill_loss") -> None:
    """The teacher's preconditions on the rows `valid` marks: q [rows, count], finite, >= 0, |Σ q − 1| <= 1e-3, and > 0
    everywhere for reverse_kl. ValueError otherwise; the other rows may hold anything."""
    q = np.asarray(q, dtype=np.float64)
    valid = np.asarray(valid, dtype=bool)
    qv = q[valid]
    if not np.isfinite(qv).all():
        raise ValueError(f"{what}: the teacher must be finite on labelled rows")
    if (qv < 0).any():
        raise ValueError(f"{what}: the teacher must be >= 0 on labelled rows")
    mass = qv.sum(axis=1)
    if (np.abs(mass - 1.0) > MASS_TOL).any():
        bad = int(np.argmax(np.abs(mass - 1.0) > MASS_TOL))
        raise ValueError(f"{what}: a teacher row sums to {mass[bad]!r}, not to 1 within {MASS_TOL} (labelled row {bad})")
    if kind == "reverse_kl" and (qv <= 0).any():
        raise ValueError(f"{what}: reverse_kl needs a teacher > 0 on the whole range of every labelled row (its divergence is "
                         "infinite otherwise) — smooth the teacher, or use forward_kl / jsd")


def _xlogy(x, logy):
    """x·logy with the term 0 where the weight x is 0."""
    with np.errstate(all="ignore"):
        return np.where(x > 0, x * logy, 0.0)


def distill_loss(logits, targets, teacher, cfg: Optional[DistillLossConfig] = None,
                 ignore_index: int = IGNORE_INDEX) -> DistillLossResult:
    """`teacher`: [rows, count] over the range (count = n without one), column j being token first + j."""
    cfg = cfg or DistillLossConfig()
    n_full = np.shape(logits)[1]
    first, count = cfg.token_range or (0, n_full)
    sliced, tg = slice_range(logits, targets, (first, count), ignore_index, "distill_loss")
    l = np.asarray(sliced, dtype=np.float64)
    rows, n = l.shape
    valid = tg != ignore_index
    if not np.isfinite(l).all():
        raise ValueError("distill_loss: logits must be finite")
    q = np.asarray(teacher, dtype=np.float64)
    if q.shape != (rows, n):
        raise ValueError(f"distill_loss: teacher shape {q.shape}, expected {(rows, n)} (one row per logits row, over the range)")
    check_teacher(q, valid, cfg.kind)
    q = np.where(valid[:, None], q, 0.0)
    T, beta, sft = float(cfg.temperature), float(cfg.beta), float(cfg.sft_coef)
    logp_all, p, H = row_softmax(l, T)
    z = l / T
    m = z.max(axis=1)
    log_s = np.log(np.exp(z - m[:, None]).sum(axis=1))
    a = np.where(valid, tg, 0)
    logp = logp_all[np.arange(rows), a]
    Q = q.sum(axis=1)
    with np.errstate(all="ignore"):
        logq = np.log(q)
        if cfg.kind == "forward_kl":
            D = _xlogy(q, logq - logp_all).sum(axis=1)
            c = Q
            dz = p * Q[:, None] - q
        else:
            if cfg.kind == "reverse_kl":
                u = logp_all - logq
                D = _xlogy(p, u).sum(axis=1)
                c = D
            else:
                mix = beta * q + (1.0 - beta) * p
                logm = np.log(mix)
                u = (1.0 - beta) * (logp_all - logm)
                c = _xlogy(p, u).sum(axis=1)
                D = beta * _xlogy(q, logq - logm).sum(axis=1) + c
            dz = np.where(p > 0, p * (u - c[:, None]), 0.0)
        teacher_entropy = -_xlogy(q, logq).sum(axis=1)
    row_loss = D + sft * (-logp)
    agree = (np.argmax(l, axis=1) == np.argmax(q, axis=1)).astype(np.float64)      # first argmax; z is monotone in l
    idx = np.arange(n, dtype=np.float64)
    bin_gap = np.abs(((p - q) * idx).sum(axis=1))
    nv = int(valid.sum())
    onehot = np.zeros_like(l)
    onehot[np.arange(rows), a] = 1.0
    dl = np.zeros((rows, n_full), dtype=np.float64)
    if nv:
        core = (dz + sft * (p - onehot)) / (T * nv)
        core[~valid] = 0.0
        dl[:, first:first + count] = core
    zero = lambda v: np.where(valid, v, 0.0)
    mean = lambda v: float(v[valid].sum() / nv) if nv else 0.0
    stats = np.array([mean(row_loss), nv, mean(D), mean(H), mean(teacher_entropy), mean(agree), mean(-logp), mean(bin_gap)],
                     dtype=np.float64)
    return DistillLossResult(logp=zero(logp), entropy=zero(H), divergence=zero(D), row_loss=zero(row_loss), agree=zero(agree),
                             m=zero(m), log_s=zero(log_s), c=zero(c), teacher_entropy=zero(teacher_entropy), bin_gap=zero(bin_gap),
                             valid=valid, loss=stats[0], stats=stats, dlogits=dl)
