"""The preference-pair loss of the training step (DPO family): the host SPECIFICATION (numpy, fp64) of
`bl_preference_loss_f32` (csrc/policy.hip); its gradient is served by the policy loss's backward kernels.

Rows, targets, `IGNORE_INDEX`, the temperature T and `token_range` are the policy loss's (training/policy_loss.py): logp_r,
p_i, m, S and H of a valid row are defined there, over the token range if one is set. `group_rows` consecutive rows are one
sequence b; G_b is the set of its valid rows and n_b = |G_b|. An int32 `pair[b]` per sequence says where it stands: +k is
the chosen side of pair k, −k the rejected side, 0 in no pair; k runs over 1…P and a side may hold several sequences (the
trajectory-level form: every step of the preferred trajectory against every step of the other). With per-row reference
log-probabilities ref_r (None: the reference-free form, ref_r = 0):

    c_b     = 1 ("sum")  or  1 / n_b ("mean")                  (seq_norm)
    δ_b     = c_b · Σ_{r∈G_b} (logp_r − ref_r)                 summed in row order; 0 if n_b = 0
    Δ_k     = Σ_{pair[b]=+k} δ_b − Σ_{pair[b]=−k} δ_b          each sum in ascending b
    h_k     = β·Δ_k − γ
    ℓ_k     = −(1−ε)·logσ(h_k) − ε·logσ(−h_k)                  kind="sigmoid" (DPO; ε = label_smoothing: cDPO; γ > 0, no
                                                               reference and "mean": SimPO)
            = (h_k/β − 1/(2β))²                                kind="ipo"     (γ = ε = 0)
            = max(0, 1 − h_k)                                  kind="hinge"   (SLiC; ε = 0)
    ℓ'_k    = σ(h_k) − (1−ε)  |  2·(h_k/β − 1/(2β))/β  |  −[h_k < 1]
    N_k     = Σ_{pair[b]=+k} n_b
    nll_k   = −Σ_{pair[b]=+k} Σ_{r∈G_b} logp_r / N_k           (the chosen side's token-mean NLL: RPO's SFT term)
    loss    = (1/P) · Σ_k (ℓ_k + α·nll_k)
    g_r     = ℓ'_k · β · sign(pair[b]) · c_b − [pair[b] > 0]·α / N_k      for r ∈ G_b, k = |pair[b]|; 0 if pair[b] = 0
    dlogits_{r,i} = g_r · (δ_{i,a_r} − p_i) / (T · P)           0 on ignored rows and outside the token range

logσ(h) is −softplus(−h). The step statistics are PREF_STAT_NAMES (means over the pairs; slots 0 and 1 are (loss, P), the
divisor the backward kernel reads), the per-pair statistics PAIR_STAT_NAMES, the per-sequence ones SEQ_STAT_NAMES.

Preconditions (ValueError): the pair ids are dense in 1…P with P ≥ 1; every pair has a valid row on each side; logits and
ref are finite on the valid rows of paired sequences. A sequence with pair = 0 may carry labels: its logp, H, δ_b and n_b
are reported like any other's (this is how `token_logprobs()` records a reference), it contributes nothing to the loss and
its rows get g = 0, so dlogits = 0 (the device backward forms 0·(δ − p) there: exact zeros for finite logits).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .policy_loss import IGNORE_INDEX, PolicyLossConfig, _group_sums, row_softmax, slice_range

# the step statistics vector (fp32 [8]); slots 0 and 1 are (loss, divisor) as cross-entropy's mean_and_count
PREF_STAT_NAMES = ("loss", "n_pairs", "pref", "accuracy", "margin", "reward_chosen", "reward_rejected", "nll")
# per pair (fp32 [P, 4]) and per sequence (fp32 [B, 4]; g is ℓ'_k·β·sign·c_b, the α term left out)
PAIR_STAT_NAMES = ("h", "loss", "dloss", "nll")
SEQ_STAT_NAMES = ("delta", "n", "logp", "g")
KINDS = ("sigmoid", "ipo", "hinge")
SEQ_NORMS = ("sum", "mean")


@dataclass(frozen=True)
class PreferenceLossConfig:
    beta: float = 0.1
    kind: str = "sigmoid"
    label_smoothing: float = 0.0                     # ε (cDPO)
    margin: float = 0.0                              # γ (SimPO's target margin)
    sft_coef: float = 0.0                            # α (RPO's weight of the chosen side's NLL)
    seq_norm: str = "sum"                            # δ_b is the sum ("sum") or the mean ("mean") over the sequence's tokens
    temperature: float = 1.0
    token_range: Optional[Tuple[int, int]] = None    # (first, count): the policy is over these tokens alone
    reference_free: bool = False                     # no ref_logprobs (SimPO, ORPO-style)

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"PreferenceLossConfig: kind is one of {KINDS}, got {self.kind!r}")
        if self.seq_norm not in SEQ_NORMS:
            raise ValueError(f"PreferenceLossConfig: seq_norm is 'sum' or 'mean', got {self.seq_norm!r}")
        object.__setattr__(self, "token_range", PolicyLossConfig(token_range=self.token_range).token_range)
        if not (np.isfinite(self.temperature) and self.temperature > 0):
            raise ValueError("PreferenceLossConfig: temperature must be > 0")
        if not (np.isfinite(self.beta) and self.beta > 0):
            raise ValueError("PreferenceLossConfig: beta must be > 0")
        if not (0 <= self.label_smoothing < 0.5):
            raise ValueError("PreferenceLossConfig: 0 <= label_smoothing < 0.5")
        if not (np.isfinite(self.margin) and self.margin >= 0):
            raise ValueError("PreferenceLossConfig: margin must be >= 0")
        if not (np.isfinite(self.sft_coef) and self.sft_coef >= 0):
            raise ValueError("PreferenceLossConfig: sft_coef must be >= 0")
        if self.kind == "ipo" and (self.margin != 0 or self.label_smoothing != 0):
            raise ValueError("PreferenceLossConfig: kind='ipo' takes margin = 0 and label_smoothing = 0")
        if self.kind == "hinge" and self.label_smoothing != 0:
            raise ValueError("PreferenceLossConfig: kind='hinge' takes label_smoothing = 0")
        object.__setattr__(self, "reference_free", bool(self.reference_free))

    def backward_config(self) -> PolicyLossConfig:
        """What the policy loss's backward op reads of a configuration: T and the token range, no entropy bonus."""
        return PolicyLossConfig(temperature=self.temperature, token_range=self.token_range)


@dataclass
class PreferenceLossResult:
    logp: np.ndarray          # [rows]  log π(a); 0 on ignored rows
    entropy: np.ndarray       # [rows]  H, likewise
    valid: np.ndarray         # [rows]  bool
    g: np.ndarray             # [rows]
    loss: float
    n_pairs: int
    stats: np.ndarray         # [8] fp64, PREF_STAT_NAMES
    pair_stats: np.ndarray    # [P, 4] fp64, PAIR_STAT_NAMES
    seq_stats: np.ndarray     # [B, 4] fp64, SEQ_STAT_NAMES
    dlogits: np.ndarray       # [rows, n] fp64


def log_sigmoid(h):
    """log σ(h) = −softplus(−h), stable on both sides."""
    h = np.asarray(h, dtype=np.float64)
    return -(np.maximum(-h, 0.0) + np.log1p(np.exp(-np.abs(h))))


def sigmoid(h):
    h = np.asarray(h, dtype=np.float64)
    e = np.exp(-np.abs(h))
    return np.where(h >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def pair_terms(h, cfg: PreferenceLossConfig):
    """(ℓ_k, ℓ'_k) of h_k."""
    h = np.asarray(h, dtype=np.float64)
    if cfg.kind == "sigmoid":
        eps = cfg.label_smoothing
        return -(1.0 - eps) * log_sigmoid(h) - eps * log_sigmoid(-h), sigmoid(h) - (1.0 - eps)
    if cfg.kind == "ipo":
        u = h / cfg.beta - 1.0 / (2.0 * cfg.beta)
        return u * u, 2.0 * u / cfg.beta
    return np.maximum(0.0, 1.0 - h), -(h < 1.0).astype(np.float64)


def check_pairs(pair, n_valid) -> int:
    """The pair-id preconditions for `pair` int [B] and the sequences' valid-row counts [B] → P. ValueError otherwise."""
    pair = np.asarray(pair)
    if pair.ndim != 1 or not np.issubdtype(pair.dtype, np.integer):
        raise ValueError(f"pair: an integer vector, one entry per sequence, got {pair.dtype} {pair.shape}")
    n_valid = np.asarray(n_valid)
    if n_valid.shape != pair.shape:
        raise ValueError(f"pair: {pair.shape[0]} entries for {n_valid.shape[0]} sequences")
    ids = np.unique(np.abs(pair[pair != 0]))
    P = int(ids.size)
    if P < 1:
        raise ValueError("pair: no pair in the batch")
    if ids[0] != 1 or ids[-1] != P:
        raise ValueError(f"pair: ids must be dense in 1…P, got {ids[:8].tolist()}{'…' if P > 8 else ''}")
    for k in range(1, P + 1):
        for sign, side in ((1, "chosen"), (-1, "rejected")):
            if n_valid[pair == sign * k].sum() < 1:
                raise ValueError(f"pair {k}: no labelled token on its {side} side")
    return P


def preference_loss(logits, targets, pair, ref_logprobs=None, cfg: Optional[PreferenceLossConfig] = None,
                    group_rows: Optional[int] = None, ignore_index: int = IGNORE_INDEX) -> PreferenceLossResult:
    """logits [rows, n], targets [rows], pair int [rows / group_rows], ref_logprobs [rows] or None (iff cfg.reference_free)."""
    cfg = cfg or PreferenceLossConfig()
    if (ref_logprobs is None) != cfg.reference_free:
        raise ValueError("preference_loss: ref_logprobs is given unless cfg.reference_free")
    rows, n = np.shape(logits)
    if group_rows is None or int(group_rows) != group_rows or group_rows < 1 or rows % int(group_rows):
        raise ValueError(f"preference_loss: needs group_rows >= 1 dividing the {rows} rows, got {group_rows!r}")
    group_rows = int(group_rows)
    B = rows // group_rows
    first, count = cfg.token_range if cfg.token_range is not None else (0, n)
    sliced, tg = slice_range(logits, targets, (first, count), ignore_index, "preference_loss")
    valid = tg != ignore_index
    if valid.any() and tg[valid].min() < 0:
        raise ValueError(f"preference_loss: targets must lie in [0, {n}) or be {ignore_index}")
    pair = np.asarray(pair)
    n_b = valid.reshape(B, group_rows).sum(axis=1)
    P = check_pairs(pair, n_b)
    pair = pair.astype(np.int64)
    used = valid & np.repeat(pair != 0, group_rows)           # the rows that are looked at
    l = np.where(valid[:, None], np.asarray(sliced, dtype=np.float64), 0.0)
    if not np.isfinite(l[used]).all():
        raise ValueError("preference_loss: logits must be finite on the labelled rows of paired sequences")
    ref = np.zeros(rows)
    if ref_logprobs is not None:
        ref = np.asarray(ref_logprobs, dtype=np.float64)
        if ref.shape != (rows,):
            raise ValueError(f"ref_logprobs: shape {ref.shape}, expected {(rows,)}")
        ref = np.where(valid, ref, 0.0)
        if not np.isfinite(ref[used]).all():
            raise ValueError("ref_logprobs: non-finite value(s) on labelled rows of paired sequences")
    T = float(cfg.temperature)
    with np.errstate(all="ignore"):                           # an unpaired sequence's rows may hold anything
        logp_all, p, H = row_softmax(l, T)
    a = np.where(valid, tg, 0)
    logp = np.where(valid, logp_all[np.arange(rows), a], 0.0)
    d_sum, _ = _group_sums(logp - ref, valid, group_rows)
    lp_sum, _ = _group_sums(logp, valid, group_rows)
    c_b = 1.0 / np.maximum(n_b, 1) if cfg.seq_norm == "mean" else np.ones(B)
    delta = c_b * d_sum
    beta, gamma, alpha = float(cfg.beta), float(cfg.margin), float(cfg.sft_coef)
    rc, rr, N, nll = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    for b in range(B):                                        # ascending b
        k = abs(int(pair[b])) - 1
        if pair[b] > 0:
            rc[k] += delta[b]
            N[k] += n_b[b]
            nll[k] += lp_sum[b]
        elif pair[b] < 0:
            rr[k] += delta[b]
    nll = -nll / N
    Delta = rc - rr
    h = beta * Delta - gamma
    lk, dk = pair_terms(h, cfg)
    loss = float((lk + alpha * nll).sum() / P)
    kb = np.abs(pair) - 1
    g_seq = np.where(pair != 0, dk[kb] * beta * np.sign(pair) * c_b, 0.0)
    g_b = g_seq - np.where(pair > 0, alpha / N[kb], 0.0)
    g = np.where(used, np.repeat(g_b, group_rows), 0.0)
    onehot = np.zeros_like(l)
    onehot[np.arange(rows), a] = 1.0
    dl = np.zeros((rows, n))
    dl[:, first:first + count] = np.where(used[:, None], g[:, None] * (onehot - p) / (T * P), 0.0)
    mean = lambda v: float(np.sum(v) / P)
    stats = np.array([loss, P, mean(lk), mean((Delta > 0).astype(np.float64)), mean(beta * Delta), mean(beta * rc),
                      mean(beta * rr), mean(nll)], dtype=np.float64)
    seq_stats = np.stack([delta, n_b.astype(np.float64), lp_sum, g_seq], axis=1)
    return PreferenceLossResult(logp=logp, entropy=np.where(valid, H, 0.0), valid=valid, g=g, loss=loss, n_pairs=P, stats=stats,
                                pair_stats=np.stack([h, lk, dk, nll], axis=1), seq_stats=seq_stats, dlogits=dl)
