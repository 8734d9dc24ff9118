"""Beam search over the action tokens: the host SPECIFICATION (numpy) of `bl_beam_step_f32` (csrc/beam.hip).

This module is to the beam step what `sampling.py` is to the sampler: the definition. The device kernel is its
bit-identical twin — tokens, parents, both integers of every weight pair and the fp32 scores.

The search. W beams of one prompt are extended for a FIXED number n of tokens; no beam finishes early and EOS is an
ordinary token. All hypotheses therefore have the same length at every step, so HF's `length_penalty` and `early_stopping`
cannot change their order: the model surface accepts and ignores them. With the policy restricted to the action tokens
(`action_tokens_only=True`) no EOS can occur at all, and the search is HF's `generate(num_beams=W, do_sample=False)` up to
fp32 rounding at near-ties: HF ranks the same W × count continuations by the sum of `log_softmax` values in the model's
dtype, this module by the sums below.

One step (`beam_step`) for beam rows j = 0 … W-1 with logits l_{j,i} and running scores s_j:
  m_j      the row maximum
  w_{j,i}  = rint(exp_spec(l_{j,i} - m_j) · 2^30), exactly `sampling.weights(l_j, 1)`: an integer in [0, 2^30]
  total_j  = Σ_i w_{j,i}: exact integer arithmetic (below 2^45), so the order of summation does not matter
  lz_j     = log_spec(fp32(total_j) · 2^-30): the log of the softmax denominator, a fixed sequence of individually
             rounded fp32 operations like `exp_spec` (the int → fp32 conversion rounds to nearest even, the scaling is exact)
  c_{j,i}  = fp32(fp32(s_j + fp32(l_{j,i} - m_j)) - lz_j): the candidate's joint log-probability
The W survivors are the first W candidates of the total order "c descending, then flat index j·n + i ascending": ties
are fully defined (bf16-rounded logits make exact ties common), and -inf scores order by index. The order is taken on
`order_key(c)`, the integer image of the float order that `bl_argmax_f32` uses (−0 = +0; a NaN would rank on top: NaN
logits are outside the definition, as for a sampled row, but the kernel's parents and tokens stay in range whatever the
logits hold). Survivor k reports tokens[k] = i, parents[k] = j, wt[k] = (w_{j,i}, total_j) — the pair
`sampling.score_rows` gives token i on row j under the default `SamplingParams()` — and new_scores[k] = c_{j,i}.

Step 0 is no special case: the caller passes scores = [0, -inf, …, -inf] (`start_scores`), so every survivor descends
from beam 0 even though all W rows hold the same logits. W <= the number of tokens is required: fewer candidates than
beams would leave slots without a finite hypothesis at step 0.

`vocab=(first, count)` means what it means everywhere in `sampling.py`: the same on the slice, ids in full-vocabulary
numbering.

The domain (tests/test_beam_edge_gpu.py holds the kernel to all of it, on fp32 logits that are not bf16-rounded): -inf
logits are INSIDE the definition as long as every row maximum is finite — the candidate weighs 0 and scores -inf; +inf and
NaN logits are outside. Scores are any fp32 <= 0 down to -1e30, and -inf for a dead beam; a prompt whose beams are ALL
dead has only -inf candidates and its survivors are the first W flat indices. total_j runs from 2^30 (a peaked row:
lz_j = log_spec(1) = 0) to 36 480 · 2^30 > 2^45 (an all-equal row of the widest width the kernel takes), so fp32(total_j)
rounds a 46-bit integer.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np

from .sampling import _LN2_HI, _LN2_LO, check_vocab, weights

MAX_BEAMS = 16                       # the kernel's limit (one workgroup ranks W rows; the engines' batch-invariant 16 rows)
_f32 = np.float32
_SQRT2 = _f32(1.41421354)
_LOG_C = tuple(_f32(v) for v in (1.0 / 9, 1.0 / 7, 1.0 / 5, 1.0 / 3))            # atanh series in z = s², degree 3 … 0


def log_spec(x) -> np.ndarray:
    """ln x for fp32 x >= 1, every operation individually rounded (numpy never contracts); the device twin is `log_spec`
    in csrc/beam.hip under `#pragma clang fp contract(off)`. x = 2^e · m by bit operations, m moved into (√2/2, √2] (the
    halving is exact); f = m - 1 is exact (Sterbenz), s = f / (2 + f), |s| <= 0.17158, and
        ln m = 2·atanh(s) = 2s·(1 + z/3 + z²/5 + z³/7 + z⁴/9 + …),  z = s² <= 0.02944,
    truncated after z⁴/9 (Horner, separate multiply and add); ln x = e·LN2_HI + (e·LN2_LO + ln m) with exp_spec's two
    constants (e <= 15 and LN2_HI has 9 bits: that product is exact).
    Error, u = 2^-24: the dropped tail is below z⁵/11 / (1 - z) = 2.1e-9 = 0.04 u of 2s; s carries 2 u (the sum 2 + f and
    the quotient), the correction s·z·P(z) <= 0.0101·|s| carries at most 18 u of itself, and their sum rounds once more:
    |ln m| is off by at most 2·|s|·(2 + 0.19 + 1.02 + 0.04) u <= 1.12 u. e·LN2_LO (|·| <= 3.2e-3, constant and product
    rounded) adds 0.01 u, the sum e·LN2_LO + ln m (|·| <= 0.35) at most 0.35 u, and the last sum u·ln x. Together
        |log_spec(x) - ln x| <= 2^-24 · (ln x + 1.5):  8.9e-8 near 1, 7.1e-7 at x = 32 064.
    tests/test_beam_cpu.py asserts it on a dense grid. The only arguments beam_step passes are fp32(total) · 2^-30, which
    lie in [1, vocab]: the row maximum alone has weight 2^30."""
    x = np.ascontiguousarray(np.asarray(x, dtype=_f32))
    b = x.view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - 127
    m = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(_f32)
    big = m > _SQRT2
    m = np.where(big, m * _f32(0.5), m)
    e = (e + big).astype(_f32)
    f = m - _f32(1.0)
    d = f + _f32(2.0)
    s = f / d
    z = s * s
    p = np.full_like(z, _LOG_C[0])
    for c in _LOG_C[1:]:
        p = p * z
        p = p + c
    p = p * z
    t = p * s
    r = t + s
    lm = r + r
    lo = e * _LN2_LO
    a = lo + lm
    hi = e * _LN2_HI
    return hi + a


def order_key(c) -> np.ndarray:
    """int32 keys whose signed order is the order of the fp32 values c (−0 and +0 share a key, NaN on top): `argmax_key`
    of csrc/bl_common.h. Candidates rank by key descending, then flat index ascending."""
    b = np.ascontiguousarray(np.asarray(c, dtype=_f32)).view(np.int32)
    b = np.where(b == np.int32(-0x80000000), np.int32(0), b)
    k = b ^ ((b >> 31) & np.int32(0x7FFFFFFF))
    return np.where(np.isnan(c), np.int32(0x7FFFFFFF), k).astype(np.int32)


def start_scores(W: int) -> np.ndarray:
    """The scores of step 0: [0, -inf, …, -inf] — all W rows hold the same prompt, only beam 0 may have children."""
    s = np.full(W, -np.inf, dtype=_f32)
    s[0] = 0.0
    return s


def beam_step(logits, scores, vocab=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """logits [W, n], scores fp32 [W] → (tokens int64 [W], parents int32 [W], wt int64 [W, 2], new_scores fp32 [W]) — what
    bl_beam_step_f32 writes for one prompt (module docstring). vocab=(first, count): the same on the slice, tokens in
    full-vocabulary numbering."""
    l = np.asarray(logits, dtype=_f32)
    if l.ndim != 2:
        raise ValueError(f"beam_step: logits [W, n], got shape {l.shape}")
    W, n = l.shape
    vocab = check_vocab(vocab, n, "beam_step")
    if vocab is not None:
        tokens, parents, wt, new = beam_step(l[:, vocab[0]:vocab[0] + vocab[1]], scores)
        return tokens + vocab[0], parents, wt, new
    s = np.asarray(scores, dtype=_f32)
    if s.shape != (W,):
        raise ValueError(f"beam_step: scores must be [{W}], got shape {s.shape}")
    if not 1 <= W <= MAX_BEAMS or W > n:
        raise ValueError(f"beam_step: {W} beams over {n} tokens: 1 <= W <= min({MAX_BEAMS}, the token count) is required")
    w = np.stack([weights(l[j], 1.0) for j in range(W)])
    total = w.sum(axis=1)
    lz = log_spec(total.astype(_f32) * _f32(2.0 ** -30))
    with np.errstate(invalid="ignore", over="ignore"):
        d = l - l.max(axis=1)[:, None]
        c = s[:, None] + d
        c = c - lz[:, None]
    flat = np.argsort(-order_key(c).reshape(-1).astype(np.int64), kind="stable")[:W]      # key descending, index ascending
    parents, tokens = flat // n, flat % n
    return (tokens.astype(np.int64), parents.astype(np.int32),
            np.stack([w[parents, tokens], total[parents]], axis=1).astype(np.int64), c[parents, tokens].astype(_f32))


def backtrack(tokens, parents, wt) -> Tuple[np.ndarray, np.ndarray]:
    """Per-step survivors tokens [n, W], parents [n, W], wt [n, W, 2] → the W finished sequences int64 [W, n] and their
    per-token weight pairs int64 [W, n, 2], in slot order of the last step = by final score, best first."""
    tokens, parents, wt = np.asarray(tokens), np.asarray(parents), np.asarray(wt)
    n, W = tokens.shape
    seq, pairs = np.zeros((W, n), np.int64), np.zeros((W, n, 2), np.int64)
    slot = np.arange(W)
    for t in range(n - 1, -1, -1):
        seq[:, t], pairs[:, t] = tokens[t, slot], wt[t, slot]
        slot = parents[t, slot].astype(np.int64)
    return seq, pairs


def beam_search(row_fn: Callable[[np.ndarray], np.ndarray], W: int, n_steps: int, vocab: Optional[Tuple[int, int]] = None):
    """A small host driver over `beam_step`; `row_fn(prefixes int64 [W, t]) → logits [W, n]` stands in for the model
    (step t sees every beam's t tokens so far). Returns (sequences int64 [W, n_steps], wt int64 [W, n_steps, 2], scores
    fp32 [W]), best first."""
    scores, prefixes = start_scores(W), np.zeros((W, 0), np.int64)
    tokens, parents, pairs = [], [], []
    for _ in range(n_steps):
        tok, par, wt, scores = beam_step(row_fn(prefixes), scores, vocab)
        prefixes = np.concatenate([prefixes[par], tok[:, None]], axis=1)
        tokens.append(tok), parents.append(par), pairs.append(wt)
    seq, wts = backtrack(np.stack(tokens), np.stack(parents), np.stack(pairs))
    assert np.array_equal(seq, prefixes)
    return seq, wts, scores
