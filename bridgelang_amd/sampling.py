"""Seeded sampling of action tokens: the host SPECIFICATION (numpy) of `bl_sample_f32` (csrc/sample.hip).

The device kernel is a bit-identical twin of `sample_rows` below — token id and both integers of the weight pair — in
the manner of `vla/image_augment.augment_frame` ↔ `bl_augment_frames_u8`. To make that possible the sampler uses no
library transcendental and no floating-point sum whose order matters:

  RNG      Philox4x32-10 (Salmon et al., SC'11; pinned by Random123's known-answer vectors). key = the sequence's
           64-bit seed (low word, high word), counter = (generation step t, 0, 0, 0), u64 = x0 << 32 | x1. A sequence's
           draws depend on its own seed and the step only: not on its batch slot, the batch size or the pipeline.
  exp      `exp_spec`: a fixed sequence of individually rounded fp32 operations (clamp at -87, n = rint(x·log2e),
           two-constant Cody–Waite reduction, degree-6 Horner with separate multiply and add, scale by 2^n).
  weights  z_i = fp32((l_i - max l) / T), w_i = rint(exp_spec(z_i) · 2^30): an integer in [0, 2^30]; everything after
           this point is exact integer arithmetic (a row of 32 064 weights sums below 2^45). A token whose probability
           is below 2^-31 of the maximum's gets weight 0 and is NEVER drawn (HF would draw it with probability < 5e-10).
  top-k    HF's TopKLogitsWarper: keep l_i >= the k-th largest logit — every tie at that value stays. 0 disables.
  top-p    HF's TopPLogitsWarper in integers, after top-k: rank by (w descending, index ascending); token i stays iff
           before_i · 2^24 < rint(top_p · 2^24) · total, before_i = the weight ranked strictly ahead of it (a 70-bit
           comparison; equivalently before_i < ceil(rint(top_p · 2^24) · total / 2^24)); the first-ranked token always
           stays. top_p >= 1 disables. 24 bits hold an fp32 top_p in [0.5, 1) exactly; a 16-bit top_p moved the boundary
           by up to 2^-17 of the mass and kept one token fewer than HF in 4 of the 200 cases of
           tests/test_sampling_cpu.py.
  draw     target = mulhi64(u64, total_kept); the token is the lowest index whose running sum of kept weights, taken
           in index order, exceeds target.
  T == 0   greedy: argmax, ties to the lowest index (exactly bl_argmax_f32); the weight pair is (1, 1).

Per row the outputs are the token id and the integer pair (w_token, total_kept); the log-probability of the drawn token
under the warped distribution is log(w_token / total_kept), taken on the host in fp64 (`logprob`) — the device never
computes a logarithm. The logits here are bf16-rounded fp32, so exact ties are common, also at the top-k and top-p
boundaries: every rule above is defined on ties. A greedy row (T == 0) is defined on NaN as well: np.argmax's answer,
the first NaN of the row (else the first maximum), so its id is always a token of the row; rows with T > 0 still require
logits free of NaN.

Scoring is the opposite direction: `score_row` / `score_rows` (device twin: `bl_score_f32`) take a GIVEN token and return
its pair (kept weight, total_kept) under the same warped distribution — no seed and no step, the score does not depend on
them. The defining property: for every token `sample_row` can draw from a row, `score_row` of that token returns
`sample_row`'s pair; a token that top-k or top-p removed, or whose weight rounds to 0, scores (0, total_kept), i.e.
log-probability -inf. `score_rows` also returns the kept weights of an index range (the 256 action bins, say): exact
per-token probabilities, and with `range_entropy` the entropy over that range.

A restricted policy: `vocab=(first, count)` on the four row functions makes the policy the softmax of
`l[first : first + count]` alone (device twins: `bl_sample_range_f32` / `bl_score_range_f32`). The definition is one line:
the result is what the function returns on that slice — maximum, top-k, top-p, the draw and the greedy argmax are all
taken over the slice — with token ids reported in full-vocabulary numbering. Every token outside the range has
probability 0 and is never read: it scores (0, total_kept), like a token that top-k removed. An OpenVLA action is one of
256 bins carried by token ids vocab_size - 256 … vocab_size - 1, so the action policy is `vocab=(31744, 256)`.

The domain (tests/test_sample_edge_gpu.py holds the kernels to all of it, on fp32 logits that are not bf16-rounded):
  logits   -inf is INSIDE the definition as long as the row maximum is finite: z = -inf, the clamp at -87 gives the weight
           rint(e^-87 · 2^30) = 0, so a masked token is never drawn and scores (0, total_kept). +inf and NaN are OUTSIDE
           for T > 0 (l - max would be NaN); a greedy row is defined on both, see above.
  T        0 (greedy), or any finite fp32 > 0: from 2^-100 (z overflows to -inf: only the maxima weigh) to 1e30 (z -> 0:
           every finite logit weighs 2^30). (l - max) / T is the IEEE fp32 QUOTIENT, not l - max times a rounded 1 / T.
  top_k    0 and every k >= n: off. 1 … n - 1: every tie at the k-th value stays; -0 and +0 are one value.
  top_p    any fp32 in (0, 1) through rint(top_p · 2^24): 1e-6 keeps the first-ranked token alone, 1 - 2^-24 (p24 =
           2^24 - 1) drops at most the lightest tail; zero weights are never kept or counted. >= 1: off.
  n        the kernels take multiples of 4 from 4 to 36 480; an all-maximum row of that width sums to 36 480 · 2^30 > 2^45,
           which the 70-bit top-p comparison and the uint64 running sums hold.
  step     0 … 2^31 - 1 (the Philox counter's first word).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np

WEIGHT_ONE = 1 << 30                 # weight of the row maximum
GOLDEN64 = 0x9E3779B97F4A7C15        # seed stride between the copies of `sample_actions`
_M64 = (1 << 64) - 1
_f32 = np.float32


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key) -> Tuple[np.ndarray, ...]:
    """counter: 4 words, key: 2 words (scalars or equal-shaped arrays) → the 4 output words as uint64 arrays < 2^32."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in key)
    m32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]          # 32 x 32 → 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
    return tuple(c)


def draw_u64(seed, t: int) -> np.ndarray:
    """The 64 random bits of generation step t for the sequence(s) with this seed (any integer; taken mod 2^64)."""
    s = np.asarray(seed).astype(np.int64, copy=False).astype(np.uint64) if not isinstance(seed, int) else np.uint64(seed & _M64)
    x = philox4x32_10((np.uint64(t), 0, 0, 0), (s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)))
    return (x[0] << np.uint64(32)) | x[1]


def mulhi64(a, b) -> np.ndarray:
    """High 64 bits of the 128-bit product of two uint64 (arrays): floor(a · b / 2^64)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    m, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    a0, a1, b0, b1 = a & m, a >> s, b & m, b >> s
    mid = (a0 * b0 >> s) + (a1 * b0 & m) + (a0 * b1 & m)
    return a1 * b1 + (a1 * b0 >> s) + (a0 * b1 >> s) + (mid >> s)


# ---- exp and the integer weights -----------------------------------------------------------------------------------------
_LOG2E, _LN2_HI, _LN2_LO = _f32(1.44269504), _f32(0.693359375), _f32(-2.12194440e-4)
_EXP_C = tuple(_f32(v) for v in (1.0 / 720, 1.0 / 120, 1.0 / 24, 1.0 / 6, 0.5, 1.0, 1.0))      # Taylor, degree 6 … 0


def exp_spec(x) -> np.ndarray:
    """e^x for x <= 0 in fp32, every operation individually rounded (numpy never contracts); the device twin is
    `exp_spec` in csrc/sample.hip under `#pragma clang fp contract(off)`. n·_LN2_HI is exact (9-bit constant, |n| <= 126),
    so r is the reduced argument to within an ulp; |r| <= 0.347. Max relative error: see tests/test_sampling_cpu.py."""
    x = np.maximum(np.asarray(x, dtype=_f32), _f32(-87.0))
    n = np.rint(x * _LOG2E)
    r = x - n * _LN2_HI
    r = r - n * _LN2_LO
    p = np.full_like(r, _EXP_C[0])
    for c in _EXP_C[1:]:
        p = p * r
        p = p + c
    scale = ((n.astype(np.int32) + 127) << 23).view(_f32)              # 2^n, n in [-126, 0]: a normal number
    return p * scale


def weights(logits, temperature) -> np.ndarray:
    """int64 weights of one row (before top-k / top-p): rint(exp_spec((l - max) / T) · 2^30)."""
    l = np.asarray(logits, dtype=_f32)
    z = (l - l.max()) / _f32(temperature)
    return np.rint(exp_spec(z) * _f32(WEIGHT_ONE)).astype(np.int64)


def kept_weights(logits, temperature, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """The row's weights with every token that top-k or top-p removes set to 0."""
    l = np.asarray(logits, dtype=_f32)
    w = weights(l, temperature)
    n = l.shape[0]
    if 0 < top_k < n:
        kth = np.partition(l, n - top_k)[n - top_k]
        w = np.where(l >= kth, w, 0)
    if _f32(top_p) < _f32(1.0):
        p24 = int(np.rint(_f32(top_p) * _f32(16777216.0)))
        order = np.argsort(-w, kind="stable")                          # w descending, index ascending
        ws = w[order]
        before = np.cumsum(ws) - ws
        keep = before < max(1, (p24 * int(ws.sum()) + (1 << 24) - 1) >> 24)      # Python integers: the product has 70 bits
        out = np.zeros_like(w)
        out[order[keep]] = ws[keep]
        w = out
    return w


def pick(kept: np.ndarray, u64) -> Tuple[np.ndarray, np.ndarray, int]:
    """Draw from kept weights with the random word(s) u64 → (token id(s), their weight(s), total_kept)."""
    run = np.cumsum(kept)
    total = int(run[-1])
    target = mulhi64(u64, np.uint64(total)).astype(np.int64)
    ids = np.searchsorted(run, target, side="right")
    return ids, kept[ids], total


def check_vocab(vocab, n: int, what: str = "vocab") -> Optional[Tuple[int, int]]:
    """None or (first, count) with the range inside [0, n) → the pair as Python integers; ValueError otherwise."""
    if vocab is None:
        return None
    first, count = int(vocab[0]), int(vocab[1])
    if first < 0 or count < 1 or first + count > n:
        raise ValueError(f"{what}: the token range [{first}, {first + count}) is empty or leaves [0, {n})")
    return first, count


def sample_row(logits, temperature: float, top_k: int, top_p: float, seed: int, t: int, vocab=None) -> Tuple[int, int, int]:
    """One row, one step → (token id, w_token, total_kept). vocab=(first, count): the same on l[first : first + count],
    the id in full-vocabulary numbering."""
    l = np.asarray(logits, dtype=_f32)
    vocab = check_vocab(vocab, l.shape[0], "sample_row")
    if vocab is not None:
        i, w, total = sample_row(l[vocab[0]:vocab[0] + vocab[1]], temperature, top_k, top_p, seed, t)
        return i + vocab[0], w, total
    if not _f32(temperature) > 0:
        return int(np.argmax(l)), 1, 1
    i, w, total = pick(kept_weights(l, temperature, int(top_k), float(top_p)), draw_u64(int(seed), t))
    return int(i), int(w), total


def sample_rows(logits, temperature, top_k, top_p, seed, t: int, vocab=None) -> Tuple[np.ndarray, np.ndarray]:
    """logits [rows, n] with one setting per row → ids int64 [rows], wt int64 [rows, 2] — what bl_sample_f32 writes
    (with vocab=(first, count): bl_sample_range_f32)."""
    l = np.asarray(logits, dtype=_f32)
    vocab = check_vocab(vocab, l.shape[1], "sample_rows")
    ids, wt = np.zeros(l.shape[0], np.int64), np.zeros((l.shape[0], 2), np.int64)
    for r in range(l.shape[0]):
        ids[r], wt[r, 0], wt[r, 1] = sample_row(l[r], temperature[r], top_k[r], top_p[r], int(seed[r]), t, vocab)
    return ids, wt


def score_row(logits, temperature: float, top_k: int, top_p: float, token: int, vocab=None) -> Tuple[int, int]:
    """One row, one given token → (w_token, total_kept): `sample_row`'s pair whenever it draws `token`. vocab=(first,
    count): the same on l[first : first + count]; a token outside the range scores (0, total_kept)."""
    l = np.asarray(logits, dtype=_f32)
    vocab = check_vocab(vocab, l.shape[0], "score_row")
    if vocab is not None:
        first, count = vocab
        inside = first <= int(token) < first + count
        w, total = score_row(l[first:first + count], temperature, top_k, top_p, int(token) - first if inside else 0)
        return (w if inside else 0), total
    if not _f32(temperature) > 0:
        return int(int(token) == int(np.argmax(l))), 1
    kept = kept_weights(l, temperature, int(top_k), float(top_p))
    return int(kept[int(token)]), int(kept.sum())


def score_rows(logits, temperature, top_k, top_p, tokens, first: int = 0, count: int = 0, vocab=None) -> Tuple[np.ndarray, np.ndarray]:
    """logits [rows, n] with one setting and one token per row → wt int64 [rows, 2] and range_wt int32 [rows, count] =
    the kept weights of tokens first … first + count - 1 (a greedy row: the one-hot of its argmax) — what bl_score_f32
    writes. vocab=(vfirst, vcount): the policy is over that token range (bl_score_range_f32); `first`, `count` and the
    tokens keep their full-vocabulary numbering, and the report range must lie inside `vocab`."""
    l = np.asarray(logits, dtype=_f32)
    rows, n = l.shape
    vocab = check_vocab(vocab, n, "score_rows")
    if vocab is not None:
        vf, vc = vocab
        if count < 0 or (count and (first < vf or first + count > vf + vc)):
            raise ValueError(f"score_rows: the range [{first}, {first + count}) leaves the token range [{vf}, {vf + vc})")
        tok = np.asarray(tokens, dtype=np.int64)
        if ((tok < 0) | (tok >= n)).any():
            raise ValueError(f"score_rows: a token is outside [0, {n})")
        inside = (tok >= vf) & (tok < vf + vc)
        wt, range_wt = score_rows(l[:, vf:vf + vc], temperature, top_k, top_p, np.where(inside, tok - vf, 0),
                                  first - vf if count else 0, count)
        wt[~inside, 0] = 0
        return wt, range_wt
    if count < 0 or (count and (first < 0 or first + count > n)):
        raise ValueError(f"score_rows: the range [{first}, {first + count}) leaves [0, {n})")
    wt, range_wt = np.zeros((rows, 2), np.int64), np.zeros((rows, count), np.int32)
    for r in range(rows):
        tok = int(tokens[r])
        if not 0 <= tok < n:
            raise ValueError(f"score_rows: token {tok} of row {r} is outside [0, {n})")
        if not _f32(temperature[r]) > 0:
            kept = np.zeros(n, np.int64)
            kept[int(np.argmax(l[r]))] = 1
        else:
            kept = kept_weights(l[r], temperature[r], int(top_k[r]), float(top_p[r]))
        wt[r] = kept[tok], kept.sum()
        range_wt[r] = kept[first:first + count]
    return wt, range_wt


def logprob(wt) -> np.ndarray:
    """fp64 log-probability of the drawn (or scored) tokens under the warped distribution, from weight pairs [..., 2];
    -inf where the weight is 0 (a scored token outside the support)."""
    wt = np.asarray(wt, dtype=np.float64)
    w, total = wt[..., 0], wt[..., 1]
    inside = w > 0
    return np.where(inside, np.log(np.where(inside, w, total) / total), -np.inf)


def range_entropy(range_wt, total_kept) -> Tuple[np.ndarray, np.ndarray]:
    """fp64 (-Σ p log p, Σ p) over a range of kept weights [..., count] with p = w / total_kept [...]: the entropy
    contribution of the range's tokens (0 · log 0 = 0) and the probability mass the range holds. The mass is 1 when the
    range covers the support, and the first value is then the entropy of the warped distribution."""
    w = np.asarray(range_wt, dtype=np.float64)
    p = w / np.asarray(total_kept, dtype=np.float64)[..., None]
    inside = w > 0
    return -(p * np.log(np.where(inside, p, 1.0))).sum(axis=-1), p.sum(axis=-1)


def derive_seed(seed, j: int) -> np.ndarray:
    """Seed of copy j of a sequence (`sample_actions`): seed + 0x9E3779B97F4A7C15·j mod 2^64, as int64 bit patterns."""
    s = np.atleast_1d(np.asarray(seed)).astype(np.int64).astype(np.uint64)
    return (s + np.uint64((GOLDEN64 * j) & _M64)).astype(np.int64)


# ---- settings ------------------------------------------------------------------------------------------------------------
@dataclass
class SamplingParams:
    """Sampling settings; every field is a scalar or one value per sequence. temperature 0 = greedy for that sequence.
    seed=None draws the per-sequence seeds from torch's default CPU generator (so `torch.manual_seed` makes a run
    repeatable)."""
    temperature: Any = 1.0
    top_k: Any = 0
    top_p: Any = 1.0
    seed: Optional[Any] = None

    def resolve(self, batch: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """→ (temperature f32 [B], top_k i32 [B], top_p f32 [B], seed i64 [B]); validates the values."""
        def per_row(v, dtype, what):
            a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != batch):
                raise ValueError(f"SamplingParams.{what}: a scalar or {batch} values, got shape {a.shape}")
            return np.ascontiguousarray(np.broadcast_to(a.astype(dtype), (batch,)))
        T, k, p = per_row(self.temperature, _f32, "temperature"), per_row(self.top_k, np.int64, "top_k"), per_row(self.top_p, _f32, "top_p")
        if not np.all(np.isfinite(T)) or np.any(T < 0):
            raise ValueError("SamplingParams.temperature must be finite and >= 0 (0 = greedy)")
        if np.any(k < 0) or np.any(k > np.iinfo(np.int32).max):
            raise ValueError("SamplingParams.top_k must be >= 0 (0 = off)")
        if np.any(np.isnan(p)) or np.any(p <= 0):
            raise ValueError("SamplingParams.top_p must be > 0 (>= 1 = off)")
        if self.seed is None:
            import torch
            seed = torch.randint(-(1 << 63), (1 << 63) - 1, (batch,), dtype=torch.int64).numpy()
        else:
            s = self.seed
            s = s.detach().cpu().numpy() if hasattr(s, "detach") else s
            flat = [int(v) & _M64 for v in np.asarray(s, dtype=object).reshape(-1)]
            if len(flat) not in (1, batch) or np.asarray(s, dtype=object).ndim > 1:
                raise ValueError(f"SamplingParams.seed: a scalar or {batch} values")
            seed = np.array(flat * (batch if len(flat) == 1 else 1), dtype=np.uint64).astype(np.int64)
        return T, k.astype(np.int32), p, seed
