"""Edge inputs for the generation kernels (csrc/sample.hip, csrc/beam.hip) and the census that proves they bite. numpy only.

The sibling tests feed those kernels bf16-rounded randn·3 rows at power-of-two temperatures. Such rows leave the low 16 key
bits constant (the third radix pass and half of the second never tell two candidates apart) and make `(l − max) / T` exact
in any implementation. Everything here is fp32 and NOT bf16-rounded:

  key_of / logit_of / first_diff_digit   the uint32 order image of `sample.hip::key_of` and the radix digit (1: bits 21–31,
                                         2: bits 10–20, 3: bits 0–9) in which two keys first differ
  build_rows                             seeded rows of the kinds in KINDS with settings cycling T_COMMON / T_EXTREME / greedy,
                                         `k_cycle(n)` and P_CYCLE; seeds partly searched so that the draw lands where asked
  sample_case                            rows + the specification's answers (bridgelang_amd/sampling.py), once per shape
  restate                                a restatement of `sampling.kept_weights` on integer keys; with `mutant=` one of the
                                         MUTANTS, a deliberately wrong twin used only to prove that the rows tell it apart
  census / forced_census                 class name → rows, decided on the specification's outputs alone
  beam_case / beam_census                the same for `beam.beam_step`

Which classes a shape must hold is written down in `required_classes` / `required_beam_classes`, from the shape alone.
"""
import functools
from collections import namedtuple

import numpy as np

from bridgelang_amd import beam as BM
from bridgelang_amd import sampling as S

_f32 = np.float32
WAVES = 16
STEPS = (0, 3, (1 << 31) - 1)            # Philox counters: the first, the sibling tests', the largest the entry point takes
SEARCH_STEP = 3                          # the step the searched seeds aim at
KEY_ZERO = 0x80000000


# ---- keys --------------------------------------------------------------------------------------------------------------------
def key_of(l) -> np.ndarray:
    """uint32 keys whose unsigned order is the order of the fp32 values; −0 and +0 share the key 0x80000000."""
    l = np.asarray(l, dtype=_f32)
    b = np.ascontiguousarray(np.where(l == 0, _f32(0.0), l).astype(_f32)).view(np.uint32)
    return np.where((b >> np.uint32(31)) != 0, ~b, b | np.uint32(KEY_ZERO)).astype(np.uint32)


def logit_of(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    b = np.where((k >> np.uint32(31)) != 0, k ^ np.uint32(KEY_ZERO), ~k).astype(np.uint32)
    return np.ascontiguousarray(b).view(_f32)


def first_diff_digit(a, b) -> int:
    """The radix pass (1, 2, 3 = bits 21–31, 10–20, 0–9) that first tells the uint32 values a and b apart; 0 if equal."""
    x = int(a) ^ int(b)
    return 0 if x == 0 else 1 if x >> 21 else 2 if x >> 10 else 3


def wave_span(n: int) -> int:
    """Indices per wave in the kernel's walk: 16 waves, contiguous spans, a multiple of 64."""
    return ((n + WAVES - 1) // WAVES + 63) & ~63


# ---- settings and rows ---------------------------------------------------------------------------------------------------------
T_COMMON = (0.7, 1.3, 0.9, float(_f32(1.0) / _f32(3.0)), 1.0)
T_EXTREME = (2.0 ** -100, 1e-3, 1e30)
P_CYCLE = (1e-6, 0.5, 0.9, 0.95, float(np.nextafter(_f32(1.0), _f32(0.0))), 1.0)       # fp32 below 1.0 = 1 − 2^-24
KINDS = ("natural", "kth1p", "natural", "kth2p", "peaked", "kth3p", "natural", "kth1n", "wide", "kth2n", "natural", "kth3n",
         "neg_inf", "zero_kth", "natural", "flat")
GOALS = ("first", "last", "lane0", "lane63", "where")     # "where": a wave (n >= 32064) or the 4-element tail span (n = 1028)


def k_cycle(n: int):
    return (0, 1, 2, 50, n - 1, n, n + 5)


def _plant_kth(l, k, digit):
    """The (k+1)-th largest key becomes A, the k-th A + 2^s with bit s of A clear (s = 21, 10, 0 for digit 1, 2, 3): the two
    differ in exactly that bit. Keys below stay below (clamped to A), the other top-k keys stay at or above A + 2^s."""
    s = {1: 21, 2: 10, 3: 0}[digit]
    keys = key_of(l).astype(np.int64)
    order = np.argsort(-keys, kind="stable")
    top, rest = order[:k], order[k:]
    a = int(keys[rest[0]]) & ~(1 << s)
    keys[rest] = np.minimum(keys[rest], a)
    keys[top] = np.maximum(keys[top], a + (1 << s))
    keys[top[-1]] = a + (1 << s)
    return logit_of(keys.astype(np.uint32))


def _plant_zero(l, k, rng):
    """k − 2 positive entries, four zeros (+0, −0, +0, −0), the rest negative: the k-th largest value is 0."""
    n = l.shape[0]
    perm = rng.permutation(n)
    a = np.abs(l) + _f32(0.01)
    out = -a
    out[perm[:k - 2]] = a[perm[:k - 2]]
    out[perm[k - 2:k + 2]] = np.array([0.0, -0.0, 0.0, -0.0], dtype=_f32)
    return out.astype(_f32)


def build_rows(rows: int, n: int, seed: int):
    """→ l fp32 [rows, n], T fp32, k int32, p fp32 (one setting per row) and the row kinds. Deterministic in its arguments."""
    l = np.zeros((rows, n), _f32)
    T, k, p = np.zeros(rows, _f32), np.zeros(rows, np.int32), np.zeros(rows, _f32)
    kinds = []
    for r in range(rows):
        rng = np.random.default_rng([seed, n, r])
        kind = KINDS[r % len(KINDS)]
        T[r] = T_COMMON[r % len(T_COMMON)]
        if r % 11 == 7:
            T[r] = T_EXTREME[(r // 11) % len(T_EXTREME)]
        if r % 9 == 4:
            T[r] = 0.0                                                # greedy rows between the sampled ones
        k[r] = k_cycle(n)[r % 7]
        p[r] = P_CYCLE[(r + r // 16) % len(P_CYCLE)]
        x = (rng.standard_normal(n) * 3).astype(_f32)
        if kind.startswith("kth"):
            if not 0 < k[r] < n:
                k[r] = 1 + r % (n - 1)
            x = _plant_kth((x + _f32(-20.0 if kind[4] == "n" else 20.0)).astype(_f32), int(k[r]), int(kind[3]))
        elif kind == "zero_kth":
            if not 2 <= k[r] <= n - 2:
                k[r] = 2 + r % (n - 3)
            x = _plant_zero(x, int(k[r]), rng)
        elif kind == "peaked":
            x[int(rng.integers(n))] = x.max() + _f32(100.0)
        elif kind == "wide":
            x = (rng.standard_normal(n) * 60).astype(_f32)
        elif kind == "neg_inf":
            x[r % 3::3] = -np.inf
            if not np.isfinite(x).any():
                x[0] = _f32(0.5)
        elif kind == "flat":
            x[:] = _f32((-1.25, 3.0, 0.0, 17.3)[(r // 16) % 4])
        l[r] = x
        kinds.append(kind)
    return l, T, k, p, kinds


# ---- the specification restated on keys, and its mutants -----------------------------------------------------------------------
MUTANTS = ("rcp", "fma", "lowdigit", "p16", "tie_last")


def _fma(a, b, c):
    """One rounding for a·b + c: the fp32 product is exact in fp64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_f32)


def _exp_fma(x):
    """`sampling.exp_spec` with the two Cody–Waite steps and the six Horner steps contracted."""
    x = np.maximum(np.asarray(x, dtype=_f32), _f32(-87.0))
    n = np.rint(x * S._LOG2E)
    r = _fma(-n, S._LN2_HI, x)
    r = _fma(-n, S._LN2_LO, r)
    p = np.full_like(r, S._EXP_C[0])
    for c in S._EXP_C[1:]:
        p = _fma(p, r, c)
    return p * ((n.astype(np.int32) + 127) << 23).view(_f32)


def restate(l, T, k, p, mutant=None):
    """→ (weights after top-k, kept weights) of one row with T > 0. mutant=None: `sampling.kept_weights`, with top-k taken
    on the integer keys. Mutants: "rcp" z = d·fl(1/T); "fma" contracted exp; "lowdigit" top-k compares key >> 10; "p16"
    top_p quantised to 16 bits; "tie_last" of the ties at w* the last m stay instead of the first m."""
    l = np.asarray(l, dtype=_f32)
    n = l.shape[0]
    with np.errstate(all="ignore"):
        d = l - l.max()
        z = d * (_f32(1.0) / _f32(T)) if mutant == "rcp" else d / _f32(T)
        e = _exp_fma(z) if mutant == "fma" else S.exp_spec(z)
        w = np.rint(e * _f32(S.WEIGHT_ONE)).astype(np.int64)
    if 0 < k < n:
        keys = key_of(l)
        if mutant == "lowdigit":
            keys = keys >> np.uint32(10)
        w = np.where(keys >= np.partition(keys, n - k)[n - k], w, 0)
    wk = w
    if _f32(p) < _f32(1.0):
        p24 = int(np.rint(_f32(p) * _f32(16777216.0)))
        if mutant == "p16":
            p24 = int(np.rint(_f32(p) * _f32(65536.0))) << 8
        order = np.argsort(-w, kind="stable")
        ws = w[order]
        before = np.cumsum(ws) - ws
        keep = before < max(1, (p24 * int(ws.sum()) + (1 << 24) - 1) >> 24)
        out = np.zeros_like(w)
        out[order[keep]] = ws[keep]
        if mutant == "tie_last":
            wstar = out[out > 0].min()
            ties = np.flatnonzero(w == wstar)
            m = int(np.count_nonzero(out[ties]))
            out[ties] = 0
            out[ties[len(ties) - m:]] = wstar
        w = out
    return wk, w


# ---- a sampler / scorer case: rows, the specification's answers, once -----------------------------------------------------------
Case = namedtuple("Case", "n vocab full l T k p seeds kinds wk kept total ids wt tok tok_wt")


def _search_seed(run, total, goal, n, r):
    """The first of 4096 candidate seeds whose draw at SEARCH_STEP meets the goal, or None."""
    cand = (np.int64(r + 1) << np.int64(20)) + np.arange(4096, dtype=np.int64)
    with np.errstate(all="ignore"):
        idx = np.searchsorted(run, S.mulhi64(S.draw_u64(cand, SEARCH_STEP), np.uint64(total)).astype(np.int64), side="right")
    nz = np.flatnonzero(np.diff(np.concatenate([[0], run])))
    if goal == "first":
        hit = idx == nz[0]
    elif goal == "last":
        hit = idx == nz[-1]
    elif goal == "lane0":
        hit = idx % 64 == 0
    elif goal == "lane63":
        hit = idx % 64 == 63
    elif n == 1028:
        hit = idx >= 1024
    else:
        hit = idx // wave_span(n) == (r // 5) % WAVES
    hit = np.flatnonzero(hit)
    return int(cand[hit[0]]) if hit.size else None


def _forced(r, l, T, k, wk, kept, first, count, n):
    """The scorer's forced token of row r, in full-vocabulary numbering, cycling: a dropped tie at w*, a token below the
    k-th value, a token of weight 0, a token of the last wave span, a token outside the range, the maximum."""
    c = (r + r // 6) % 6
    span = wave_span(count)
    last_lo = (count - 1) // span * span
    fallback = last_lo + (r * 7) % (count - last_lo)
    if not T > 0:
        return first + (int(np.argmax(l)) if c == 5 else fallback)
    if c == 0:
        nz = kept[kept > 0]
        drop = np.flatnonzero((wk == nz.min()) & (kept == 0))
        return first + (int(drop[0]) if drop.size else fallback)
    if c == 1:
        keys = key_of(l)
        below = np.flatnonzero(keys < np.sort(keys)[count - k]) if 0 < k < count else np.array([], int)
        return first + (int(below[len(below) // 2]) if below.size else int(np.argmin(l)))
    if c == 2:
        zero = np.flatnonzero(wk == 0)
        return first + (int(zero[-1]) if zero.size else int(np.argmin(l)))
    if c == 3:
        return first + fallback
    if c == 4:
        outside = [t for t in (first - 1, first + count, 0, n - 1) if 0 <= t < n and not first <= t < first + count]
        return outside[r % len(outside)] if outside else first + fallback
    return first + int(np.argmax(l))


@functools.lru_cache(maxsize=None)
def sample_case(n: int, first: int, count: int, rows: int) -> Case:
    """Rows of `n` columns whose policy is the columns [first, first + count); every column outside it holds NaN / +inf.
    The answers are the specification's: `kept` = `sampling.kept_weights` per row (a greedy row: the one-hot of its
    argmax), ids / wt per step of STEPS = `sampling.pick` on them with `sampling.draw_u64` — what `sampling.sample_rows`
    computes, the weights taken once instead of once per step — and the forced tokens' pairs as `sampling.score_rows`."""
    seed = 7 * n + first + count
    l, T, k, p, kinds = build_rows(rows, count, seed)
    seeds = np.random.default_rng(seed).integers(-(1 << 63), (1 << 63) - 1, rows, dtype=np.int64)
    wk, kept, total = np.zeros((rows, count), np.int64), np.zeros((rows, count), np.int64), np.zeros(rows, np.int64)
    tok = np.zeros(rows, np.int64)
    for r in range(rows):
        if T[r] > 0:
            with np.errstate(all="ignore"):
                kept[r] = S.kept_weights(l[r], T[r], int(k[r]), float(p[r]))
            wk[r] = restate(l[r], T[r], int(k[r]), 1.0)[0]
            if r % 3:                                                 # two rows in three aim their draw
                got = _search_seed(np.cumsum(kept[r]), int(kept[r].sum()), GOALS[(r + r // 5) % len(GOALS)], count, r)
                seeds[r] = seeds[r] if got is None else got
        else:
            kept[r, int(np.argmax(l[r]))] = 1
            wk[r] = kept[r]
        total[r] = kept[r].sum()
        tok[r] = _forced(r, l[r], T[r], int(k[r]), wk[r], kept[r], first, count, n)
    ids, wt = {}, {}
    for t in STEPS:
        ids[t], wt[t] = np.zeros(rows, np.int64), np.ones((rows, 2), np.int64)
        for r in range(rows):
            if T[r] > 0:
                with np.errstate(all="ignore"):
                    i, w, tot = S.pick(kept[r], S.draw_u64(int(seeds[r]), t))
                ids[t][r], wt[t][r] = first + int(i), (int(w), tot)
            else:
                ids[t][r] = first + int(np.argmax(l[r]))
    inside = (tok >= first) & (tok < first + count)
    tok_wt = np.stack([np.where(inside, kept[np.arange(rows), np.where(inside, tok - first, 0)], 0), total], axis=1)
    full = np.empty((rows, n), _f32)
    full[:, 0::2], full[:, 1::2] = np.nan, np.inf
    full[:, first:first + count] = l
    vocab = None if (first, count) == (0, n) else (first, count)
    for a in (full, l, T, k, p, seeds, wk, kept, total, tok, tok_wt, *ids.values(), *wt.values()):
        a.setflags(write=False)
    return Case(n, vocab, full, l, T, k, p, seeds, tuple(kinds), wk, kept, total, ids, wt, tok, tok_wt)


# ---- census ----------------------------------------------------------------------------------------------------------------------
def census(case: Case) -> dict:
    """Class name → rows, from the rows and the specification's outputs alone."""
    count = case.l.shape[1]
    span = wave_span(count)
    names = [f"topk_digit{d}_{s}" for d in (1, 2, 3) for s in ("pos", "neg")] + ["topk_zero_tie"] + \
            [f"topp_digit{d}" for d in (1, 2, 3)] + ["topp_zeros_skipped", "ties_across_waves", "single_weight", "total_above_2_45"] + \
            [f"draw_wave_{w}" for w in range(WAVES)] + ["draw_tail_wave", "draw_first_kept", "draw_last_kept", "draw_lane0", "draw_lane63"]
    out = {name: set() for name in names}
    for r in range(case.l.shape[0]):
        if not case.T[r] > 0:
            continue
        l, k, p, wk, kept = case.l[r], int(case.k[r]), case.p[r], case.wk[r], case.kept[r]
        if 0 < k < count:
            sk = np.sort(key_of(l))[::-1]
            kth, nxt = int(sk[k - 1]), int(sk[k])
            if kth != nxt:
                out[f"topk_digit{first_diff_digit(kth, nxt)}_{'pos' if kth >> 31 else 'neg'}"].add(r)
            zeros = l[l == 0]
            if kth == KEY_ZERO and np.signbit(zeros).any() and not np.signbit(zeros).all():
                out["topk_zero_tie"].add(r)
        nz = np.flatnonzero(kept)
        if _f32(p) < _f32(1.0):
            wstar = int(kept[nz].min())
            dropped = wk[(kept == 0) & (wk > 0) & (wk < wstar)]
            if dropped.size:
                out[f"topp_digit{first_diff_digit(wstar, int(dropped.max()))}"].add(r)
            if (wk == 0).any() and np.array_equal(wk, kept):
                out["topp_zeros_skipped"].add(r)
            ties = np.flatnonzero(wk == wstar)
            stay = ties[kept[ties] > 0]
            if stay.size < ties.size and np.unique(stay // span).size >= 2:
                out["ties_across_waves"].add(r)
        if case.total[r] == S.WEIGHT_ONE:
            out["single_weight"].add(r)
        if int(wk.sum()) > 1 << 45:
            out["total_above_2_45"].add(r)
        first = 0 if case.vocab is None else case.vocab[0]
        for t in STEPS:
            i = int(case.ids[t][r]) - first
            if count >= 32064:
                out[f"draw_wave_{i // span}"].add(r)
            if count == 1028 and i >= 1024:
                out["draw_tail_wave"].add(r)
            if i == nz[0]:
                out["draw_first_kept"].add(r)
            if i == nz[-1]:
                out["draw_last_kept"].add(r)
            if i % 64 == 0:
                out["draw_lane0"].add(r)
            if i % 64 == 63:
                out["draw_lane63"].add(r)
    return {name: sorted(v) for name, v in out.items()}


def required_classes(count: int) -> list:
    """The classes a policy of `count` columns must hold, from the width alone. The top-k plants, the zero tie, the single
    weight and the skipped zeros exist at every width (n = 4 included); lane 63 needs 64 columns, ties in two wave spans
    need two spans (n >= 68). Where top-p cuts depends on how close neighbouring weights lie: digit 1 from 64 columns on,
    digit 2 from 1024, digit 3 (two weights that differ below 2^10) only among the 32 064 natural weights. A total above 2^45
    needs more than 32 768 maxima; the wave classes are asked for where every wave owns more than 2000 columns."""
    req = [f"topk_digit{d}_{s}" for d in (1, 2, 3) for s in ("pos", "neg")]
    req += ["topk_zero_tie", "single_weight", "topp_zeros_skipped", "draw_first_kept", "draw_last_kept", "draw_lane0"]
    if count >= 64:
        req += ["draw_lane63", "topp_digit1"]
    if count >= 68:
        req += ["ties_across_waves"]
    if count >= 1024:
        req += ["topp_digit2"]
    if count == 1028:
        req += ["draw_tail_wave"]
    if count >= 32064:
        req += ["topp_digit3"] + [f"draw_wave_{w}" for w in range(WAVES)]
    if count >= 36480:
        req += ["total_above_2_45"]
    return req


FORCED = ("forced_dropped_tie", "forced_below_kth", "forced_weight_zero", "forced_last_span", "forced_outside_range", "forced_kept")


def forced_census(case: Case) -> dict:
    """Class name → rows whose forced token falls in it."""
    count = case.l.shape[1]
    first = 0 if case.vocab is None else case.vocab[0]
    span = wave_span(count)
    out = {name: [] for name in FORCED}
    for r in range(case.l.shape[0]):
        t = int(case.tok[r]) - first
        if not 0 <= t < count:
            assert case.tok_wt[r, 0] == 0
            out["forced_outside_range"].append(r)
            continue
        if t >= (count - 1) // span * span:
            out["forced_last_span"].append(r)
        if not case.T[r] > 0:
            continue
        l, k, wk, kept = case.l[r], int(case.k[r]), case.wk[r], case.kept[r]
        if kept[t] > 0:
            out["forced_kept"].append(r)
        elif wk[t] > 0 and wk[t] == kept[kept > 0].min():
            out["forced_dropped_tie"].append(r)
        if 0 < k < count and key_of(l[t]) < np.sort(key_of(l))[count - k]:
            out["forced_below_kth"].append(r)
        with np.errstate(all="ignore"):
            if S.weights(l, case.T[r])[t] == 0:
                out["forced_weight_zero"].append(r)
    return out


def assert_census(case: Case) -> None:
    got, forced = census(case), forced_census(case)
    count = case.l.shape[1]
    empty = [name for name in required_classes(count) if not got[name]]
    need = [name for name in FORCED if name != "forced_outside_range" or case.vocab is not None]
    if count < 64:
        need.remove("forced_dropped_tie")                             # 64 rows of 4 or 8 columns: no tie is dropped at a forced token's turn
    empty += [name for name in need if not forced[name]]
    assert not empty, (case.n, case.vocab, f"empty classes {empty}", {n: len(v) for n, v in {**got, **forced}.items()})


def mutant_rows(case: Case, mutant: str) -> list:
    """Rows of the case on which the mutant keeps other weights than the specification (so other ids or wt can follow)."""
    return [r for r in range(case.l.shape[0]) if case.T[r] > 0 and
            not np.array_equal(restate(case.l[r], case.T[r], int(case.k[r]), float(case.p[r]), mutant)[1], case.kept[r])]


# ---- beam -------------------------------------------------------------------------------------------------------------------------
BeamCase = namedtuple("BeamCase", "W n vocab full l s tok par wt sc")
BEAM_CLASSES = ("owner_same_row", "owner_other_row", "owner_other_sweep", "all_dead", "lz_zero", "lz_big_true", "lz_big_false",
                "neg_inf_logit", "dead_beam", "score_1e30", "total_above_2_45")
SWEEP = 4096                             # columns one sweep of the step kernel covers


@functools.lru_cache(maxsize=None)
def beam_case(groups: int, W: int, n: int, vocab) -> BeamCase:
    """fp32 rows with plants per prompt, and `beam.beam_step`'s answers. Per prompt, at policy columns c0 (a multiple of 4):
      rows 0 and 1   twins (logits and score −0.25); their best candidates are c0 and c0 + 1 (one thread's four columns) and,
                     between the two where the policy is wider than a sweep, c0 + 4096 (the same thread, the next sweep)
      row 2          peaked: one logit 100 above the rest, so total = 2^30 and lz = 0; score −1
      row 3          dead (score −inf); three equal maxima 100 above the rest: total = 3·2^30, mantissa 1.5 > 1.41421354
      row 4          score −1e30
      row 5          all logits equal: total = count·2^30 (above 2^45 at 36 480 columns), every candidate of the row ties
      rows 6 …       natural, every fifth logit −inf, scores −3 − 4·|randn|
    With one beam the row is row 0. The last of several prompts has ALL scores −inf. Columns outside the policy hold NaN / +inf."""
    first, count = vocab if vocab is not None else (0, n)
    rng = np.random.default_rng([groups, W, n, first])
    rows = groups * W
    l = (rng.standard_normal((rows, count)) * 3).astype(_f32)
    s = (-3 - 4 * np.abs(rng.standard_normal(rows))).astype(_f32)
    for g in range(groups):
        r0 = g * W
        c0 = 4 * int(rng.integers(max(1, (min(count - SWEEP, SWEEP) if count > SWEEP else count - 4) // 4)))
        l[r0, 3::7] = -np.inf
        top = l[r0].max()
        l[r0, c0], l[r0, c0 + 1] = top + _f32(2.0), top + _f32(1.5)
        if count > SWEEP:
            l[r0, c0 + SWEEP] = top + _f32(1.75)
        s[r0] = -0.25
        if W >= 2:
            l[r0 + 1], s[r0 + 1] = l[r0], s[r0]
        if W >= 3:
            l[r0 + 2, int(rng.integers(count))] = l[r0 + 2].max() + _f32(100.0)
            s[r0 + 2] = -1.0
        if W >= 4:
            l[r0 + 3, rng.permutation(count)[:3]] = l[r0 + 3].max() + _f32(100.0)
            s[r0 + 3] = -np.inf
        if W >= 5:
            s[r0 + 4] = -1e30
        for j in range(4, W):
            l[r0 + j, j % 5::5] = -np.inf
            if not np.isfinite(l[r0 + j]).any():
                l[r0 + j, 0] = 0.0
        if W >= 6:
            l[r0 + 5] = _f32(1.5)
    if groups >= 2:
        s[(groups - 1) * W:] = -np.inf
    full = np.empty((rows, n), _f32)
    full[:, 0::2], full[:, 1::2] = np.nan, np.inf
    full[:, first:first + count] = l
    want = [BM.beam_step(full[g * W:(g + 1) * W], s[g * W:(g + 1) * W], (first, count)) for g in range(groups)]
    tok, par, wt, sc = (np.concatenate([w[i] for w in want]) for i in range(4))
    for a in (full, l, s, tok, par, wt, sc):
        a.setflags(write=False)
    return BeamCase(W, n, vocab, full, l, s, tok, par, wt, sc)


def beam_census(case: BeamCase) -> dict:
    """Class name → prompts (the lz and input classes: rows), from the inputs and the specification's survivors alone."""
    W = case.W
    first = 0 if case.vocab is None else case.vocab[0]
    out = {name: [] for name in BEAM_CLASSES}
    rows = case.l.shape[0]
    for g in range(rows // W):
        sl = slice(g * W, (g + 1) * W)
        if np.all(np.isneginf(case.s[sl])):
            out["all_dead"].append(g)
        i, j = case.tok[sl] - first, case.par[sl]
        pairs = [(a, b) for a in range(W) for b in range(a + 1, W)]
        if any(j[a] == j[b] and i[a] // 4 == i[b] // 4 for a, b in pairs):
            out["owner_same_row"].append(g)
        if any(j[a] != j[b] and i[a] // 4 == i[b] // 4 for a, b in pairs):
            out["owner_other_row"].append(g)
        if any((i[a] % SWEEP) // 4 == (i[b] % SWEEP) // 4 and i[a] // SWEEP != i[b] // SWEEP for a, b in pairs):
            out["owner_other_sweep"].append(g)
    for r in range(rows):
        total = int(S.weights(case.l[r], 1.0).sum())
        x = np.array([total], np.int64).astype(_f32) * _f32(2.0 ** -30)
        if BM.log_spec(x)[0] == 0 and total == S.WEIGHT_ONE:
            out["lz_zero"].append(r)
        m = ((x.view(np.uint32) & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(_f32)[0]
        out["lz_big_true" if m > BM._SQRT2 else "lz_big_false"].append(r)
        if np.isneginf(case.l[r]).any():
            out["neg_inf_logit"].append(r)
        if np.isneginf(case.s[r]) and not np.all(np.isneginf(case.s[r // W * W:(r // W + 1) * W])):
            out["dead_beam"].append(r)
        if case.s[r] == _f32(-1e30):
            out["score_1e30"].append(r)
        if total > 1 << 45:
            out["total_above_2_45"].append(r)
    return out


def required_beam_classes(groups: int, W: int, count: int) -> list:
    """From the shape alone: the plants of `beam_case` need the rows they sit on (docstring there); the last of several
    prompts is dead, so a shape with two prompts of one beam holds the all-dead class and the row classes of prompt 0."""
    req = ["neg_inf_logit"]
    if groups >= 2:
        req += ["all_dead"]
    if W >= 4:
        req += ["owner_same_row", "owner_other_row", "lz_zero", "lz_big_true", "lz_big_false", "dead_beam"]
    if W >= 5:
        req += ["score_1e30"]
        if count > SWEEP:
            req += ["owner_other_sweep"]
    if W >= 6 and count >= 36480:
        req += ["total_above_2_45"]
    return req


def assert_beam_census(groups: int, case: BeamCase) -> None:
    got = beam_census(case)
    count = case.l.shape[1]
    empty = [name for name in required_beam_classes(groups, case.W, count) if not got[name]]
    assert not empty, (groups, case.W, case.n, case.vocab, f"empty classes {empty}", {n: len(v) for n, v in got.items()})


# ---- the shapes the GPU tests run --------------------------------------------------------------------------------------------------
SAMPLE_SHAPES = [(n, 0, n) for n in (4, 8, 64, 68, 1024, 1028, 4096, 32064, 36480)] + [(36488, 8, 36480), (32064, 31744, 256)]
BEAM_SHAPES = [(2, 1, 4, None), (1, 4, 4, None), (2, 4, 8, None), (2, 16, 4096, None), (2, 16, 4100, None), (1, 16, 8196, None),
               (1, 16, 36480, None), (2, 5, 36488, (8, 36480)), (2, 4, 32064, (31744, 256))]


def sample_rows_for(count: int) -> int:
    return 256 if count >= 32064 else 64
