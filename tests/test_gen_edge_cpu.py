"""The edge cases of tests/gen_edge_ref.py on the CPU: every case list the GPU tests run (test_sample_edge_gpu.py,
test_beam_edge_gpu.py) holds every class it is meant to hold, its answers are the specification's, every mutant of the
specification changes some row of it, and the builders are deterministic. Every comparison is exact."""
import numpy as np
import pytest

from bridgelang_amd import beam as BM
from bridgelang_amd import sampling as S

import gen_edge_ref as E


def _case(shape):
    n, first, count = shape
    return E.sample_case(n, first, count, E.sample_rows_for(count))


def test_key_helpers():
    v = np.array([-np.inf, -3e38, -20.5, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 20.5, 3e38], np.float32)
    k = E.key_of(v)
    assert k.dtype == np.uint32 and k[5] == k[6] == E.KEY_ZERO and np.all(np.diff(k.astype(np.int64))[[0, 1, 2, 3, 4, 6, 7, 8, 9]] > 0)
    back = E.logit_of(k)
    assert np.array_equal(back[[0, 1, 2, 3, 4, 7, 8, 9, 10]], v[[0, 1, 2, 3, 4, 7, 8, 9, 10]]) and not np.signbit(back[5])
    assert [E.first_diff_digit(5, 5), E.first_diff_digit(1 << 21, 0), E.first_diff_digit(1 << 20, 0), E.first_diff_digit(1 << 10, 0),
            E.first_diff_digit(1 << 9, 0), E.first_diff_digit(1, 0), E.first_diff_digit(1 << 31, 1)] == [0, 1, 2, 2, 3, 3, 1]
    assert [E.wave_span(n) for n in (4, 68, 1024, 1028, 32064, 36480)] == [64, 64, 64, 128, 2048, 2304]


@pytest.mark.parametrize("shape", E.SAMPLE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_sample_case_holds_its_classes(shape):
    case = _case(shape)
    print({name: len(v) for name, v in {**E.census(case), **E.forced_census(case)}.items() if v})
    E.assert_census(case)
    count = shape[2]
    rows = case.l.shape[0]
    assert np.isfinite(case.l.max(axis=1)).all() and not np.isnan(case.l).any() and not np.isposinf(case.l).any()
    assert np.isneginf(case.l).any() and (case.T == 0).sum() >= rows // 9
    assert {float(t) for t in case.T} >= {float(np.float32(t)) for t in E.T_COMMON + E.T_EXTREME}
    assert {int(k) for k in case.k} >= {0, 1, count - 1, count, count + 5} and {float(p) for p in case.p} == {float(np.float32(p)) for p in E.P_CYCLE}
    assert ((case.l.view(np.uint32) & 0xFFFF) != 0).mean() > 0.5                                  # fp32, not bf16-rounded
    # the restatement on keys is the specification, and Σ kept = total_kept
    for r in range(0, rows, 1 if count <= 4096 else 8):
        if case.T[r] > 0:
            assert np.array_equal(E.restate(case.l[r], case.T[r], int(case.k[r]), float(case.p[r]))[1], case.kept[r]), r
    assert np.array_equal(case.kept.sum(axis=1), case.total) and (case.kept >= 0).all() and case.kept.max() <= S.WEIGHT_ONE


@pytest.mark.parametrize("shape", [s for s in E.SAMPLE_SHAPES if s[2] <= 4096], ids=lambda s: "-".join(map(str, s)))
def test_sample_case_answers_are_sample_rows_and_score_rows(shape):
    """The case takes every row's weights once and draws from them per step; here the specification's own row functions
    run on the full rows (NaN / +inf outside the policy) and must give the same."""
    case = _case(shape)
    n, first, count = shape
    with np.errstate(all="ignore"):
        for t in E.STEPS:
            ids, wt = S.sample_rows(case.full, case.T, case.k, case.p, case.seeds, t, vocab=case.vocab)
            assert np.array_equal(ids, case.ids[t]) and np.array_equal(wt, case.wt[t]), t
        wt, full = S.score_rows(case.full, case.T, case.k, case.p, case.tok, first, count, vocab=case.vocab)
    assert np.array_equal(wt, case.tok_wt) and np.array_equal(full, case.kept)
    assert not np.array_equal(case.ids[0], case.ids[3]) and not np.array_equal(case.ids[3], case.ids[E.STEPS[2]])


def test_every_mutant_changes_the_new_rows():
    counts = {m: 0 for m in E.MUTANTS}
    for shape in E.SAMPLE_SHAPES:
        if shape[2] > 32064:
            continue
        case = _case(shape)
        here = {m: len(E.mutant_rows(case, m)) for m in E.MUTANTS}
        print(shape, here)
        assert all(here.values()), (shape, here)
        for m in E.MUTANTS:
            counts[m] += here[m]
    print("rows changed per mutant:", counts)


def test_rcp_mutant_is_invisible_on_the_sibling_rows():
    """Why the new rows exist: at T in {0.5, 1, 2} the quotient (l − max) / T is exact, so d · fl(1/T) changes nothing."""
    from test_sampling_gpu import _rows
    l, T, k, p, _ = _rows(256, 32064, seed=256 + 32064)
    for r in range(256):
        if T[r] > 0:
            want = S.kept_weights(l[r], T[r], int(k[r]), float(p[r]))
            assert np.array_equal(E.restate(l[r], T[r], int(k[r]), float(p[r]), "rcp")[1], want), r


@pytest.mark.parametrize("shape", E.BEAM_SHAPES, ids=lambda s: "-".join(map(str, s[:3])))
def test_beam_case_holds_its_classes(shape):
    groups, W, n, vocab = shape
    case = E.beam_case(*shape)
    print({name: len(v) for name, v in E.beam_census(case).items()})
    E.assert_beam_census(groups, case)
    first, count = vocab if vocab is not None else (0, n)
    assert np.isfinite(case.l.max(axis=1)).all() and not np.isnan(case.l).any() and not np.isposinf(case.l).any()
    assert ((case.par >= 0) & (case.par < W)).all() and ((case.tok >= first) & (case.tok < first + count)).all()
    assert (case.l.view(np.uint32) & 0xFFFF).any()
    for g in range(groups):                                              # survivors come best first
        keys = BM.order_key(case.sc[g * W:(g + 1) * W]).astype(np.int64)
        assert np.all(np.diff(keys) <= 0)


def test_builders_are_deterministic():
    a, b = E.build_rows(64, 68, 5), E.build_rows(64, 68, 5)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    assert not np.array_equal(a[0], E.build_rows(64, 68, 6)[0])
    c, d = E.sample_case.__wrapped__(1028, 0, 1028, 64), E.sample_case.__wrapped__(1028, 0, 1028, 64)
    for name in ("full", "T", "k", "p", "seeds", "kept", "tok", "tok_wt"):
        assert np.array_equal(getattr(c, name), getattr(d, name), equal_nan=True), name
    assert all(np.array_equal(c.ids[t], d.ids[t]) and np.array_equal(c.wt[t], d.wt[t]) for t in E.STEPS)
    e, f = E.beam_case.__wrapped__(2, 16, 4100, None), E.beam_case.__wrapped__(2, 16, 4100, None)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(e[3:], f[3:]))
