"""bl_sample_f32 / bl_score_f32 and their _range twins (csrc/sample.hip, csrc/sample_spec.h) on the edge rows of
tests/gen_edge_ref.py, held to bridgelang_amd/sampling.py BIT FOR BIT: fp32 logits that are not bf16-rounded, temperatures
that are no power of two, the row widths at which a wave owns nothing, four elements or the full 160 KB LDS image, and the
value edges (−inf logits, clamped and zero weights, a single weight, totals above 2^45, T = 2^-100 … 1e30, top_k in
{1, n − 1, n, n + 5}, top_p = 1e-6 and 1 − 2^-24, ±0 at the k-th value, step 2^31 − 1). Every comparison is array_equal.

The census of gen_edge_ref (`assert_census`) is asserted on a case BEFORE the device is touched, so a GPU run is never
softer than tests/test_gen_edge_cpu.py; that file also proves that five wrong twins of the specification (reciprocal for
the divide, contracted exp, top-k on key >> 10, 16-bit top_p, the LAST m ties) each change rows of these cases.

Buffers: ld = n + 12; every column outside the policy (padding, and the columns outside a token range) holds NaN / +inf.
The scorer's range_wt covers the WHOLE policy and sits between 64-element guards, so every kept weight of every row is
compared; Σ range_wt == total_kept. Every launch is repeated over the same buffers and must give identical bits.

Branch → case (class names are gen_edge_ref.census's; widths are policy widths)
  key_of            negative logits (kinds kth*n: every key inverted), positive (kth*p), ±0 sharing a key at the k-th value
                    (topk_zero_tie), −inf (kind neg_inf: key 0x007fffff, weight 0)
  load loop         n 4, 8 (one, two active threads), 64, 68 (waves 1 … 15 own no index), 1024 (exactly one 16-byte pass for
                    256 threads), 4096 (one pass for all), 32064, 36480 (nine passes, the full LDS image); ranged: base 8 at
                    n 36488, base 31744 with 256 columns
  hist_add          leader path: kind flat (one bin holds the row), peaked, single_weight; scattered path: natural and wide rows
  select_bin<true>  the top bin: top_k 1; the lowest non-empty bin: top_k n − 1; need inside a bin shared by hundreds: top_k 50
  select_bin<false> the top bin: top_p 1e-6 and kind peaked (bound → the first-ranked weight); the lowest non-empty bin:
                    top_p 1 − 2^-24 (topp_zeros_skipped: zero weights never enter a histogram, every other weight stays)
  radix passes      topk_digit1 / 2 / 3 _pos / _neg: the k-th and (k + 1)-th keys differ in exactly one bit of that pass
                    (bit 21, 10, 0): a wrong shift or mask in a pass keeps k + 1 or k − 1 tokens; topp_digit1 / 2 / 3: w* and
                    the largest dropped weight first differ in that pass
  weights           T 0.7, 1.3, 0.9, fp32(1/3) (the IEEE divide: the rcp mutant changes 132 rows), T 2^-100 and 1e-3 (z → −inf,
                    the −87 clamp, weights 0), T 1e30 (every weight 2^30), kind wide (σ 60: most z below −87), −inf logits,
                    total_above_2_45 (flat and T = 1e30 rows at 36480 columns)
  top-p bound, m    the 70-bit product at totals above 2^45 with p24 = 2^24 − 1; bound 1 at top_p 1e-6; m < the number of
                    ties: kind flat with top_p < 1 and the integer tails of natural rows
  tie prefix        ties_across_waves: kept ties at w* in two or more wave spans and one tie dropped (n >= 68)
  target walk       draw_wave_0 … 15 (n >= 32064), draw_tail_wave (n 1028: index 1024 … 1027, a 4-element span),
                    draw_first_kept, draw_last_kept, draw_lane0, draw_lane63; steps 0, 3, 2^31 − 1
  greedy exit       every ninth row; its id is bl_argmax_f32's
  SCORE exits       forced_kept, forced_dropped_tie (weight w*, rank >= m), forced_below_kth, forced_weight_zero,
                    forced_last_span, forced_outside_range (ranged: below the base and above the range), greedy rows
"""
import numpy as np
import pytest
import torch

import gen_edge_ref as E

pytestmark = pytest.mark.gpu
GUARD = 64
IDS = ["-".join(map(str, s)) for s in E.SAMPLE_SHAPES]


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def _setup(shape, dev):
    """The case (census asserted first), then its rows on the device: ld = n + 12, NaN / +inf outside the policy."""
    n, first, count = shape
    case = E.sample_case(n, first, count, E.sample_rows_for(count))
    E.assert_census(case)
    rows = case.full.shape[0]
    buf = torch.empty(rows, n + 12)
    buf[:, 0::2], buf[:, 1::2] = float("nan"), float("inf")
    buf[:, :n] = torch.from_numpy(case.full.copy())
    assert bool(torch.isfinite(buf[:, first:first + count]).any(dim=1).all()) and not bool(torch.isfinite(buf[:, n:]).any())
    buf = buf.to(dev)
    d = lambda a: torch.from_numpy(a.copy()).to(dev)
    return case, buf, buf[:, :n], d(case.T), d(case.k), d(case.p)


def _rows_report(case, bad, *cols):
    return [(int(r), case.kinds[r], float(case.T[r]), int(case.k[r]), float(case.p[r])) + tuple(np.asarray(c[r]).tolist() for c in cols)
            for r in bad[:8]]


@pytest.mark.parametrize("shape", E.SAMPLE_SHAPES, ids=IDS)
def test_sampler_equals_specification(dev, shape):
    from bridgelang_amd import ops
    n, first, count = shape
    case, buf, logits, dT, dk, dp = _setup(shape, dev)
    rows = logits.shape[0]
    dseed = torch.from_numpy(case.seeds.copy()).to(dev)
    greedy = case.T == 0
    for step in E.STEPS:
        runs = []
        for _ in range(2):                                               # the second launch: identical bits
            ids = torch.full((rows,), -1, dtype=torch.int64, device=dev)
            wt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
            op = ops.sample(logits, dT, dk, dp, dseed, step, ids, wt, vocab=case.vocab)
            assert op.name == ("bl_sample_f32" if case.vocab is None else "bl_sample_range_f32")
            runs.append((ids.cpu().numpy(), wt.cpu().numpy()))
        got_ids, got_wt = runs[0]
        print(f"step {step}: ids equal {int((got_ids == case.ids[step]).sum())} / {rows}, "
              f"wt equal {int((got_wt == case.wt[step]).all(axis=1).sum())} / {rows}")
        bad = np.flatnonzero((got_ids != case.ids[step]) | (got_wt != case.wt[step]).any(axis=1))
        assert bad.size == 0, (step, _rows_report(case, bad, got_ids, case.ids[step], got_wt, case.wt[step]))
        assert np.array_equal(runs[1][0], got_ids) and np.array_equal(runs[1][1], got_wt), f"step {step}: a second launch differs"
        assert ((got_ids >= first) & (got_ids < first + count)).all() and (got_wt[greedy] == 1).all()
    arg = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    ops.argmax(buf[:, first:first + count], arg)                         # a greedy row IS bl_argmax_f32's answer on the policy's columns
    assert greedy.any() and np.array_equal(got_ids[greedy], first + arg.cpu().numpy()[greedy])


@pytest.mark.parametrize("shape", E.SAMPLE_SHAPES, ids=IDS)
def test_scorer_equals_specification(dev, shape):
    from bridgelang_amd import ops
    n, first, count = shape
    case, buf, logits, dT, dk, dp = _setup(shape, dev)
    rows = logits.shape[0]
    # the sampler's own draws score the sampler's pairs
    ids = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    swt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
    ops.sample(logits, dT, dk, dp, torch.from_numpy(case.seeds.copy()).to(dev), E.SEARCH_STEP, ids, swt, vocab=case.vocab)
    wt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
    op = ops.score(logits, dT, dk, dp, ids, wt, vocab=case.vocab)
    assert op.name == ("bl_score_f32" if case.vocab is None else "bl_score_range_f32")
    assert torch.equal(wt, swt) and np.array_equal(wt.cpu().numpy(), case.wt[E.SEARCH_STEP])
    # forced tokens, and the kept weight of every token of the policy
    dtok = torch.from_numpy(case.tok.copy()).to(dev)
    runs = []
    for _ in range(2):
        wt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
        flat = torch.full((rows * count + 2 * GUARD,), -1, dtype=torch.int32, device=dev)
        ops.score(logits, dT, dk, dp, dtok, wt, first, flat[GUARD:GUARD + rows * count].view(rows, count), vocab=case.vocab)
        runs.append((wt.cpu().numpy(), flat.cpu().numpy()))
    got_wt, got_flat = runs[0]
    assert (got_flat[:GUARD] == -1).all() and (got_flat[-GUARD:] == -1).all(), "range_wt written outside [rows, count]"
    got_rw = got_flat[GUARD:-GUARD].reshape(rows, count).astype(np.int64)
    print(f"wt equal {int((got_wt == case.tok_wt).all(axis=1).sum())} / {rows}, kept weights equal "
          f"{int((got_rw == case.kept).sum())} / {rows * count}")
    bad = np.flatnonzero((got_rw != case.kept).any(axis=1))
    assert bad.size == 0, _rows_report(case, bad, (got_rw != case.kept).sum(axis=1), got_rw.sum(axis=1), case.total)
    bad = np.flatnonzero((got_wt != case.tok_wt).any(axis=1))
    assert bad.size == 0, _rows_report(case, bad, case.tok, got_wt, case.tok_wt)
    assert np.array_equal(got_rw.sum(axis=1), got_wt[:, 1])              # Σ over the whole policy = total_kept
    assert np.array_equal(runs[1][0], got_wt) and np.array_equal(runs[1][1], got_flat), "a second launch differs"
