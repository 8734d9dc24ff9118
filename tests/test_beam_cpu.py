"""Beam search over the action tokens, host side (no GPU): `bridgelang_amd.beam` — the specification the kernel
bl_beam_step_f32 is held to — and the argument checks of the model surface and the engine that need no device."""
import itertools

import numpy as np
import pytest
import torch

from bridgelang_amd import beam as BM
from bridgelang_amd import sampling as S

F32 = np.float32


def bf16(x) -> np.ndarray:
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def rows_bf16(seed: int, W: int, n: int, scale: float = 2.0) -> np.ndarray:
    return bf16(np.random.default_rng(seed).standard_normal((W, n)) * scale)


# ---- log_spec ------------------------------------------------------------------------------------------------------------
def test_log_spec_accuracy():
    """|log_spec(x) - ln x| <= 2^-24 · (ln x + 1.5) on [1, 32 064] — the bound beam.log_spec derives in its docstring from
    the series' remainder (0.04 u), the roundings of s and of the correction (1.12 u on ln m), e·LN2_LO and its sum
    (0.36 u) and the last sum (u · ln x)."""
    pows = 2.0 ** np.arange(0, 15)
    near = [np.nextafter(F32(p * f), F32(d), dtype=F32) for p in pows for f in (1.0, np.sqrt(2.0)) for d in (0.0, np.inf)]
    chain = []
    for p in list(pows) + list(pows * np.sqrt(2.0)):      # the neighbours on both sides, 4 ulps deep
        lo = hi = F32(p)
        for _ in range(4):
            lo, hi = np.nextafter(lo, F32(0), dtype=F32), np.nextafter(hi, F32(np.inf), dtype=F32)
            chain += [lo, hi]
    x = np.concatenate([np.geomspace(1.0, 32064.0, 2_000_000).astype(F32), np.arange(1, 32065, dtype=F32), pows.astype(F32),
                        (pows * np.sqrt(2.0)).astype(F32), np.array(near + chain, dtype=F32), np.array([32064.0], dtype=F32)])
    x = np.unique(x[(x >= 1) & (x <= 32064)])
    ref = np.log(x.astype(np.float64))
    got = BM.log_spec(x)
    assert got.dtype == F32 and got[0] == 0.0                                    # ln 1 = 0 exactly
    err, bound = np.abs(got.astype(np.float64) - ref), 2.0 ** -24 * (ref + 1.5)
    print(f"log_spec: {x.size} arguments, max |err| = {err.max():.3e} at x = {x[err.argmax()]!r}, "
          f"max err / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), (err / bound).max()


# ---- beam_step -----------------------------------------------------------------------------------------------------------
def test_one_beam_is_the_argmax_lowest_index_on_ties():
    for seed in range(5):
        l = rows_bf16(seed, 1, 260)
        l[0, [200, 17, 99]] = l.max() + F32(1.0)                                 # three equal maxima
        tok, par, wt, sc = BM.beam_step(l, BM.start_scores(1))
        assert tok.tolist() == [17] == [int(np.argmax(l[0]))] and par.tolist() == [0]
        assert wt[0, 0] == S.WEIGHT_ONE and tok.dtype == np.int64 and par.dtype == np.int32 and sc.dtype == F32


def test_planted_ties_resolve_by_flat_index():
    row = np.array([0, 3, 3, 1, -2, 0.5, 3, -1], dtype=F32)                      # tokens 1, 2 and 6 tie inside the row
    l = np.stack([row, row, row])
    tok, par, _, sc = BM.beam_step(l, np.array([0, 0, -5], dtype=F32))           # beams 0 and 1 tie across rows
    assert tok.tolist() == [1, 2, 6] and par.tolist() == [0, 0, 0] and sc[0] == sc[1] == sc[2]
    tok, par, _, sc = BM.beam_step(np.stack([row, row, row, row]), np.array([-5, 0, -5, 0], dtype=F32))
    assert list(zip(par.tolist(), tok.tolist())) == [(1, 1), (1, 2), (1, 6), (3, 1)] and len(set(sc.tolist())) == 1
    # -inf scores order by index too: two live candidates, the dead ones follow in flat order
    l2 = np.full((3, 4), -np.inf, dtype=F32)
    l2[:, 2], l2[:, 3] = 1.0, 0.0
    tok, par, _, sc = BM.beam_step(l2, BM.start_scores(3))
    assert list(zip(par.tolist(), tok.tolist())) == [(0, 2), (0, 3), (0, 0)] and sc[2] == -np.inf


@pytest.mark.parametrize("W", [2, 5, 16])
def test_start_vector_weights_and_vocab(W):
    n, first, count = 260, 128, 64
    l = rows_bf16(10 + W, W, n)
    l[:] = l[0]                                                                 # step 0: the beams are identical rows
    tok, par, wt, sc = BM.beam_step(l, BM.start_scores(W))
    assert np.all(par == 0) and tok.tolist() == np.argsort(-l[0], kind="stable")[:W].tolist()
    assert np.all(np.diff(sc) <= 0) and np.all(np.isfinite(sc))
    # a later step: every row its own logits and score, one beam dead
    l = rows_bf16(20 + W, W, n)
    s = (np.random.default_rng(W).standard_normal(W) * 2 - 5).astype(F32)
    s[W // 2] = -np.inf
    one = np.ones(W, F32)
    for vocab in (None, (first, count)):
        tok, par, wt, sc = BM.beam_step(l, s, vocab)
        assert np.all(par != W // 2) and np.all((par >= 0) & (par < W))
        want, _ = S.score_rows(l[par], one, np.zeros(W, np.int32), one, tok, vocab=vocab)
        assert np.array_equal(wt, want), "wt is score_rows' pair of the chosen (row, token), bit for bit"
        flat = par.astype(np.int64) * n + tok
        assert all((sc[k] > sc[k + 1]) or (sc[k] == sc[k + 1] and flat[k] < flat[k + 1]) for k in range(W - 1))
        if vocab is not None:
            t2, p2, w2, s2 = BM.beam_step(l[:, first:first + count], s)
            assert np.array_equal(tok, t2 + first) and np.array_equal(par, p2) and np.array_equal(wt, w2)
            assert np.array_equal(sc.view(np.uint32), s2.view(np.uint32))


def test_more_beams_than_tokens_raises():
    l = rows_bf16(0, 5, 260)
    with pytest.raises(ValueError):
        BM.beam_step(l, np.zeros(5, F32), vocab=(0, 4))
    with pytest.raises(ValueError):
        BM.beam_step(rows_bf16(0, 3, 2), np.zeros(3, F32))
    with pytest.raises(ValueError):
        BM.beam_step(rows_bf16(0, 17, 260), np.zeros(17, F32))
    with pytest.raises(ValueError):
        BM.beam_step(l, np.zeros(5, F32), vocab=(250, 20))


# ---- beam_search ---------------------------------------------------------------------------------------------------------
class Table:
    """A stand-in model: a seeded lookup from the prefix to a bf16-rounded logits row over `count` live tokens, padded
    with -inf columns to `cols` (dead tokens: weight 0, score -inf)."""

    def __init__(self, seed: int, count: int, cols: int = 0, scale: float = 2.0):
        self.seed, self.count, self.cols, self.scale, self.rows = seed, count, max(cols, count), scale, {}

    def row(self, prefix) -> np.ndarray:
        key = tuple(int(t) for t in prefix)
        if key not in self.rows:
            r = np.full(self.cols, -np.inf, dtype=F32)
            r[:self.count] = bf16(np.random.default_rng([self.seed, len(key), *key]).standard_normal(self.count) * self.scale)
            self.rows[key] = r
        return self.rows[key]

    def __call__(self, prefixes) -> np.ndarray:
        return np.stack([self.row(p) for p in prefixes])

    def logp64(self, prefix) -> np.ndarray:
        r = self.row(prefix)[:self.count].astype(np.float64)
        return r - r.max() - np.log(np.exp(r - r.max()).sum())


def reference_beams(table: Table, W: int, n: int):
    """A straightforward fp64 beam search (log_softmax, sort) → (sequences, scores, the smallest gap it ever decided
    by: last kept vs first dropped at every step, and between the returned neighbours at the end)."""
    beams, gap = [((), 0.0)], np.inf
    for _ in range(n):
        cand = sorted(((s + lp, p + (i,)) for p, s in beams for i, lp in enumerate(table.logp64(p))), key=lambda c: -c[0])
        if len(cand) > W:
            gap = min(gap, cand[W - 1][0] - cand[W][0])
        beams = [(p, s) for s, p in cand[:W]]
    scores = np.array([s for _, s in beams])
    return np.array([p for p, _ in beams]), scores, min(gap, -np.diff(scores).max())


def test_beam_search_wide_enough_is_exact():
    """count = 4 live tokens, n = 3 and W = 16 = 4²: no live prefix is ever dropped before the last step, so the result is the
    global top 16 of all 64 sequences by joint probability, in order. (The rows are padded to 16 columns with -inf so that
    W <= the column count the module requires; the dead columns never outrank a live one.)"""
    table = Table(seed=5, count=4, cols=16)
    seq, wt, scores = BM.beam_search(table, 16, 3)
    every = sorted(((sum(table.logp64(p[:t])[p[t]] for t in range(3)), p) for p in itertools.product(range(4), repeat=3)),
                   key=lambda c: -c[0])
    joint = np.array([s for s, _ in every])
    assert -np.diff(joint[:17]).max() >= 1e-3, "the table must separate its top 17 sequences"
    assert seq.tolist() == [list(p) for _, p in every[:16]] and seq[0].tolist() == list(every[0][1])
    assert np.abs(scores - joint[:16]).max() < 5e-5
    assert np.abs(S.logprob(wt).sum(axis=1) - joint[:16]).max() < 1e-5           # the pairs are the per-token probabilities


@pytest.mark.parametrize("W", [2, 5])
@pytest.mark.parametrize("count,seed", [(8, 1), (8, 2), (256, 1), (256, 2)])
def test_beam_search_against_the_straightforward_reference(W, count, seed):
    """Seven steps. Where the fp64 reference decides every cut and the final order by >= 1e-3 (asserted for every table),
    the fp32 specification must agree: per step it rounds three sums at |score| < 64 (<= 3 · 2^-19 = 5.7e-6), log_spec adds
    <= 7.1e-7 and the integer weights <= 3e-7 relative of the denominator — below 5e-5 after seven steps."""
    n = 7
    table = Table(seed=100 * count + seed, count=count)
    want, want_scores, gap = reference_beams(table, W, n)
    assert gap >= 1e-3, f"table (count {count}, seed {seed}, W {W}) decides by {gap:.2e}: build it so that the gap holds"
    seq, wt, scores = BM.beam_search(table, W, n)
    assert np.array_equal(seq, want) and np.all(np.abs(want_scores) < 64)
    assert np.abs(scores - want_scores).max() < 5e-5
    assert np.abs(S.logprob(wt).sum(axis=1) - want_scores).max() < 1e-5


def test_backtrack_hand_made_tree():
    # step 0: slots a b c (all from the start beam). step 1: slot 0 <- a, slot 1 <- a (two children), slot 2 <- c; b is dead.
    # step 2: slot 0 <- old slot 2, slot 1 <- old slot 0, slot 2 <- old slot 0.
    tokens = np.array([[10, 11, 12], [20, 21, 22], [30, 31, 32]])
    parents = np.array([[0, 0, 0], [0, 0, 2], [2, 0, 0]], dtype=np.int32)
    wt = np.stack([tokens * 2, tokens * 3], axis=-1)
    seq, pairs = BM.backtrack(tokens, parents, wt)
    assert seq.tolist() == [[12, 22, 30], [10, 20, 31], [10, 20, 32]] and 11 not in seq and 21 not in seq
    assert np.array_equal(pairs[..., 0], seq * 2) and np.array_equal(pairs[..., 1], seq * 3)
    assert seq.dtype == np.int64 and pairs.shape == (3, 3, 2)


# ---- argument checks that need no device ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from bridgelang_amd import weights as Wt
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"d": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    m = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device="cpu", dims=Wt.tiny_dims())

    def no_engine(*a, **k):
        raise AssertionError("an argument error must be raised before an engine is asked for")
    m.engine = no_engine
    return m


def test_surface_refuses_what_beams_do_not_combine_with(model):
    ids, pv = torch.ones(2, 6, dtype=torch.int64), torch.zeros(2, 6, 224, 224)
    gen = lambda **kw: model.generate(ids, 7, pixel_values=pv, **kw)
    for bad in (0, -1, 17, 2.5, True, "4"):
        with pytest.raises(ValueError, match="num_beams"):
            gen(num_beams=bad)
    with pytest.raises(ValueError, match="num_beams"):
        gen(num_beams=8, vocab_range=(31744, 4))                                 # more beams than the policy has tokens
    for W, R in ((4, 5), (4, 0), (1, 2), (3, 1.5)):
        with pytest.raises(ValueError, match="num_return_sequences"):
            gen(num_beams=W, num_return_sequences=R)
    for kw in (dict(sampling=S.SamplingParams(seed=0)), dict(do_sample=True), dict(forced_ids=torch.zeros(2, 7, dtype=torch.int64)),
               dict(return_attention="segments"), dict(return_values="token")):
        with pytest.raises(ValueError, match="num_beams=4"):
            gen(num_beams=4, **kw)
        with pytest.raises(ValueError):
            model.predict_action(ids, "d", pixel_values=pv, num_beams=4, **kw)
    with pytest.raises(ValueError, match="pixel_values"):
        model.generate(ids, 7, num_beams=4)
    with pytest.raises(ValueError, match="token"):
        model.beam_actions(ids, pv, "d", num_beams=4, return_values="token")
    with pytest.raises(ValueError, match="num_beams"):
        model.beam_actions(ids, pv, "d", num_beams=17)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.beam_actions(ids, pv, "d", num_beams=4, num_return_sequences=5)
    with pytest.raises(ValueError, match="unnorm_keys"):
        model.beam_actions(ids, pv, ["d"], num_beams=4)
    with pytest.raises(AssertionError, match="before an engine"):               # a valid call does reach the engine
        gen(num_beams=4, num_return_sequences=2, length_penalty=2.0, early_stopping=True)


def test_engine_refuses_what_beams_do_not_combine_with():
    from bridgelang_amd import weights as Wt
    from bridgelang_amd.attention_taps import AttnTaps
    from bridgelang_amd.engine import BeamTrace, OpenVLAEngine
    w = Wt.allocate(Wt.tiny_dims(), "cpu")
    for kw, word in ((dict(sample=True), "sample"), (dict(score=True), "score"), (dict(all_rows=True), "generation plan"),
                     (dict(attn_taps=AttnTaps(layers=None, full=True, segments=False)), "attn_taps"),
                     (dict(value="token"), "token")):
        with pytest.raises(ValueError, match=word):
            OpenVLAEngine(w, 4, 8, beams=4, **kw)
    for beams in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="beams"):
            OpenVLAEngine(w, 16, 8, beams=beams)
    with pytest.raises(ValueError, match="multiple"):
        OpenVLAEngine(w, 6, 8, beams=4)
    with pytest.raises(ValueError, match="exceeds"):
        OpenVLAEngine(w, 8, 8, beams=8, vocab_range=(31744, 4))
    with pytest.raises(ValueError, match="vocab_range"):                         # still refused on the plain greedy plan
        OpenVLAEngine(w, 4, 8, vocab_range=(31744, 256))
    assert BeamTrace._fields == ("tokens", "parents", "wt", "scores")
