"""bl_score_f32 and everything built on it, held to the specification bridgelang_amd/sampling.py::score_rows BIT FOR BIT:
the kernel on the planted rows, forced tokens and ranges of tests/test_scoring_cpu.py; the sampler it shares its code with
(unchanged); the score=True engine against the sample=True engine whose draws it scores (eager, captured, right-padded,
batch-invariant); the staggered pipeline against the engine; and the model surface (`score_actions`, `generate(forced_ids=)`)."""
import functools

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from test_sampling_gpu import B, L, _ctx, _params
from test_scoring_cpu import V, assert_hard_classes_present, forced_tokens, hard_classes, planted_rows, wave_span

pytestmark = pytest.mark.gpu

STEP = 3
ACTION_RANGE = (31744, 256)             # the action tokens [vocab_size - n_action_bins, vocab_size) of the 32 000-token tokenizer


# ---- kernel against specification ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(rows, n):
    """Rows, forced tokens and the specification's answers (over the FULL range: every range is a slice of it), once."""
    l, T, k, p, seeds = planted_rows(rows, n, seed=rows + n)
    tok = forced_tokens(l, T, k, p, seeds, STEP)
    wt, full = S.score_rows(l, T, k, p, tok, 0, n)
    for a in (l, T, k, p, seeds, tok, wt, full):
        a.setflags(write=False)
    return l, T, k, p, seeds, tok, wt, full


def _device_rows(l, dev):
    """ld = n + 12 with +inf in the padding columns, which must not be read."""
    rows, n = l.shape
    buf = torch.full((rows, n + 12), float("inf"), dtype=torch.float32)
    buf[:, :n] = torch.from_numpy(l.copy())
    return buf.to(dev)[:, :n]


def _ranges(n):
    span = wave_span(n)
    out = [None, (span - 3, 8), (n - 1, 1)]                           # none; straddling the first wave-span boundary; one element
    if n == V:
        out.append(ACTION_RANGE)
    if n == 260:
        out.append((0, n))
    return out


@pytest.mark.parametrize("rows,n", [(256, V), (64, 260), (1, V), (5, 260)])
def test_kernel_equals_specification(dev, rows, n):
    from bridgelang_amd import ops
    l, T, k, p, seeds, tok, want_wt, full = _case(rows, n)
    if rows >= 64:                                                    # the shapes with rows enough to hold every class
        assert_hard_classes_present(hard_classes(l, T, k, p, tok))
    d = lambda a: torch.from_numpy(a.copy()).to(dev)
    logits, dT, dk, dp, dtok = _device_rows(l, dev), d(T), d(k), d(p), d(tok)
    guard = 64
    for rng in _ranges(n):
        wt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
        if rng is None:
            ops.score(logits, dT, dk, dp, dtok, wt)
        else:
            first, count = rng
            flat = torch.full((rows * count + 2 * guard,), -1, dtype=torch.int32, device=dev)
            ops.score(logits, dT, dk, dp, dtok, wt, first, flat[guard:guard + rows * count].view(rows, count))
            got = flat.cpu().numpy()
            assert (got[:guard] == -1).all() and (got[-guard:] == -1).all(), f"range {rng}: wrote outside [rows, count]"
            got = got[guard:-guard].reshape(rows, count)
            bad = np.flatnonzero((got != full[:, first:first + count]).any(axis=1))
            assert bad.size == 0, (rng, [(int(r), float(T[r]), int(k[r]), float(p[r])) for r in bad[:8]])
        got_wt = wt.cpu().numpy()
        bad = np.flatnonzero((got_wt != want_wt).any(axis=1))
        assert bad.size == 0, (rng, [(int(r), float(T[r]), int(k[r]), float(p[r]), int(tok[r]), got_wt[r].tolist(), want_wt[r].tolist())
                                     for r in bad[:8]])


def test_sampler_unchanged_beside_the_scorer(dev):
    """bl_sample_f32 shares stages 1–4 with the scorer: its ids and wt on the same buffers, before and after a scoring
    launch, are the specification's."""
    from bridgelang_amd import ops
    rows, n = 64, 260
    l, T, k, p, seeds, tok, want_wt, full = _case(rows, n)
    want_ids, want_swt = S.sample_rows(l, T, k, p, seeds, STEP)
    d = lambda a: torch.from_numpy(a.copy()).to(dev)
    logits, dT, dk, dp, dseed, dtok = _device_rows(l, dev), d(T), d(k), d(p), d(seeds), d(tok)
    runs = []
    for _ in range(2):
        ids = torch.full((rows,), -1, dtype=torch.int64, device=dev)
        swt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
        ops.sample(logits, dT, dk, dp, dseed, STEP, ids, swt)
        runs.append((ids.cpu().numpy(), swt.cpu().numpy()))
        wt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
        rw = torch.full((rows, n), -1, dtype=torch.int32, device=dev)
        ops.score(logits, dT, dk, dp, dtok, wt, 0, rw)
        assert np.array_equal(wt.cpu().numpy(), want_wt) and np.array_equal(rw.cpu().numpy(), full)
        # scoring the sampler's own draws gives the sampler's pairs
        ops.score(logits, dT, dk, dp, ids, wt)
        assert torch.equal(wt, swt)
    for got_ids, got_swt in runs:
        assert np.array_equal(got_ids, want_ids) and np.array_equal(got_swt, want_swt)


def test_kernel_rejects_what_it_cannot_hold(dev):
    from bridgelang_amd import ops
    from bridgelang_amd._lib import BridgeLangHipError
    z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=dev)

    def run(n, first=0, count=0):
        rw = z(torch.int32, 2, count) if count else None
        ops.score(z(torch.float32, 2, n), z(torch.float32, 2), z(torch.int32, 2), z(torch.float32, 2), z(torch.int64, 2),
                  z(torch.int64, 2, 2), first, rw)
    for kw in (dict(n=36484), dict(n=262), dict(n=260, first=257, count=4), dict(n=260, first=-1, count=4)):
        with pytest.raises(BridgeLangHipError, match="BL_E_SHAPE"):
            run(**kw)
    f = z(torch.float32, 2)
    good = dict(logits=z(torch.float32, 2, 8), temperature=f, top_k=z(torch.int32, 2), top_p=f, tokens=z(torch.int64, 2),
                wt=z(torch.int64, 2, 2))
    for name, wrong in (("tokens", z(torch.int32, 2)), ("top_k", z(torch.int64, 2)), ("wt", z(torch.int32, 2, 2)),
                        ("logits", z(torch.bfloat16, 2, 8)), ("range_wt", z(torch.int64, 2, 4)), ("range_wt", z(torch.int32, 3, 4))):
        with pytest.raises(TypeError):
            ops.score(**{**good, name: wrong})
    run(260, 256, 4)                                                  # the last four tokens: inside


# ---- tiny-model engine -----------------------------------------------------------------------------------------------------
def _check_against_spec(eng, params, tag):
    """The run's own logits and forced tokens through the specification, step by step."""
    T, k, p, _ = params.resolve(eng.B)
    logits, tok = eng.logits.cpu().numpy(), eng.gen_ids.cpu().numpy()
    wt = eng.gen_wt.cpu().numpy()
    first, count = eng.score_range if eng.score_range is not None else (0, 0)
    for t in range(eng.n_new):
        want_wt, want_rw = S.score_rows(logits[t], T, k, p, tok[t], first, count)
        assert np.array_equal(wt[t], want_wt), f"{tag}: step {t}"
        if count:
            assert np.array_equal(eng.gen_range_wt[t].cpu().numpy(), want_rw), f"{tag}: range weights of step {t}"


def test_engine_scores_what_the_sampling_engine_drew(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    ids, pv = c["make_inputs"](c["dims"], B, L, seed=21)
    ids, pv = ids.to(dev), pv.to(dev)
    samp = OpenVLAEngine(c["w"], B, L, sample=True)
    eng = OpenVLAEngine(c["w"], B, L, score=True, score_range=ACTION_RANGE)
    one = OpenVLAEngine(c["w"], 1, L, score=True, score_range=ACTION_RANGE)
    greedy = OpenVLAEngine(c["w"], B, L)
    forced_sets = []
    for salt, captured in ((1, False), (2, True), (3, True)):         # one graph, two different sets of forced ids
        if captured and eng._graph is None:
            eng.capture()
        params = _params(B, salt)
        forced = samp.generate(ids, pv, params).clone()
        wt, rw = eng.score(ids, pv, forced, params)
        torch.cuda.synchronize()
        tag = f"captured={captured} salt={salt}"
        assert torch.equal(eng.gen_wt, samp.gen_wt) and torch.equal(wt, samp.gen_wt.permute(1, 0, 2)), tag
        assert torch.equal(eng.logits, samp.logits) and torch.equal(eng.gen_ids, samp.gen_ids), tag
        assert tuple(rw.shape) == (B, eng.n_new, ACTION_RANGE[1])
        _check_against_spec(eng, params, tag)
        forced_sets.append(forced.cpu())
        T, k, p, _ = params.resolve(B)
        for b in range(B):                                            # the project's batch-invariance rule
            pb = S.SamplingParams(float(T[b]), int(k[b]), float(p[b]))
            wt1, rw1 = one.score(ids[b:b + 1], pv[b:b + 1], forced[b:b + 1], pb)
            assert torch.equal(wt1[0], wt[b]) and torch.equal(rw1[0], rw[b]), f"{tag}: sequence {b} differs from its batch-1 run"
    assert not torch.equal(forced_sets[1], forced_sets[2])
    # forced ids that leave the draw at step 2: the steps up to it see the same logits, the later ones other logits
    params = _params(B, 3)
    other = forced.clone()
    other[:, 2] = torch.where(other[:, 2] > ACTION_RANGE[0], other[:, 2] - 1, other[:, 2] + 1)
    eng.score(ids, pv, other, params)
    torch.cuda.synchronize()
    assert torch.equal(eng.logits[:3], samp.logits[:3])
    for t in range(3, eng.n_new):
        assert not torch.equal(eng.logits[t], samp.logits[t]), f"step {t} did not see the forced token of step 2"
    _check_against_spec(eng, params, "forced ids off the draw")
    assert torch.equal(eng.gen_ids.t(), other)                        # nothing writes the forced ids
    # the score plan is the greedy plan with every argmax replaced by the score
    assert [o.name.replace("bl_argmax_f32", "bl_score_f32") for o in greedy.all_ops()] == [o.name for o in eng.all_ops()]
    assert sum(o.name == "bl_score_f32" for o in eng.all_ops()) == eng.n_new
    for bad in (dict(sample=True, score=True), dict(score=True, all_rows=True), dict(score=True, vision_only=True),
                dict(score_range=ACTION_RANGE), dict(score=True, score_range=(32000, 100))):
        with pytest.raises(ValueError):
            OpenVLAEngine(c["w"], B, L, **bad)
    with pytest.raises(ValueError):
        greedy.set_forced_ids(forced)
    with pytest.raises(ValueError):
        eng.set_forced_ids(torch.full_like(forced, c["dims"].vocab))
    with pytest.raises(ValueError):
        eng.set_forced_ids(forced[:, :3])


def test_engine_scoring_right_padded(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    ids, pv = c["make_inputs"](c["dims"], B, L, seed=22)
    lens = [L, 4, 8]
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, n - 1] = 29871
        ids[b, n:] = 32000
        mask[b, :n] = 1
    ids, pv, mask = ids.to(dev), pv.to(dev), mask.to(dev)
    params = _params(B, 4)
    samp = OpenVLAEngine(c["w"], B, L, padded=True, sample=True)
    samp.set_sampling(params)
    samp.set_padded_inputs(ids, pv, mask)
    samp.run_eager()
    forced = samp.gen_ids.t().clone()
    eng = OpenVLAEngine(c["w"], B, L, padded=True, score=True, score_range=ACTION_RANGE)
    eng.set_sampling(params)
    eng.set_forced_ids(forced)
    eng.set_padded_inputs(ids, pv, mask)
    eng.run_eager()
    assert torch.equal(eng.gen_wt, samp.gen_wt) and torch.equal(eng.logits, samp.logits)
    _check_against_spec(eng, params, "padded")
    T, k, p, _ = params.resolve(B)
    for b, n in enumerate(lens):
        one = OpenVLAEngine(c["w"], 1, n, score=True, score_range=ACTION_RANGE)
        wt1, rw1 = one.score(ids[b:b + 1, :n], pv[b:b + 1], forced[b:b + 1], S.SamplingParams(float(T[b]), int(k[b]), float(p[b])))
        assert torch.equal(wt1[0], eng.gen_wt[:, b]) and torch.equal(rw1[0], eng.gen_range_wt[:, b]), \
            f"padded sequence {b} (length {n}) differs from its un-padded batch-1 score"


# ---- pipeline --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_pipeline_equals_engine(dev, padded):
    """Every submitted batch comes out with the wt and range weights of OpenVLAEngine(score=True) on that batch — which are
    the sampling engine's pairs, the forced ids being its draws — through the captured slot rotations and the drain."""
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    c = _ctx(dev)
    PB, PL, N = 2, 12, 10
    g = torch.Generator().manual_seed(78)
    samp = OpenVLAEngine(c["w"], PB, PL, padded=padded, sample=True)
    eng = OpenVLAEngine(c["w"], PB, PL, padded=padded, score=True, score_range=ACTION_RANGE)
    batches, want = [], []
    for s in range(N):
        ids, pv = c["make_inputs"](c["dims"], PB, PL, seed=80 + s)
        mask = torch.ones(PB, PL, dtype=torch.long)
        if padded and s != 0:
            for b, n in enumerate(torch.randint(2, PL + 1, (PB,), generator=g).tolist()):
                ids[b, n - 1] = 29871
                ids[b, n:] = 32000
                mask[b, n:] = 0
        ids, pv, mask, sp = ids.to(dev), pv.to(dev), mask.to(dev), _params(PB, 30 + s)
        forced = None
        for e in (samp, eng):                                         # the sampling engine draws, the score engine scores its draws
            e.set_sampling(sp)
            if forced is not None:
                e.set_forced_ids(forced)
            e.set_padded_inputs(ids, pv, mask) if padded else e.set_inputs(ids, pv)
            e.run_eager()
            forced = samp.gen_ids.t().clone()
        assert torch.equal(eng.gen_wt, samp.gen_wt)
        batches.append((ids, pv, mask, sp, forced))
        want.append((eng.gen_wt.permute(1, 0, 2).clone().cpu(), eng.gen_range_wt.permute(1, 0, 2).clone().cpu()))

    pipe = StaggeredDecodePipeline(c["w"], PB, PL, padded=padded, score=True, score_range=ACTION_RANGE)
    ids, pv, mask, _, _ = batches[0]
    for e in pipe.engines:
        e.set_padded_inputs(ids, pv, mask) if padded else e.set_inputs(ids, pv)
    pipe.capture()
    got = []
    for s, (ids, pv, mask, sp, forced) in enumerate(batches):
        out = pipe.step(ids, pv, mask, sampling=sp, forced_ids=forced) if padded else pipe.step(ids, pv, sampling=sp, forced_ids=forced)
        if s >= pipe.slots - 1:
            got.append(tuple(o.clone().cpu() for o in out))
    got += [tuple(o.cpu() for o in x) for x in pipe.flush()]
    assert len(got) == N
    for s in range(N):
        assert torch.equal(got[s][0], want[s][0]), f"batch {s}: weight pairs differ from the engine's"
        assert torch.equal(got[s][1], want[s][1]), f"batch {s}: range weights differ from the engine's"
    if not padded:
        with pytest.raises(ValueError):
            pipe.step(ids, pv, sampling=sp)                            # a score pipeline's batch needs its forced ids
        with pytest.raises(ValueError):
            StaggeredDecodePipeline(c["w"], PB, PL).step(ids, pv, forced_ids=forced)


# ---- surface ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=W.tiny_dims()).init_synthetic(seed=11)


def test_score_actions_surface(model, dev):
    from test_engine_gpu import make_inputs
    ids, pv = make_inputs(model.dims, 2, 10, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    sp = S.SamplingParams(temperature=[1.0, 2.0], top_k=[50, 0], top_p=[0.95, 1.0], seed=[123, -9])
    actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=4)
    got = model.score_actions(ids, pv, token_ids=tokens, sampling=sp)
    assert got.shape == (2, 4, 7) and got.dtype == np.float64 and np.array_equal(got, lp)
    n_bins, first = model.config.n_action_bins, model.vocab_size - model.config.n_action_bins
    # actions= is token_ids= of their tokens (candidates moved into the decodable range, where the encoding is a bijection)
    cand = np.clip(tokens, model.vocab_size - 255, model.vocab_size - 1)
    acts = model.actions_from_token_ids(cand, "bridge_orig")
    assert np.array_equal(model.token_ids_from_actions(acts, "bridge_orig"), cand)
    assert np.array_equal(model.score_actions(ids, pv, actions=acts, unnorm_key="bridge_orig", sampling=sp),
                          model.score_actions(ids, pv, token_ids=cand, sampling=sp))
    # K = 1 and [B, n]
    a = model.score_actions(ids, pv, token_ids=tokens[:, 2], sampling=sp)
    assert a.shape == (2, 1, 7) and np.array_equal(a, lp[:, 2:3])
    assert np.array_equal(model.score_actions(ids, pv, token_ids=torch.from_numpy(tokens[:, 2:3]), sampling=sp), a)
    # a candidate outside top-k: -inf at that step, finite before it; the later steps are conditioned on it
    kp = S.SamplingParams(temperature=1.0, top_k=4)
    full = model.with_empty_token(ids)
    base = model.generate(full, 7, pixel_values=pv)[:, -7:].cpu().numpy()              # the greedy tokens: inside any top-k
    lg, wt, bins = model.score_actions(ids, pv, token_ids=base, sampling=kp, return_bins=True)
    assert np.all(np.isfinite(lg))
    out, step = base.copy(), 3
    for b in range(2):
        out[b, step] = first + np.flatnonzero(bins[b, 0, step] == 0)[0]               # an action token top-k removed at that step
    lo = model.score_actions(ids, pv, token_ids=out, sampling=kp)
    assert np.all(lo[:, 0, step] == -np.inf) and np.array_equal(lo[:, 0, :step], lg[:, 0, :step])
    # return_bins: the weight pairs, and the kept weight of every action token
    lp2, wt, bins = model.score_actions(ids, pv, token_ids=tokens, sampling=sp, return_bins=True)
    assert np.array_equal(lp2, lp) and np.array_equal(S.logprob(wt), lp)
    assert wt.shape == (2, 4, 7, 2) and wt.dtype == np.int64 and bins.shape == (2, 4, 7, n_bins) and bins.dtype == np.int32
    assert np.all(bins.astype(np.int64).sum(-1) <= wt[..., 1]) and np.all(bins >= 0)
    _, cwt, cbins = model.score_actions(ids, pv, token_ids=cand, sampling=sp, return_bins=True)     # action tokens, all of them
    assert np.array_equal(np.take_along_axis(cbins, (cand - first)[..., None], axis=-1)[..., 0], cwt[..., 0])
    for b_, w_ in ((bins, wt), (cbins, cwt)):
        ent, mass = S.range_entropy(b_, w_[..., 1])
        assert np.all(np.isfinite(ent)) and np.all(ent >= 0) and np.all(np.isfinite(mass)) and np.all(mass >= 0)
    # generate(forced_ids=): prompt ‖ forced ids, and the pairs
    forced = torch.from_numpy(tokens[:, 0].copy()).to(dev)
    seq, gwt = model.generate(full, 7, pixel_values=pv, sampling=sp, forced_ids=forced)
    assert torch.equal(seq, torch.cat([full, forced], dim=1)) and np.array_equal(gwt.cpu().numpy(), wt[:, 0])
    # a right-padded batch equals the un-padded calls
    short = torch.cat([ids[1:, :5], torch.full((1, ids.shape[1] - 5), 32000, device=dev)], dim=1)
    both = torch.cat([ids[:1], short], dim=0)
    mask = torch.ones_like(both)
    mask[1, 5:] = 0
    cand = tokens[:, :2]
    padded = model.score_actions(both, pv, token_ids=cand, sampling=sp, attention_mask=mask)
    alone0 = model.score_actions(ids[:1], pv[:1], token_ids=cand[:1], sampling=S.SamplingParams(1.0, 50, 0.95))
    alone1 = model.score_actions(short[:, :5], pv[1:], token_ids=cand[1:], sampling=S.SamplingParams(2.0, 0, 1.0))
    assert np.array_equal(padded[0], alone0[0]) and np.array_equal(padded[1], alone1[0])
    for kw in (dict(), dict(token_ids=tokens, actions=actions)):
        with pytest.raises(ValueError):
            model.score_actions(ids, pv, sampling=sp, **kw)
    with pytest.raises(ValueError):
        model.score_actions(ids, pv, token_ids=np.full((2, 7), model.dims.vocab))
