"""Beam search over the action tokens on the device, held to bridgelang_amd/beam.py BIT FOR BIT: bl_beam_step_f32 on planted
rows (tokens, parents, both integers of wt, scores), bl_beam_reorder_kv_bf16 against a host gather, the beams= engine step by
step against the specification (eager, captured, right-padded, batch-invariant), its KV caches proven through a score=True
engine, and the model surface (`generate(num_beams=)`, `predict_action(num_beams=)`, `beam_actions`)."""
import functools

import numpy as np
import pytest
import torch

from bridgelang_amd import beam as BM
from bridgelang_amd import sampling as S
from test_sampling_gpu import L, _ctx

pytestmark = pytest.mark.gpu

V = 32064
ACTION_RANGE = (31744, 256)
GUARD = 64


# ---- bl_beam_step_f32 against the specification ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(groups, W, n, vocab):
    """bf16-rounded rows with planted duplicates, scores of a previous step with -inf entries, and the specification's
    answers, once."""
    rng = np.random.default_rng(1000 * groups + 10 * W + n % 7)
    rows = groups * W
    l = torch.from_numpy((rng.standard_normal((rows, n)) * 3).astype(np.float32)).to(torch.bfloat16).float().numpy()
    s = (-np.abs(rng.standard_normal(rows)) * 4).astype(np.float32)
    first, count = vocab if vocab is not None else (0, n)
    for g in range(groups):
        r0 = g * W
        cols = first + (np.arange(4) * 61 + 7 * g) % count
        l[r0, cols] = l[r0, first:first + count].max()                        # ties at the top inside a row
        if W >= 2:                                                               # beam 1 = beam 0, logits and score: ties across beams
            l[r0 + 1], s[r0 + 1] = l[r0], s[r0]
        if W >= 4:
            s[r0 + 3] = -np.inf                                                  # a dead beam
        if W >= 5:
            l[r0 + 4] = np.round(l[r0 + 4])                                      # coarse logits: many equal candidates
    if groups == 3:
        s[2 * W:] = BM.start_scores(W)                                           # the last prompt is at step 0
        l[2 * W:] = l[2 * W]
    want = [BM.beam_step(l[g * W:(g + 1) * W], s[g * W:(g + 1) * W], vocab) for g in range(groups)]
    tok, par, wt, sc = (np.concatenate([w[i] for w in want]) for i in range(4))
    for a in (l, s, tok, par, wt, sc):
        a.setflags(write=False)
    return l, s, tok, par, wt, sc


def _device_rows(l, dev):
    """ld = n + 12 with +inf in the padding columns, which must not be read."""
    rows, n = l.shape
    buf = torch.full((rows, n + 12), float("inf"), dtype=torch.float32)
    buf[:, :n] = torch.from_numpy(l.copy())
    return buf.to(dev)[:, :n]


def _guarded(rows, tail, dtype, fill, dev):
    size = rows * int(np.prod(tail, dtype=np.int64))
    flat = torch.full((size + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return flat, flat[GUARD:GUARD + size].view((rows,) + tail)


@pytest.mark.parametrize("groups,W,n,vocab", [(1, 1, 260, None), (3, 2, 260, None), (2, 5, 260, None), (1, 16, 260, None),
                                              (2, 4, V, ACTION_RANGE), (1, 16, V, None)])
def test_beam_step_kernel_equals_specification(dev, groups, W, n, vocab):
    from bridgelang_amd import ops
    l, s, want_tok, want_par, want_wt, want_sc = _case(groups, W, n, vocab)
    rows = groups * W
    assert np.isinf(s).any() or W < 4
    logits, s_in = _device_rows(l, dev), torch.from_numpy(s.copy()).to(dev)
    tok_f, tok = _guarded(rows, (), torch.int64, -7, dev)
    par_f, par = _guarded(rows, (), torch.int32, -7, dev)
    wt_f, wt = _guarded(rows, (2,), torch.int64, -7, dev)
    sc_f, sc = _guarded(rows, (), torch.float32, 123.0, dev)
    ops.beam_step(logits, W, s_in, tok, par, wt, sc, vocab=vocab)
    torch.cuda.synchronize()
    for flat, fill in ((tok_f, -7), (par_f, -7), (wt_f, -7), (sc_f, 123.0)):
        assert bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all()), "wrote outside its outputs"
    got_par, got_tok = par.cpu().numpy(), tok.cpu().numpy()
    first, count = vocab if vocab is not None else (0, n)
    assert ((got_par >= 0) & (got_par < W)).all() and ((got_tok >= first) & (got_tok < first + count)).all()
    assert np.array_equal(got_par, want_par) and np.array_equal(got_tok, want_tok), (got_par, want_par, got_tok, want_tok)
    assert np.array_equal(wt.cpu().numpy(), want_wt)
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_sc.view(np.uint32)), (sc.cpu().numpy(), want_sc)
    assert torch.equal(s_in.cpu(), torch.from_numpy(s.copy()))


def test_beam_step_kernel_rejects_what_it_cannot_hold(dev):
    from bridgelang_amd import ops
    from bridgelang_amd._lib import BridgeLangHipError

    def run(rows, W, n, vocab=None, ok=False):
        out = (torch.full((rows,), -7, dtype=torch.int64, device=dev), torch.full((rows,), -7, dtype=torch.int32, device=dev),
               torch.full((rows, 2), -7, dtype=torch.int64, device=dev), torch.full((rows,), 123.0, dtype=torch.float32, device=dev))
        call = lambda: ops.beam_step(torch.zeros(rows, n, device=dev), W, torch.zeros(rows, device=dev), *out, vocab=vocab)
        if ok:
            call()
            torch.cuda.synchronize()
            assert all(bool((o != f).all()) for o, f in zip(out, (-7, -7, -7, 123.0)))
            return
        with pytest.raises(BridgeLangHipError, match="BL_E_SHAPE"):
            call()
        torch.cuda.synchronize()
        assert all(bool((o == f).all()) for o, f in zip(out, (-7, -7, -7, 123.0))), "a rejected call launched something"
    run(17, 17, 260)                                                             # more beams than a workgroup ranks
    run(8, 8, 260, (0, 4))                                                       # more beams than tokens
    run(2, 2, 36484)                                                             # beyond the sampler's row limit
    run(2, 2, 262)                                                               # n % 4
    run(2, 2, 260, (257, 8))                                                     # the range leaves the row
    run(2, 2, 260, (2, 8))                                                       # a range off the 16-byte grid
    run(2, 2, 260, (256, 4), ok=True)                                            # the last four tokens: inside
    with pytest.raises(ValueError):
        ops.beam_step(torch.zeros(6, 260, device=dev), 4, torch.zeros(6, device=dev), torch.zeros(6, dtype=torch.int64, device=dev),
                      torch.zeros(6, dtype=torch.int32, device=dev), torch.zeros(6, 2, dtype=torch.int64, device=dev),
                      torch.zeros(6, device=dev))
    with pytest.raises(TypeError):
        ops.beam_step(torch.zeros(4, 260, device=dev), 4, torch.zeros(4, device=dev), torch.zeros(4, dtype=torch.int64, device=dev),
                      torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, 2, dtype=torch.int64, device=dev),
                      torch.zeros(4, device=dev))


# ---- bl_beam_reorder_kv_bf16 against a host gather ---------------------------------------------------------------------------
PARENTS = {"identity": [0, 1, 2, 3], "permutation": [2, 0, 3, 1], "all-from-one": [2, 2, 2, 2],
           "two-children-own-slot-overwritten": [1, 0, 0, 3]}      # slot 0 feeds slots 1 and 2 and is itself overwritten by slot 1


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("n_rows", [1, 6])
@pytest.mark.parametrize("per_row", [False, True])
def test_reorder_kernel_equals_host_gather(dev, H, n_rows, per_row):
    from bridgelang_amd import ops
    W, hd, cache_len = 4, 128, 64
    names = list(PARENTS)
    groups = len(names)
    rows = groups * W
    g = torch.Generator().manual_seed(100 * H + 10 * n_rows + per_row)
    caches = [torch.randn(rows, H, cache_len, hd, generator=g).to(torch.bfloat16).to(dev) for _ in range(4)]      # K, V of 2 layers
    before = [c.cpu().clone() for c in caches]
    parents = torch.tensor([p for name in names for p in PARENTS[name]], dtype=torch.int32)
    starts = [17, 5, 64 - n_rows, 30] if per_row else [23] * groups              # a prompt's rows share their start
    row0 = torch.tensor([s for s in starts for _ in range(W)], dtype=torch.int32)
    ops.beam_reorder_kv(ops.cache_table(caches), caches, W, parents.to(dev), row0.to(dev) if per_row else starts[0], n_rows)
    torch.cuda.synchronize()
    for c, b in zip(caches, before):
        want = b.clone()
        for e in range(groups):
            for k in range(W):
                src = e * W + int(parents[e * W + k])
                want[e * W + k, :, starts[e]:starts[e] + n_rows] = b[src, :, starts[e]:starts[e] + n_rows]
        got = c.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "moved rows differ from the gather, or bytes outside them changed"
    assert not torch.equal(caches[0].cpu().view(torch.int16), before[0].view(torch.int16))


def test_reorder_kernel_rejects_what_it_cannot_hold(dev):
    from bridgelang_amd import ops
    from bridgelang_amd._lib import BridgeLangHipError
    caches = [torch.zeros(8, 2, 64, 128, dtype=torch.bfloat16, device=dev)]
    table, par = ops.cache_table(caches), torch.zeros(8, dtype=torch.int32, device=dev)
    for W, row0, n_rows in ((3, 0, 1), (17, 0, 1), (4, 60, 6), (4, -1, 2), (4, 0, 0)):
        with pytest.raises(BridgeLangHipError, match="BL_E_SHAPE"):
            ops.beam_reorder_kv(table, caches, W, par, row0, n_rows)
    with pytest.raises(TypeError):
        ops.beam_reorder_kv(table, caches, 4, par.long(), 0, 1)
    # a parent outside the prompt's slots keeps the slot's rows; a per-row start outside the cache moves nothing
    caches[0].copy_(torch.randn(8, 2, 64, 128).to(torch.bfloat16))
    before = caches[0].clone()
    ops.beam_reorder_kv(table, caches, 4, torch.tensor([9, -1, 2, 3] * 2, dtype=torch.int32, device=dev), 3, 2)
    ops.beam_reorder_kv(table, caches, 4, torch.tensor([1, 0, 3, 2] * 2, dtype=torch.int32, device=dev),
                        torch.tensor([63] * 4 + [-2] * 4, dtype=torch.int32, device=dev), 2)
    torch.cuda.synchronize()
    want = before.clone()
    want[[0, 1, 2, 3], :, 63] = before[[1, 0, 3, 2], :, 63]                     # row 63 is inside, row 64 is not
    assert torch.equal(caches[0].view(torch.int16), want.view(torch.int16))


# ---- the beams= engine ---------------------------------------------------------------------------------------------------------
def _check_against_spec(eng, tag):
    """The run's own logits and scores through the specification, step by step → the backtracked (ids, wt) and the trace."""
    W, tr = eng.beams, eng.beam_trace()
    logits = eng.logits.cpu().numpy()
    tok, par, wt, sc = (x.cpu().numpy() for x in tr)
    for t in range(eng.n_new):
        for e in range(eng.B // W):
            rows = slice(e * W, (e + 1) * W)
            prev = BM.start_scores(W) if t == 0 else sc[t - 1, rows]
            w_tok, w_par, w_wt, w_sc = BM.beam_step(logits[t, rows], prev, eng.vocab_range)
            assert np.array_equal(tok[t, rows], w_tok) and np.array_equal(par[t, rows], w_par), f"{tag}: step {t} prompt {e}"
            assert np.array_equal(wt[t, rows], w_wt), f"{tag}: weight pairs of step {t} prompt {e}"
            assert np.array_equal(sc[t, rows].view(np.uint32), w_sc.view(np.uint32)), f"{tag}: scores of step {t} prompt {e}"
    r = eng.result()
    ids, pairs = r.ids.cpu().numpy(), r.wt.cpu().numpy()
    for e in range(eng.B // W):
        rows = slice(e * W, (e + 1) * W)
        w_ids, w_pairs = BM.backtrack(tok[:, rows], par[:, rows], wt[:, rows])
        assert np.array_equal(ids[rows], w_ids) and np.array_equal(pairs[rows], w_pairs), f"{tag}: backtrack of prompt {e}"
    return ids, pairs, (tok, par, wt, sc)


def _branches(par, W):
    """Does a reorder of the run move anything: a step 1 … n_new - 2 whose parents are not the identity."""
    return any((par[t].reshape(-1, W) != np.arange(W)).any() for t in range(1, par.shape[0] - 1))


def test_engine_one_prompt_eager_then_captured(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    ids, pv = c["make_inputs"](c["dims"], 1, L, seed=41)
    eng = OpenVLAEngine(c["w"], 4, L, beams=4)
    out = eng.generate(ids.to(dev), pv.to(dev))
    torch.cuda.synchronize()
    e_ids, e_wt, e_trace = _check_against_spec(eng, "eager")
    assert np.array_equal(out.cpu().numpy(), e_ids) and _branches(e_trace[1], 4), "the run must reorder something"
    assert bool((eng.logits[0] == eng.logits[0][0]).all()), "the beams of a prompt are identical rows through the prefill"
    assert np.all(e_trace[1][0] == 0) and np.all(np.diff(e_trace[3][-1]) <= 0)
    assert len({tuple(r) for r in e_ids.tolist()}) == 4, "four distinct actions"
    eng.capture()
    ids2, pv2 = c["make_inputs"](c["dims"], 1, L, seed=42)
    for tag, (i, p) in (("captured, other input", (ids2, pv2)), ("captured", (ids, pv))):
        eng.generate(i.to(dev), p.to(dev))
        torch.cuda.synchronize()
        c_ids, c_wt, c_trace = _check_against_spec(eng, tag)
    assert np.array_equal(c_ids, e_ids) and np.array_equal(c_wt, e_wt)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(c_trace, e_trace))
    with pytest.raises(ValueError):
        eng.set_inputs(torch.cat([ids, ids2]).to(dev), torch.cat([pv, pv2]).to(dev))      # one prompt, not two
    with pytest.raises(ValueError):
        OpenVLAEngine(c["w"], 4, L).beam_trace()


def _prove_kv(dev, beams_eng, score_eng, feeds, tag):
    """The KV proof: the backtracked sequences, forced through a score=True engine that conditions every step on them with
    its own (never reordered) caches, score the beam engine's backtracked pairs bit for bit — at every step. `feeds`: one
    input per seed; the proof runs on the first whose beams change slots between decode steps (a run that never does
    would pass with a reorder that does nothing)."""
    for feed in feeds:
        feed(beams_eng, per_prompt=True)
        beams_eng.run_eager()
        torch.cuda.synchronize()
        ids, wt, trace = _check_against_spec(beams_eng, tag)
        if _branches(trace[1], beams_eng.beams):
            break
    else:
        raise AssertionError(f"{tag}: no input reorders anything")
    score_eng.set_sampling(S.SamplingParams())
    score_eng.set_forced_ids(torch.from_numpy(ids).to(dev))
    feed(score_eng, per_prompt=False)
    score_eng.run_eager()
    torch.cuda.synchronize()
    got = score_eng.gen_wt.permute(1, 0, 2).cpu().numpy()
    for t in range(beams_eng.n_new):
        assert np.array_equal(got[:, t], wt[:, t]), f"{tag}: step {t}: the beams' caches are not their sequences'"
    return feed


@pytest.mark.parametrize("vocab", [None, ACTION_RANGE])
def test_kv_proof_through_a_scoring_engine(dev, vocab):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)

    def feeds():
        for seed in range(43, 51):
            ids, pv = c["make_inputs"](c["dims"], 1, L, seed=seed)

            def feed(eng, per_prompt, ids=ids, pv=pv):
                k = 1 if per_prompt else 4
                eng.set_inputs(ids.repeat(k, 1).to(dev), pv.repeat(k, 1, 1, 1).to(dev))
            yield feed
    _prove_kv(dev, OpenVLAEngine(c["w"], 4, L, beams=4, vocab_range=vocab), OpenVLAEngine(c["w"], 4, L, score=True, vocab_range=vocab),
              feeds(), f"vocab={vocab}")


def test_kv_proof_right_padded(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)

    def feeds():
        for seed in range(60, 68):
            ids, pv = c["make_inputs"](c["dims"], 2, L, seed=seed)
            mask = torch.ones(2, L, dtype=torch.long)
            ids[1, 3], ids[1, 4:], mask[1, 4:] = 29871, 32000, 0                  # lengths L and 4

            def feed(eng, per_prompt, ids=ids, pv=pv, mask=mask):
                k = 1 if per_prompt else 2
                eng.set_padded_inputs(ids.repeat_interleave(k, 0).to(dev), pv.repeat_interleave(k, 0).to(dev),
                                      mask.repeat_interleave(k, 0).to(dev))
            feed.inputs = (ids, pv)
            yield feed
    beams = OpenVLAEngine(c["w"], 4, L, padded=True, beams=2)
    ids, pv = _prove_kv(dev, beams, OpenVLAEngine(c["w"], 4, L, padded=True, score=True), feeds(), "padded").inputs
    got = beams.result(torch.clone)
    alone = OpenVLAEngine(c["w"], 2, 4, beams=2)                                  # the short prompt alone, un-padded
    alone.generate(ids[1:, :4].to(dev), pv[1:].to(dev))
    r = alone.result()
    assert torch.equal(r.ids, got.ids[2:]) and torch.equal(r.wt, got.wt[2:])
    assert torch.equal(alone.beam_scores, beams.beam_scores[:, 2:])


def test_batch_invariance_and_one_beam(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    ids, pv = c["make_inputs"](c["dims"], 3, L, seed=45)
    eng = OpenVLAEngine(c["w"], 12, L, beams=4)
    eng.generate(ids.to(dev), pv.to(dev))
    got, scores = eng.result(torch.clone), eng.beam_scores.clone()
    _check_against_spec(eng, "three prompts")
    one = OpenVLAEngine(c["w"], 4, L, beams=4)
    for e in range(3):
        one.generate(ids[e:e + 1].to(dev), pv[e:e + 1].to(dev))
        r = one.result()
        assert torch.equal(r.ids, got.ids[4 * e:4 * e + 4]) and torch.equal(r.wt, got.wt[4 * e:4 * e + 4]), f"prompt {e}"
        assert torch.equal(one.beam_scores.view(torch.int32), scores[:, 4 * e:4 * e + 4].view(torch.int32)), f"prompt {e}: scores"
    # one beam is the greedy chain; a plain engine's plan has no beam op in it, and the beam plan is that plan with the
    # argmax replaced and the reorders added
    greedy = OpenVLAEngine(c["w"], 3, L)
    want = greedy.generate(ids.to(dev), pv.to(dev)).cpu()
    single = OpenVLAEngine(c["w"], 3, L, beams=1)
    assert torch.equal(single.generate(ids.to(dev), pv.to(dev)).cpu(), want)
    assert bool((single.beam_parent == 0).all())
    plain, beam4 = [o.name for o in OpenVLAEngine(c["w"], 12, L).all_ops()], [o.name for o in eng.all_ops()]
    assert not any("beam" in n for n in plain) and plain.count("bl_argmax_f32") == eng.n_new
    assert [n.replace("bl_beam_step_f32", "bl_argmax_f32") for n in beam4 if n != "bl_beam_reorder_kv_bf16"] == plain
    assert beam4.count("bl_beam_reorder_kv_bf16") == eng.n_new - 2 and beam4.count("bl_beam_step_f32") == eng.n_new
    assert [o.name for o in single.all_ops()] == [n.replace("bl_argmax_f32", "bl_beam_step_f32") for n in [o.name for o in greedy.all_ops()]]
    assert got._fields == ("ids", "wt", "range_wt", "values", "attention") and got.range_wt is None and got.attention is None


# ---- surface -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from test_lora_inference_gpu import new_model
    return new_model(dev)


def _inputs(model, dev, batch, seed=51):
    from test_engine_gpu import make_inputs
    ids, pv = make_inputs(model.dims, batch, 10, seed=seed)
    return ids.to(dev), pv.to(dev)


@pytest.mark.parametrize("action_tokens_only", [False, True])
def test_beam_actions_predict_action_and_scores(model, dev, action_tokens_only):
    ids, pv = _inputs(model, dev, 2)
    kw = dict(action_tokens_only=action_tokens_only)
    actions, tokens, lp = model.beam_actions(ids, pv, "bridge_orig", num_beams=4, **kw)
    assert actions.shape == (2, 4, 7) and tokens.shape == (2, 4, 7) and tokens.dtype == np.int64 and lp.shape == (2, 4, 7)
    # best first: by the fp32 scores, which follow the fp64 sums to 5e-5 each (tests/test_beam_cpu.py derives it)
    assert lp.dtype == np.float64 and np.all(np.isfinite(lp)) and np.all(np.diff(lp.sum(axis=2), axis=1) <= 1e-4)
    assert len({tuple(t) for t in tokens[0].tolist()}) == 4
    if action_tokens_only:
        first, count = model.action_token_range()
        assert tokens.min() >= first and tokens.max() < first + count
    best = model.predict_action(ids, "bridge_orig", pixel_values=pv, num_beams=4, **kw)
    assert best.shape == (2, 7) and np.array_equal(best, actions[:, 0])
    top2 = model.predict_action(ids, "bridge_orig", pixel_values=pv, num_beams=4, num_return_sequences=2, **kw)
    assert top2.shape == (2, 2, 7) and np.array_equal(top2, actions[:, :2])
    a2, t2, l2 = model.beam_actions(ids, pv, "bridge_orig", num_beams=4, num_return_sequences=2, **kw)
    assert np.array_equal(a2, actions[:, :2]) and np.array_equal(t2, tokens[:, :2]) and np.array_equal(l2, lp[:, :2])
    scored = model.score_actions(ids, pv, token_ids=tokens, **kw)
    assert np.array_equal(scored, lp), "score_actions of the beams' tokens is their log-probabilities, bit for bit"
    one = model.beam_actions(ids, pv, "bridge_orig", num_beams=1, **kw)            # one beam: the greedy action, with its log-probabilities
    assert np.array_equal(one[0][:, 0], model.predict_action(ids, "bridge_orig", pixel_values=pv, **kw))
    assert np.array_equal(model.score_actions(ids, pv, token_ids=one[1], **kw), one[2])


def test_generate_surface_and_batching(model, dev):
    ids, pv = _inputs(model, dev, 5, seed=52)
    L0 = ids.shape[1]
    out, wt = model.generate(ids[:2], 7, pixel_values=pv[:2], num_beams=3, num_return_sequences=2, return_weights=True)
    assert tuple(out.shape) == (4, L0 + 7) and out.dtype == torch.int64 and tuple(wt.shape) == (4, 7, 2)
    assert torch.equal(out[:, :L0], ids[:2].repeat_interleave(2, dim=0)), "prompt-major, as HF shapes it"
    _, tokens, lp = model.beam_actions(ids[:2], pv[:2], "bridge_orig", num_beams=3, num_return_sequences=2)
    assert np.array_equal(out[:, L0:].cpu().numpy(), tokens.reshape(4, 7)) and np.array_equal(S.logprob(wt.cpu().numpy()), lp.reshape(4, 7))
    only = model.generate(ids[:2], 7, pixel_values=pv[:2], num_beams=3)
    assert torch.equal(only, out[0::2])
    plain = model.generate(ids[:2], 7, pixel_values=pv[:2])
    assert torch.equal(model.generate(ids[:2], 7, pixel_values=pv[:2], num_beams=1, num_return_sequences=1), plain)
    assert torch.equal(model.generate(ids[:2], 7, pixel_values=pv[:2], num_beams=1, length_penalty=2.0, early_stopping=True), plain)
    # 5 prompts x 4 beams: runs of 4 prompts and 1; every prompt equals its own call
    actions, tokens, lp = model.beam_actions(ids, pv, "bridge_orig", num_beams=4)
    assert tokens.shape == (5, 4, 7)
    for b in range(5):
        a1, t1, l1 = model.beam_actions(ids[b:b + 1], pv[b:b + 1], "bridge_orig", num_beams=4)
        assert np.array_equal(t1[0], tokens[b]) and np.array_equal(l1[0], lp[b]) and np.array_equal(a1[0], actions[b]), f"prompt {b}"
    for kw in (dict(sampling=S.SamplingParams(seed=1)), dict(do_sample=True), dict(forced_ids=tokens[:2, 0]),
               dict(return_attention="segments"), dict(return_values="token"), dict(num_return_sequences=5)):
        with pytest.raises(ValueError):
            model.generate(ids[:2], 7, pixel_values=pv[:2], **{"num_beams": 4, **kw})
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError):
            model.predict_action(ids[:2], "bridge_orig", pixel_values=pv[:2], num_beams=bad)


def test_beams_under_adapters_and_with_values(model, dev):
    from bridgelang_amd.training.value_head import ValueHead
    from test_lora_inference_gpu import dyadic_adapters
    ids, pv = _inputs(model, dev, 2, seed=53)
    base = model.beam_actions(ids, pv, "bridge_orig", num_beams=4)
    model.attach_adapters(dyadic_adapters(model))
    try:
        adapted = model.beam_actions(ids, pv, "bridge_orig", num_beams=4)
        back = model.beam_actions(ids, pv, "bridge_orig", num_beams=4, use_adapters=False)
        assert all(np.array_equal(a, b) for a, b in zip(back, base)), "use_adapters=False is the base policy's beams"
        assert not np.array_equal(adapted[2], base[2]), "the adapters moved the policy"
        assert np.array_equal(model.score_actions(ids, pv, token_ids=adapted[1]), adapted[2])
    finally:
        model.detach_adapters()
    model.attach_value_head(ValueHead(model.dims.llm_dim, dev, init_std=0.05, seed=3))
    try:
        out = model.beam_actions(ids, pv, "bridge_orig", num_beams=4, return_values="action")
        assert len(out) == 4 and out[3].shape == (2,) and all(np.array_equal(a, b) for a, b in zip(out[:3], base))
        greedy_v = model.predict_action(ids, "bridge_orig", pixel_values=pv, return_values="action")[1]
        assert np.array_equal(out[3], greedy_v) and np.all(out[3] != 0), "one state, one V(s)"
    finally:
        model.detach_value_head()
