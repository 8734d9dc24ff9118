"""Attention taps end to end on a small model (full-geometry towers + a 2-layer / 512-wide / 4-head Llama, as
tests/test_hf_boundary_gpu.py builds it): `OpenVLAEngine(attn_taps=...)`, `generate(return_attention=...)`, `attention_maps`.

Bounds: the tap against an fp64 recomputation from the engine's own buffers uses the kernel test's C_P = 0.25 (derived in
tests/test_attention_probs_gpu.py); P_tap·V against the attention output the plan itself computed uses attn_ref64's forward
bound with c = C_O + C_P = 1.5 (the fused kernel's own error against the exact P, plus the tap's error in the P used here)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from attn_ref64 import C_O, assert_attn_close  # noqa: E402

from bridgelang_amd import attention_taps as T  # noqa: E402
from oracle import restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

U, FLOOR, C_P = 2.0 ** -8, 2.0 ** -110, 0.25
STATS = {"bridge_orig": {"action": {"q01": [-1.0, -0.5, -0.25, 0.0, -1.0, -2.0, 0.0], "q99": [1.0, 0.5, 0.75, 2.0, 1.0, 2.0, 1.0],
                                   "mask": [True] * 6 + [False]}}}
SMALL_LLM = dict(vocab_size=32064, pad_token_id=32000, rms_norm_eps=1e-6, hidden_size=512, intermediate_size=1536,
                 num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4)
B, L, P, N_NEW, H, HD = 2, 9, 256, 7, 4, 128
S = P + L
LENS = [9, 6]
BOTH = T.AttnTaps(full=True, segments=True)


@pytest.fixture(scope="module")
def model(dev):
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=STATS, text_config=SMALL_LLM), device=dev).init_synthetic(seed=5)


@pytest.fixture(scope="module")
def inputs(dev):
    g = torch.Generator().manual_seed(11)
    pv = (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    ids = torch.randint(3, 31743, (B, L), generator=g)
    ids[:, 0], ids[:, -1] = 1, 29871
    pad_ids, mask = ids.clone(), torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(LENS):
        pad_ids[b, n - 1] = 29871
        pad_ids[b, n:] = 32000
        mask[b, :n] = 1
    return ids.to(dev), pv, pad_ids.to(dev), mask.to(dev)


@pytest.fixture(scope="module")
def both(model, inputs):
    """One greedy generation with full probabilities and segments, shared (read-only) by the tests below."""
    ids, pv, _, _ = inputs
    out, att = model.generate(ids, N_NEW, pixel_values=pv, return_attention="both")
    return out, att


def _check_p(got, ref, what):
    got = got.detach().cpu().double()
    ratio = float(((got - ref).abs() / (C_P * U * ref + FLOOR)).max())
    print(f"attention taps: {what}: max err/bound {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: err/bound {ratio:.3g}"


@pytest.mark.parametrize("mode", ["greedy", "sampled", "forced"])
def test_taps_are_read_only(model, inputs, mode):
    from bridgelang_amd.sampling import SamplingParams
    ids, pv, _, _ = inputs
    kw, ekw = {}, {}
    if mode == "sampled":
        kw, ekw = dict(sampling=SamplingParams(temperature=[1.0, 2.0], top_k=[50, 0], top_p=[0.95, 1.0], seed=[5, -3]),
                       return_weights=True), dict(sample=True)
    if mode == "forced":
        g = torch.Generator().manual_seed(2)
        kw, ekw = dict(forced_ids=torch.randint(31000, 31743, (B, N_NEW), generator=g)), dict(score=True)
    plain = model.generate(ids, N_NEW, pixel_values=pv, **kw)
    plain_logits = model.engine(B, L, N_NEW, **ekw).logits.clone()
    tapped = model.generate(ids, N_NEW, pixel_values=pv, return_attention="both", **kw)
    assert isinstance(tapped, tuple) and isinstance(tapped[-1], T.ActionAttention)
    tapped_logits = model.engine(B, L, N_NEW, attn_taps=BOTH, **ekw).logits
    assert model.engine(B, L, N_NEW, attn_taps=BOTH, **ekw) is not model.engine(B, L, N_NEW, **ekw)
    assert torch.equal(plain_logits, tapped_logits), "the taps changed the logits"
    plain = plain if isinstance(plain, tuple) else (plain,)
    assert len(tapped) == len(plain) + 1
    for a, b in zip(plain, tapped[:-1]):       # ids, and gen_wt where the mode has them
        assert torch.equal(a, b)


@pytest.fixture
def fp8_model(model):
    model.fp8 = True            # e4m3 prefill projections: part of the engine cache key, so these engines are their own
    yield model
    model.fp8 = False


def test_taps_are_read_only_under_fp8(fp8_model, inputs):
    test_taps_are_read_only(fp8_model, inputs, "greedy")
    assert fp8_model.engine(B, L, N_NEW, attn_taps=BOTH).fp8


def test_shapes_names_rows_and_zero_tail(both):
    out, att = both
    cache_len = (S + N_NEW + 63) // 64 * 64
    assert att.names == T.DEFAULT_NAMES and att.layers == (0, 1)
    assert tuple(att.probs.shape) == (B, N_NEW, 2, H, cache_len) and tuple(att.segments.shape) == (B, N_NEW, 2, H, 4)
    assert att.probs.dtype == torch.float32 and att.segments.dtype == torch.float32
    p = att.probs.cpu().double()
    assert bool(torch.isfinite(p).all()) and bool((p >= 0).all())
    assert float((p.sum(-1) - 1).abs().max()) <= 2.0 ** -9
    for t in range(N_NEW):      # step t's query sits at row S - 1 + t: nothing beyond it
        assert bool((p[:, t, :, :, S + t:] == 0).all())
        assert bool((p[:, t, :, :, S + t - 1] > 0).all())
    assert float((att.segments.cpu().double().sum(-1) - 1).abs().max()) <= 2.0 ** -9
    assert bool((att.segments[:, 0, :, :, 3] == 0).all())      # step 0 sees no generated token


def test_segments_are_the_sums_of_full(model, inputs, both):
    ids, pv, _, _ = inputs
    _, att = both
    names, bounds = T.prompt_segments(torch.ones(B, L), P, N_NEW)

    def check(att, bounds):
        n_seg = bounds.shape[1] - 1
        p = att.probs.cpu().double().permute(0, 3, 1, 2, 4).reshape(B, H, N_NEW * 2, -1)
        s = att.segments.cpu().double().permute(0, 3, 1, 2, 4).reshape(B, H, N_NEW * 2, n_seg)
        ref = T.segment_sums(p, bounds)
        n = (bounds[:, 1:] - bounds[:, :-1]).double().view(B, 1, 1, n_seg)
        assert bool(((s - ref).abs() <= n * 2.0 ** -24 * ref + FLOOR).all())
    check(att, bounds)
    # the text cut into task | description | "\nOut:" pieces
    splits = torch.tensor([[4, 8], [3, 7]])
    _, att2 = model.generate(ids, N_NEW, pixel_values=pv, return_attention="both", text_splits=splits)
    names2, bounds2 = T.prompt_segments(torch.ones(B, L), P, N_NEW, splits)
    assert att2.names == names2 == ("bos", "image", "text0", "text1", "text2", "generated")
    assert tuple(att2.segments.shape) == (B, N_NEW, 2, H, 6) and torch.equal(att2.probs, att.probs)
    check(att2, bounds2)
    assert torch.equal(att2.segments[..., :2], att.segments[..., :2]) and torch.equal(att2.segments[..., 5], att.segments[..., 3])
    # only the asked-for layers and kinds
    _, att3 = model.generate(ids, N_NEW, pixel_values=pv, return_attention="segments", attention_layers=[1])
    assert att3.probs is None and att3.layers == (1,) and torch.equal(att3.segments[:, :, 0], att.segments[:, :, 1])


def test_padded_equals_unpadded_batch_1(model, inputs):
    ids, pv, pad_ids, mask = inputs
    out, att = model.generate(pad_ids, N_NEW, pixel_values=pv, attention_mask=mask, return_attention="both")
    plain = model.generate(pad_ids, N_NEW, pixel_values=pv, attention_mask=mask)
    assert torch.equal(out, plain)
    for b, n in enumerate(LENS):
        o1, a1 = model.generate(pad_ids[b:b + 1, :n], N_NEW, pixel_values=pv[b:b + 1], return_attention="both")
        assert torch.equal(o1[0, n:], out[b, L:])
        real = P + n + N_NEW
        assert torch.equal(a1.probs[0, ..., :real], att.probs[b, ..., :real]), f"sequence {b}: P differs from its un-padded run"
        assert bool((a1.probs[0, ..., real:] == 0).all()) and bool((att.probs[b, ..., real:] == 0).all())
        assert torch.equal(a1.segments[0], att.segments[b]), f"sequence {b}: segments differ from its un-padded run"
        assert float((att.probs[b].double().sum(-1) - 1).abs().max()) <= 2.0 ** -9


def _in_situ(eng, t, q_rot, n_keys, what):
    """The last layer's tap of step t against fp64 P from the engine's own q and cache, and P_tap·V against its own aod."""
    k = eng.k_cache[-1][:, :, :n_keys].float().cpu()
    v = eng.v_cache[-1][:, :, :n_keys].float().cpu().double()
    ref = T.probs_reference(q_rot, k, HD ** -0.5, False)
    got = eng.action_attention().probs[:, t, -1].unsqueeze(2).cpu()              # [B, H, 1, cache_len]
    assert bool((got[..., n_keys:] == 0).all())
    _check_p(got[..., :n_keys], ref, what)
    pg = got[..., :n_keys].double()
    assert_attn_close(eng.aod.view(B, H, 1, HD), pg @ v, pg @ v.abs(), C_O + C_P, f"{what}: P_tap·V vs aod")


def test_in_situ_against_the_engines_own_buffers(model, inputs):
    from bridgelang_amd.engine import OpenVLAEngine
    ids, pv, _, _ = inputs
    D = H * HD
    # step 0: after an n_new = 1 run the last layer's q row S − 1 (rotated in place), aod and cache are still there
    eng = OpenVLAEngine(model.weights, B, L, n_new=1, attn_taps=BOTH)
    eng.set_inputs(ids, pv)
    eng.run_eager()
    torch.cuda.synchronize()
    q = eng.qkv.view(B, S, 3 * D)[:, S - 1, :D].float().cpu().view(B, H, 1, HD)
    _in_situ(eng, 0, q, S, "step 0, last layer")
    # last decode step: qkvd holds its UN-rotated q (fused decode), rotated here as the kernel rotates it
    eng = OpenVLAEngine(model.weights, B, L, n_new=N_NEW, attn_taps=BOTH)
    eng.set_inputs(ids, pv)
    eng.run_eager()
    torch.cuda.synchronize()
    pos = S + N_NEW - 2
    q = eng.qkvd[:, :D].float().cpu().view(B, H, 1, HD)
    q_rot = R.apply_rope(R.Prec(), q, eng.cos.float().cpu(), eng.sin.float().cpu(), pos)
    _in_situ(eng, N_NEW - 1, q_rot, pos + 1, "last decode step, last layer")


def test_step0_taps_equal_attention_maps_rows(model, inputs, both):
    ids, pv, _, _ = inputs
    _, att = both
    maps = model.attention_maps(ids, pv)
    assert len(maps) == 2 and all(tuple(m.shape) == (B, H, S, S) and m.dtype == torch.float32 for m in maps)
    # layers before the last run the same plan on the same data in both engines, and rows are independent of the launch
    assert torch.equal(att.probs[:, 0, 0, :, :S], maps[0][:, :, S - 1, :])
    m = maps[1].cpu().double()
    assert float((m.sum(-1) - 1).abs().max()) <= 2.0 ** -9 and bool((torch.triu(m, 1) == 0).all())
    only1 = model.attention_maps(ids, pv, layers=[1])
    assert only1[0] is None and torch.equal(only1[1], maps[1])


def test_attention_maps_language_only_against_definition(model, inputs):
    from bridgelang_amd import ops
    from bridgelang_amd.engine import OpenVLAEngine
    ids, _, pad_ids, mask = inputs
    D = H * HD
    eng = OpenVLAEngine(model.weights, B, L, all_rows=True, use_mask=True, text_only=True, attn_taps=T.AttnTaps(layers=(0,), full=True,
                                                                                                               segments=False))
    eng.set_inputs(pad_ids, None)
    eng.key_mask.copy_(mask.to(torch.uint8))
    ops.run_all(eng.prefill_ops[:eng.layer_ends[0]])         # layer 0 only: qkv keeps its un-rotated q, k_cache[0] its rotated keys
    torch.cuda.synchronize()
    q = eng.qkv.view(B, L, 3, H, HD)[:, :, 0].permute(0, 2, 1, 3).float().cpu()
    q_rot = R.apply_rope(R.Prec(), q, eng.cos.float().cpu(), eng.sin.float().cpu(), 0)
    ref = T.probs_reference(q_rot, eng.k_cache[0][:, :, :L].float().cpu(), HD ** -0.5, True, mask.cpu())
    got = eng.attention_maps()
    assert got[1] is None
    _check_p(got[0], ref, "language-only layer 0")
    assert bool((got[0].cpu()[ref == 0] == 0).all())
    maps = model.attention_maps(pad_ids, attention_mask=mask, layers=[0])
    assert maps[1] is None and torch.equal(maps[0], got[0])


def test_capture_replay_equals_eager(model, inputs):
    from bridgelang_amd.engine import OpenVLAEngine
    ids, pv, _, _ = inputs
    eng = OpenVLAEngine(model.weights, B, L, n_new=N_NEW, attn_taps=BOTH)
    eng.set_inputs(ids, pv)
    eng.run_eager()
    torch.cuda.synchronize()
    want_p, want_s, want_ids = eng.tap_probs.clone(), eng.tap_seg.clone(), eng.gen_ids.clone()
    eng.capture()
    eng.tap_probs.fill_(-1.0)
    eng.tap_seg.fill_(-1.0)
    eng.replay()
    torch.cuda.synchronize()
    assert torch.equal(eng.gen_ids, want_ids) and torch.equal(eng.tap_probs, want_p) and torch.equal(eng.tap_seg, want_s)
    # one graph serves any segments: the bounds are read on the device
    names, bounds = T.prompt_segments(torch.ones(B, L), P, N_NEW, torch.tensor([[2, 5], [4, 4]]))
    eng.set_segments(names, bounds)
    eng.replay()
    torch.cuda.synchronize()
    got = eng.action_attention().segments.clone()
    eng.run_eager()
    torch.cuda.synchronize()
    assert tuple(got.shape)[-1] == 6 and torch.equal(got, eng.action_attention().segments)
    assert not torch.equal(eng.tap_seg, want_s)


def test_action_surfaces_return_attention(model, inputs):
    from bridgelang_amd.sampling import SamplingParams
    ids, pv, _, _ = inputs
    plain = model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key="bridge_orig")
    acts, att = model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key="bridge_orig", return_attention="segments")
    assert np.array_equal(plain, acts) and att.probs is None and tuple(att.segments.shape) == (B, 7, 2, H, 4)
    sp = SamplingParams(temperature=[1.0, 2.0], top_k=[50, 0], top_p=[0.95, 1.0], seed=[123, -9])
    a0, tok0, lp0 = model.sample_actions(ids, pv, "bridge_orig", sampling=sp, num_samples=2)
    a1, tok1, lp1, satt = model.sample_actions(ids, pv, "bridge_orig", sampling=sp, num_samples=2, return_attention="segments")
    assert np.array_equal(tok0, tok1) and np.array_equal(lp0, lp1) and tuple(satt.segments.shape) == (B, 2, 7, 2, H, 4)
    # the attention under GIVEN actions is the attention of the run that drew them
    lp, catt = model.score_actions(ids, pv, token_ids=tok1, sampling=sp, return_attention="segments")
    assert np.array_equal(lp, lp1) and torch.equal(catt.segments, satt.segments)


def test_what_stays_closed(model, inputs):
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    from bridgelang_amd.serve import OpenVLAServer
    ids, pv, _, _ = inputs
    with pytest.raises(NotImplementedError, match="attention_maps"):
        model(input_ids=ids, pixel_values=pv, output_attentions=True)
    with pytest.raises(ValueError, match="attention taps"):
        StaggeredDecodePipeline(model.weights, B, L, attn_taps=T.AttnTaps())
    with pytest.raises(ValueError, match="attention"):
        OpenVLAServer(model, None, attn_taps=T.AttnTaps())
    with pytest.raises(ValueError):
        model.generate(ids, N_NEW, pixel_values=pv, return_attention="everything")
    with pytest.raises(ValueError):
        model.generate(ids, N_NEW, pixel_values=pv, text_splits=[[2], [2]])
