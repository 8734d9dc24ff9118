"""e4m3 prefill under LoRA adapters (`attach_adapters(lora, fp8=True)`, `model.fp8 = True`) on the HIP path, at llm_dim = 512,
4 heads of 128, llm_inter = 1536 (tiny_dims(): the dims of test_fp8_gpu.py's engine test).

The e4m3 copies of the adapted weights are checked bit for bit against the quantiser specification (fp8_ref64.quantize_spec,
weight_image): applied to `lora.merged_reference(ad)` where the merge itself is exact (the dyadic adapters of
test_lora_inference_gpu.py), else to the adapted bf16 weights as they stand on the device.

Closeness (test_closeness_of_fp8_under_adapters), measured on an MI355X, 3 prompts of 9 tokens, first-token logits:
max |logits_fp8 − logits_bf16| / max |logits_bf16| = 0.0643 under the dyadic adapters, 0.0529 for the base model (the
existing path, the yardstick; ratio 1.215); asserted: adapted > 0, <= 2 x base, <= 0.08 (the bound of test_fp8_gpu.py).

Rollout / learner mismatch (test_learner_step_requantises), max |log ratio| between the sampler's log-probabilities and the
learner's `token_logprobs()` over 2 x 8 x 7 sampled tokens at temperature 1.3 after two optimizer steps, measured on an
MI355X: 0.01419 with the e4m3 rollout engine against 0.00601 with the bf16 one (2.4 x: the e4m3 prefill's quantisation noise
enters the importance ratio); no bound is fixed here."""
import numpy as np
import pytest
import torch

import fp8_ref64 as F
from test_engine_gpu import make_inputs
from test_lora_inference_gpu import _mismatch, dyadic_adapters, new_model, run

pytestmark = pytest.mark.gpu
B, L = 2, 10
NAMES = ("qkv_w", "o_w", "gu_w", "down_w")


def i16(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def base(dev):
    """The base model, its inputs and its own bf16 / e4m3 results — computed once, compared against, never modified."""
    model = new_model(dev)
    d = model.weights.dims
    assert (d.llm_dim, d.llm_heads, d.head_dim, d.llm_inter) == (512, 4, 128, 1536)
    ids, pv = make_inputs(model.dims, B, L, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    _, logits16 = run(model, ids, pv)
    model.fp8 = True
    try:
        _, logits8 = run(model, ids, pv)
        assert any(op.name == "bl_gemm_fp8" for op in model.engine(B, L).prefill_ops)
    finally:
        model.fp8 = False
    packed = [g.packed.clone() for g in model.weights.groups]
    return model, ids, pv, logits16, logits8, packed


def check_copies(lora, model, how: str, what: str):
    """Every layer's four (w8, scale) pairs against the specification. how = "reference": applied to merged_reference (exact
    merges); how = "device": applied to the adapted bf16 weights as they stand. Returns the e4m3 bytes, for change checks."""
    from bridgelang_amd import engine, ops
    view = lora.adapted_weights()
    cache = engine._fp8_layers(view)
    assert cache is lora._fp8 and len(cache) == len(view.layers)
    seen = []
    for i, (lw, lw0, row) in enumerate(zip(view.layers, model.weights.layers, cache)):
        for name in NAMES:
            w8, scale = row[name]
            if how == "reference":
                w = lora.merged_reference(lora.by_packed[getattr(lw0, name).data_ptr()])
                assert torch.equal(i16(ops.unpack_weight(getattr(lw, name)).cpu()), i16(w)), f"{what}: layer {i} {name}: merge not exact"
            else:
                w = ops.unpack_weight(getattr(lw, name)).contiguous().cpu()
            codes, want_s, _ = F.quantize_spec(w)
            F.assert_equal_bytes(scale.cpu().view(torch.int32), want_s.view(torch.int32), f"{what}: layer {i} {name} scales")
            F.assert_equal_bytes(i16(w8.cpu()), i16(F.weight_image(codes)), f"{what}: layer {i} {name} codes")
            seen.append(w8.clone())
    return seen


def test_adapted_fp8_engine_and_refresh(base, dev):
    from bridgelang_amd.engine import OpenVLAEngine
    model, ids, pv, _, logits8_base, packed0 = base
    lora = dyadic_adapters(model)
    model.attach_adapters(lora)                                  # plain attachment still refuses, and names the opt-in
    model.fp8 = True
    with pytest.raises(NotImplementedError, match="enable_fp8"):
        model.engine(B, L)
    model.fp8 = False
    model.attach_adapters(lora, fp8=True)
    try:
        assert lora.fp8_enabled
        before = check_copies(lora, model, "reference", "(a) after attach")                      # (a)
        ptrs = [t.data_ptr() for row in lora._fp8 for pair in row.values() for t in pair]
        model.fp8 = True
        eng = model.engine(B, L)
        assert any(op.name == "bl_gemm_fp8" for op in eng.prefill_ops)                           # (b)
        assert eng.w8 is lora._fp8 and eng is not model.engine(B, L, use_adapters=False)
        tok, logits = run(model, ids, pv)
        assert not torch.equal(logits, logits8_base)
        _, logits_b = run(model, ids, pv, use_adapters=False)
        assert torch.equal(logits_b, logits8_base), "use_adapters=False is not the base fp8 engine"
        assert all(torch.equal(g.packed, p) for g, p in zip(model.weights.groups, packed0)), "the base weights were written"
        assert model.weights.__dict__["_fp8_layers"] is not lora._fp8
        eng.set_inputs(ids, pv)                                                                  # (c): a graph captured BEFORE the refresh
        eng.capture()
        for ad in lora.adapters:
            ad.B.neg_()                                          # still dyadic: the merge stays exact
        lora.refresh()
        after = check_copies(lora, model, "reference", "(c) after refresh")
        assert all(not torch.equal(i16(a), i16(b)) for a, b in zip(before, after)), "the e4m3 copies did not change"
        assert ptrs == [t.data_ptr() for row in lora._fp8 for pair in row.values() for t in pair], "a refresh moved a buffer"
        got = eng.generate(ids, pv).clone()                      # replays the captured graph
        got_logits = eng.logits.clone()
        assert not torch.equal(got_logits, logits)
        fresh = OpenVLAEngine(lora.adapted_weights(), B, L, fp8=True)
        assert torch.equal(fresh.generate(ids, pv), got) and torch.equal(fresh.logits, got_logits)
        # generate(forced_ids=) goes through model.engine as well: the greedy tokens of this engine have positive weight under it
        out, wt = model.generate(ids, pixel_values=pv, max_new_tokens=7, forced_ids=got)
        assert torch.equal(out[:, L:], got) and bool((wt[..., 0] > 0).all())
        assert any(op.name == "bl_gemm_fp8" for k, e in model._engines.items() if "adapted" in k and "score" in k for op in e.prefill_ops)
    finally:
        model.fp8 = False
        model.detach_adapters()


def test_closeness_of_fp8_under_adapters(base, dev):
    """(d) — figures in the module docstring."""
    model, _, _, _, _, _ = base
    Bc, Lc = 3, 9
    ids, pv = make_inputs(model.dims, Bc, Lc, seed=1)
    ids, pv = ids.to(dev), pv.to(dev)
    first = lambda **kw: run(model, ids, pv, **kw)[1][0].clone()
    lora = dyadic_adapters(model)
    model.attach_adapters(lora, fp8=True)
    try:
        a16, b16 = first(), first(use_adapters=False)
        model.fp8 = True
        a8, b8 = first(), first(use_adapters=False)
    finally:
        model.fp8 = False
        model.detach_adapters()
    r_ad = ((a8 - a16).abs().amax() / a16.abs().amax()).item()
    r_base = ((b8 - b16).abs().amax() / b16.abs().amax()).item()
    print(f"\nfp8 prefill vs bf16, max |dlogit| / scale: under adapters {r_ad:.4f}, base model {r_base:.4f}, ratio {r_ad / r_base:.3f}")
    assert r_base > 0
    assert 0 < r_ad <= 2.0 * r_base
    assert r_ad <= 0.08


def test_sampled_logprobs_are_scored_bit_for_bit(base, dev):
    """(e) the existing guarantee of sample_actions / score_actions, on the e4m3 engine under adapters."""
    from bridgelang_amd import sampling as S
    model, ids, pv, _, _, _ = base
    lora = dyadic_adapters(model)
    model.attach_adapters(lora, fp8=True)
    model.fp8 = True
    try:
        sp = S.SamplingParams(temperature=1.3, seed=[5, 6])
        actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=4)
        scored = model.score_actions(ids, pv, token_ids=tokens, sampling=S.SamplingParams(temperature=1.3))
        assert np.isfinite(lp).all() and np.array_equal(scored, lp)
        assert any(op.name == "bl_gemm_fp8" for k, e in model._engines.items() if "adapted" in k for op in e.prefill_ops)
        base_lp = model.score_actions(ids, pv, token_ids=tokens, sampling=S.SamplingParams(temperature=1.3), use_adapters=False)
        assert not np.array_equal(base_lp, lp)
    finally:
        model.fp8 = False
        model.detach_adapters()


def test_building_the_step_runs_the_whole_refresh(base, dev):
    """Adapters changed AFTER attach (a checkpoint loaded into them, say), then the step is built: building runs the plan it
    copies — merge AND quantise — so before any optimizer step the adapted bf16 weights are merged_reference of the live
    A / B and the e4m3 copies their specification. (Running only the plan's last op, the quantise, would leave both on the old adapters.)"""
    from bridgelang_amd.training.step import TrainStep
    model, ids, pv, _, _, packed0 = base
    lora = dyadic_adapters(model)
    model.attach_adapters(lora, fp8=True)
    try:
        before = check_copies(lora, model, "reference", "after attach")
        old = [g.packed.clone() for g in lora.adapted_weights().groups]
        for ad in lora.adapters:
            ad.B.neg_()                                          # still dyadic: the merge stays exact; no refresh() here
        ts = TrainStep(model.weights, "lora", B, L + 8, lora=lora, max_grad_norm=float("inf"), refresh_adapted=True)
        assert [op.name for op in ts.lin.adapter_ops[-2:]] == ["bl_lora_merge_batched_bf16", "bl_quantize_weight_fp8_packed_batched"]
        after = check_copies(lora, model, "reference", "after building the step")
        assert all(not torch.equal(i16(a), i16(b)) for a, b in zip(before, after)), "the e4m3 copies are those of the old adapters"
        index = {id(g): i for i, g in enumerate(model.weights.groups)}
        for ad in lora.adapters:                                 # every adapted group, not only the decoder layers
            i = index[id(ad.group)]
            got = lora.adapted_weights().groups[i].packed
            assert not torch.equal(i16(got), i16(old[i])), ad.modules
        assert all(torch.equal(g.packed, p) for g, p in zip(model.weights.groups, packed0)), "the base weights were written"
    finally:
        model.detach_adapters()


def test_learner_step_requantises(base, dev):
    """(f) TrainStep(stage LoRA, refresh_adapted=True) built AFTER fp8 was enabled: after each step the e4m3 copies are the
    specification of the refreshed adapted weights; and the rollout / learner mismatch with the e4m3 rollout engine beside the
    bf16 one (printed; figures in the module docstring)."""
    from bridgelang_amd import sampling as S
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import group_advantages, policy_batch
    from bridgelang_amd.training.step import TrainStep
    model, ids, pv, _, _, packed0 = base
    K, n, temp = 8, 7, 1.3
    sp = S.SamplingParams(temperature=temp, seed=[5, 6])
    lora = LoraAdapters(model.weights, r=8)                      # A ~ N(0, 1/r), B = 0
    model.attach_adapters(lora, fp8=True)
    model.fp8 = True
    try:
        actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=K)
        adv = group_advantages(-np.abs(actions - 0.1).sum(-1))
        pv_rep = pv.repeat_interleave(K, 0)
        batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(B * K, n), lp.reshape(B * K, n), adv.reshape(-1))
        ts = TrainStep(model.weights, "lora", B * K, batch["input_ids"].shape[1], lora=lora, loss="policy",
                       policy=PolicyLossConfig(temperature=temp), max_grad_norm=float("inf"), refresh_adapted=True)
        assert [op.name for op in ts.lin.adapter_ops[-2:]] == ["bl_lora_merge_batched_bf16", "bl_quantize_weight_fp8_packed_batched"]
        ts.set_batch(batch["input_ids"], batch["attention_mask"], pv_rep, batch["labels"])
        ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
        before = check_copies(lora, model, "device", "(f) before the step")
        for graph in (False, True):                              # one eager step, one graph replay
            loss, norm = ts.step(0.05, graph=graph)
            assert np.isfinite(loss.item()) and norm.item() > 0
            after = check_copies(lora, model, "device", f"(f) after the step, graph={graph}")
            assert any(not torch.equal(i16(a), i16(b)) for a, b in zip(before, after)), f"graph={graph}: the e4m3 copies did not move"
            before = after
        assert all(torch.equal(g.packed, p) for g, p in zip(model.weights.groups, packed0)), "the base weights were written"

        figures = {}
        for fp8 in (True, False):                                # rollout under the trained adapters: e4m3 engine, then bf16 engine
            model.fp8 = fp8
            actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=K)
            batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(B * K, n), lp.reshape(B * K, n), adv.reshape(-1))
            figures[fp8] = _mismatch(ts, batch, pv_rep)
        print(f"\nrollout/learner max |log ratio| over {B * K * n} sampled tokens under LoRA: e4m3 rollout engine {figures[True]:.5f}, "
              f"bf16 rollout engine {figures[False]:.5f}")
        assert np.isfinite(figures[True]) and figures[True] > 0
    finally:
        model.fp8 = False
        model.detach_adapters()
