"""Inference under LoRA adapters on the HIP path (reduced-width model): `attach_adapters` / `use_adapters=`, the learner
round trip `TrainStep(..., lora=lora, refresh_adapted=True)`, and `OpenVLAServer(adapter=…)`.

Dyadic adapters here are A = i/64 (|i| <= 8), B = j/64 (|j| <= 8) at r = 8, alpha = 4 (s = 0.5): sB = j/128, every
product is a multiple of 2^-13 below 2^-7 and a sum of 8 of them a multiple of 2^-13 below 2^-4 — exact in fp32 in any
order, in the merge kernel as in `merged_state_dict()`'s fp32 `b @ a`. Both then form W + Δ with ONE fp32 add and round
it to bf16 once, so the adapted weights — and everything computed from them — equal a second model loaded from
`merged_state_dict()` bit for bit, while Δ is of the size of the synthetic weights themselves (std 0.02).

Rollout / learner mismatch. The sampled tokens' log-probabilities come from the inference engine over the MERGED weights,
the learner's `token_logprobs()` from its training forward y = [x | t]·[W | s·B]ᵀ. The two differ by rounding only: half
a bf16 ulp per merged weight on one side, the rounding of t = x·Aᵀ on the other, on top of the activation roundings that
already differ between the two forwards. The yardstick is the same quantity without adapters — a model holding the merged
weights against a plain TrainStep("vla-train") over it, same tokens — and the LoRA maximum may be at most twice that
baseline maximum. Both are printed. Measured on an MI355X (tiny dims, 2 prompts x 8 samples x 7 tokens, temperature 1.3):
see DESIGN.md §6c.
"""
import json

import numpy as np
import pytest
import torch

from gemm_ref64 import dyadic
from test_engine_gpu import make_inputs

pytestmark = pytest.mark.gpu

STATS = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
B, L = 2, 10


def new_model(dev, seed=11):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=STATS), device=dev, dims=W.tiny_dims()).init_synthetic(seed=seed)


def run(model, ids, pv, **kw):
    """(action token ids [B, 7], the engine's logits [7, B, vocab]) of one greedy `predict_action`."""
    model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key="bridge_orig", **kw)
    eng = model.engine(ids.shape[0], ids.shape[1], use_adapters=kw.get("use_adapters"))
    return eng.gen_ids.t().clone(), eng.logits.clone()


def dyadic_adapters(model):
    from bridgelang_amd.training.lora import LoraAdapters
    lora = LoraAdapters(model.weights, r=8, alpha=4)
    sd = {}
    for i, ad in enumerate(lora.adapters):
        for j, mod in enumerate(ad.modules):
            out, inp = ad.shapes[j]
            sd[f"base_model.model.{mod}.lora_A.weight"] = dyadic((8, inp), 2000 + 8 * i + j, 6, 8)
            sd[f"base_model.model.{mod}.lora_B.weight"] = dyadic((out, 8), 3000 + 8 * i + j, 6, 8)
    return lora.load_state_dict(sd)


@pytest.fixture(scope="module")
def base(dev):
    """The base model, its inputs and its own results — computed once, compared against, never modified."""
    model = new_model(dev)
    ids, pv = make_inputs(model.dims, B, L, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    tok, logits = run(model, ids, pv)
    packed = [g.packed.clone() for g in model.weights.groups]
    return model, ids, pv, tok, logits, packed


def test_peft_init_is_the_base_model(base, dev):
    from bridgelang_amd.training.lora import LoraAdapters
    model, ids, pv, tok0, logits0, _ = base
    lora = LoraAdapters(model.weights, r=8)                     # A ~ N(0, 1/r), B = 0
    model.attach_adapters(lora)
    try:
        tok, logits = run(model, ids, pv)
        assert model.engine(B, L) is not model.engine(B, L, use_adapters=False)
        assert torch.equal(tok, tok0) and torch.equal(logits, logits0)
        for gv, gw in zip(lora.adapted_weights().groups, model.weights.groups):
            assert torch.equal(gv.packed.view(torch.int16), gw.packed.view(torch.int16))
    finally:
        model.detach_adapters()
    assert not any("adapted" in k for k in model._engines)
    with pytest.raises(ValueError):
        model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key="bridge_orig", use_adapters=True)


def test_dyadic_adapters_equal_the_merged_model(base, dev):
    model, ids, pv, tok0, logits0, packed0 = base
    lora = dyadic_adapters(model)
    merged = new_model(dev, seed=3).load_state_dict(lora.merged_state_dict())
    want_tok, want_logits = run(merged, ids, pv)
    model.attach_adapters(lora)
    try:
        index = {id(g): i for i, g in enumerate(model.weights.groups)}
        for ad in lora.adapters:
            i = index[id(ad.group)]
            assert torch.equal(lora.adapted_weights().groups[i].packed.view(torch.int16),
                               merged.weights.groups[i].packed.view(torch.int16)), ad.modules
        tok, logits = run(model, ids, pv)
        assert torch.equal(tok, want_tok) and torch.equal(logits, want_logits)
        assert not torch.equal(logits, logits0)
        tok_b, logits_b = run(model, ids, pv, use_adapters=False)
        assert torch.equal(tok_b, tok0) and torch.equal(logits_b, logits0)
        assert all(torch.equal(g.packed, p) for g, p in zip(model.weights.groups, packed0)), "the base weights were written"
        model.fp8 = True
        with pytest.raises(NotImplementedError):
            model.engine(B, L)
    finally:
        model.fp8 = False
        model.detach_adapters()


def _mismatch(ts, batch, pv_rep):
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv_rep, batch["labels"])
    ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
    ts.forward()
    on = batch["labels"] != -100
    return float((ts.token_logprobs().cpu().double() - batch["old_logprobs"].double())[on].abs().max())


def test_learner_round_trip_and_mismatch(base, dev):
    from bridgelang_amd import sampling as S
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import group_advantages, policy_batch
    from bridgelang_amd.training.step import TrainStep
    model, ids, pv, _, _, packed0 = base
    K, n, temp = 8, 7, 1.3
    sp = S.SamplingParams(temperature=temp, seed=[5, 6])
    lora = LoraAdapters(model.weights, r=8)
    model.attach_adapters(lora)
    try:
        actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=K)
        adv = group_advantages(-np.abs(actions - 0.1).sum(-1))
        pv_rep = pv.repeat_interleave(K, 0)
        batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(B * K, n), lp.reshape(B * K, n), adv.reshape(-1))
        ts = TrainStep(model.weights, "lora", B * K, batch["input_ids"].shape[1], lora=lora, loss="policy",
                       policy=PolicyLossConfig(temperature=temp), max_grad_norm=float("inf"), refresh_adapted=True)
        ts.set_batch(batch["input_ids"], batch["attention_mask"], pv_rep, batch["labels"])
        ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
        score = lambda **kw: model.score_actions(ids, pv, token_ids=tokens, sampling=S.SamplingParams(temperature=temp), **kw)
        before, before_base = score(), score(use_adapters=False)
        assert np.array_equal(before, lp) and np.array_equal(before, before_base)        # B = 0: adapted == base == the rollout
        eng = model.engine(B, L)                                # the adapted greedy engine, captured BEFORE the step
        eng.set_inputs(ids, pv)
        eng.capture()
        buf = lora.adapted_weights().adapted_arena.buf
        for graph in (False, True):                             # one eager step, one graph replay
            loss, norm = ts.step(0.05, graph=graph)
            assert np.isfinite(loss.item()) and norm.item() > 0
            after = score()
            assert not np.array_equal(after, before), f"graph={graph}: the adapted policy did not move"
            assert np.array_equal(score(use_adapters=False), before_base), f"graph={graph}: the base policy moved"
            now = buf.clone()
            lora.refresh()                                      # the step's own refresh ran after the adapters' write-back
            assert torch.equal(buf.view(torch.int16), now.view(torch.int16)), f"graph={graph}: stale adapted weights after the step"
            before = after
        assert all(torch.equal(g.packed, p) for g, p in zip(model.weights.groups, packed0)), "the base weights were written"
        got = eng.generate(ids, pv).clone()                     # replays the graph captured before the steps
        got_logits = eng.logits.clone()
        fresh = OpenVLAEngine(lora.adapted_weights(), B, L)
        assert torch.equal(fresh.generate(ids, pv), got) and torch.equal(fresh.logits, got_logits)

        # rollout / learner mismatch under the trained adapters, against the adapter-free baseline on the merged weights
        actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=K)
        batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(B * K, n), lp.reshape(B * K, n), adv.reshape(-1))
        lora_max = _mismatch(ts, batch, pv_rep)
        merged = new_model(dev, seed=3).load_state_dict(lora.merged_state_dict())
        lp_m = merged.score_actions(ids, pv, token_ids=tokens, sampling=S.SamplingParams(temperature=temp))
        batch_m = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(B * K, n), lp_m.reshape(B * K, n), adv.reshape(-1))
        ts_m = TrainStep(merged.weights, "vla-train", B * K, batch_m["input_ids"].shape[1], loss="policy",
                         policy=PolicyLossConfig(temperature=temp))
        base_max = _mismatch(ts_m, batch_m, pv_rep)
        print(f"\nrollout/learner max |log ratio| over {B * K * n} sampled tokens: LoRA (merged engine vs adapter forward) "
              f"{lora_max:.5f}, adapter-free baseline {base_max:.5f}, ratio {lora_max / base_max:.3f}")
        assert base_max > 0 and lora_max <= 2.0 * base_max
    finally:
        model.detach_adapters()


def test_server_with_adapter_directory(dev, tmp_path):
    from PIL import Image
    from safetensors.torch import save_file
    from bridgelang_amd import serve
    from bridgelang_amd.extern.hf.processing_prismatic import PrismaticProcessor
    from test_serve_gpu import CharTokenizer
    vla = new_model(dev)
    src = dyadic_adapters(vla)
    save_file({k: v.contiguous() for k, v in src.state_dict().items()}, str(tmp_path / "adapter_model.safetensors"))
    (tmp_path / "adapter_config.json").write_text(json.dumps({"peft_type": "LORA", "r": 8, "lora_alpha": 4, "lora_dropout": 0.0,
                                                              "target_modules": "all-linear", "init_lora_weights": "gaussian"}))
    proc = PrismaticProcessor(tokenizer=CharTokenizer())
    server = serve.OpenVLAServer(vla, proc, max_batch=4, max_wait_ms=20, adapter=tmp_path)
    try:
        assert vla._adapters is not None and vla._adapters.scaling == 0.5
        img = np.random.default_rng(0).integers(0, 256, (224, 224, 3), dtype=np.uint8)
        instr = "grasp the snack bag"
        x = proc(serve.get_openvla_prompt(instr, "openvla/openvla-7b"), Image.fromarray(img).convert("RGB"))
        call = lambda **kw: vla.predict_action(input_ids=x["input_ids"].to(dev), pixel_values=x["pixel_values"].to(dev, torch.bfloat16),
                                               unnorm_key="bridge_orig", do_sample=False, **kw)
        want = call()
        got = serve.decode_tree(server.predict_action({"image": serve.encode_ndarray(img), "instruction": instr, "unnorm_key": "bridge_orig"}))
        assert np.array_equal(got, want)
        merged = new_model(dev, seed=3).load_state_dict(src.merged_state_dict())
        assert np.array_equal(want, merged.predict_action(input_ids=x["input_ids"].to(dev), pixel_values=x["pixel_values"].to(dev, torch.bfloat16),
                                                          unnorm_key="bridge_orig", do_sample=False))
        print("server under adapters:", got, " base policy:", call(use_adapters=False))
    finally:
        server.close()
