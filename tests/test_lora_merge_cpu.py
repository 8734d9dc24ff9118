"""The host side of inference under LoRA adapters: the merge specification (training/lora.py::merged_reference), the
adapted weight view (weights.py::VLAWeights.adapted_view) and `load_adapter` — on CPU-allocated tiny weights, no kernel.

Dyadic adapters. A = i/8 (|i| <= 8), B = j/16 (|j| <= 16), s = alpha / r = 4 / 8 = 0.5, W = i/64 (|i| <= 127): sB = j/32
exactly, every product is a multiple of 2^-8 with |·| <= 0.5, and W + Σ over r = 8 of them is a multiple of 2^-8 below 6 —
exact in fp32 as well as in fp64. `merged_state_dict()` (PEFT's merge_and_unload in fp32 torch, per module) and
`merged_reference` (fp64, per fused group) then round the same exact value once: the packed results must be equal bit for
bit for a single, a stacked (q ‖ k ‖ v) and an interleaved (gate / up) group.
"""
import json

import numpy as np
import pytest
import torch

import train_ref64 as T64
from gemm_ref64 import dyadic, gauss


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def tiny():
    """CPU weights with dyadic GEMM groups + dyadic adapters at r = 8, alpha = 4 (s = 0.5). Shared, never modified."""
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.lora import LoraAdapters
    w = W.allocate(W.tiny_dims(), "cpu")
    for gi, g in enumerate(w.groups):
        st = torch.zeros(g.n, g.k)
        for name in g.members:                       # members only: K padding and padded rows stay zero
            pl = w.placements[name]
            W._block_view(st.view(-1), pl).copy_(dyadic((pl.rows, pl.cols), 1000 + gi, 6, 127))
        W._pack(st.to(torch.bfloat16), g.packed)
    lora = LoraAdapters(w, r=8, alpha=4)
    sd = {}
    for i, ad in enumerate(lora.adapters):
        for j, mod in enumerate(ad.modules):
            out, inp = ad.shapes[j]
            sd[f"base_model.model.{mod}.lora_A.weight"] = dyadic((8, inp), 2000 + 8 * i + j, 3, 8)
            sd[f"base_model.model.{mod}.lora_B.weight"] = dyadic((out, 8), 3000 + 8 * i + j, 4, 16)
    lora.load_state_dict(sd)
    return w, lora, sd


def test_spec_against_an_independent_restatement():
    """numpy fp64 sums term by term and train_ref64.rb64 (round(v / ulp)·ulp) instead of the bit manipulation of bf16_rne_bits."""
    from bridgelang_amd.training.lora import bf16_rne_bits, merged_reference
    n, k, R, s = 32, 64, 64, 0.37
    W, A, B = (t.to(torch.bfloat16) for t in (gauss((n, k), 1, 0.02), gauss((R, k), 2, 1.0 / 32), gauss((n, R), 3, 0.05)))
    got, total, sB = merged_reference(W, A, B, s, exact=True)
    sb = (B.float().numpy() * np.float32(s)).astype(np.float32)
    sb = torch.from_numpy(sb).to(torch.bfloat16).double().numpy()                    # fp32 product, one RNE to bf16
    assert np.array_equal(sb, sB.double().numpy())
    ref = W.double().numpy().copy()
    for r in range(R):
        ref += sb[:, r:r + 1] * A.double().numpy()[r:r + 1, :]
    assert np.abs(ref - total.numpy()).max() <= 2.0 ** -50
    want = T64.rb64(torch.from_numpy(ref))
    assert torch.equal(got.double(), want) and float((got.double() - W.double()).abs().max()) > 0
    # the single rounding itself: ties to even, and a value fp32 would round up to a tie first
    x = np.array([1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -30, 1 + 3 * 2.0 ** -8, -1 - 3 * 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -40, 0.0])
    assert [hex(v) for v in bf16_rne_bits(x)] == ["0x3f80", "0x3f80", "0x3f81", "0x3f82", "0xbf82", "0x3f80", "0x0"]
    v = torch.from_numpy(np.random.default_rng(0).standard_normal(4096) * 3.0)
    assert np.array_equal(bf16_rne_bits(v.numpy()), bits(T64.rb64(v).to(torch.bfloat16)).numpy().view(np.uint16))


def test_zero_update_is_the_identity_bit_for_bit():
    from bridgelang_amd.training.lora import merged_reference
    W = gauss((16, 32), 4, 0.02).to(torch.bfloat16)
    W.view(-1)[:4] = torch.tensor([0.0, -0.0, 2.0 ** -120, -3.0], dtype=torch.bfloat16)
    A, B = gauss((64, 32), 5).to(torch.bfloat16), gauss((16, 64), 6).to(torch.bfloat16)
    assert torch.equal(bits(merged_reference(W, A, torch.zeros_like(B), 0.5)), bits(W))        # PEFT's initial state
    assert torch.equal(bits(merged_reference(W, A, B, 0.0)), bits(W))
    # an update below half an ulp of W is absorbed; K-padding columns (A's are zero) stay zero
    one, a, b = torch.ones(16, 32, dtype=torch.bfloat16), torch.zeros(64, 32, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.bfloat16)
    a[0], b[:, 0] = 2.0 ** -5, 2.0 ** -5
    assert torch.equal(merged_reference(one, a, b, 0.5), one)
    W[:, 24:], A[:, 24:] = 0, 0
    assert bool((merged_reference(W, A, B, 0.5)[:, 24:] == 0).all())


@pytest.mark.parametrize("mode", ["single", "concat", "interleave"])
def test_dyadic_merge_equals_merged_state_dict(tiny, mode):
    from bridgelang_amd import weights as W
    w, lora, _ = tiny
    ads = [ad for ad in lora.adapters if ad.mode == mode]
    assert ads and len(ads[0].modules) == {"single": 1, "concat": 3, "interleave": 2}[mode]
    w2 = W.allocate(w.dims, "cpu").load_state_dict(lora.merged_state_dict())
    index = {id(g): i for i, g in enumerate(w.groups)}
    for ad in ads:
        ref = lora.merged_reference(ad)
        packed = torch.zeros_like(ad.group.packed)
        W._pack(ref, packed)
        assert torch.equal(bits(packed), bits(w2.groups[index[id(ad.group)]].packed)), ad.modules
        assert not torch.equal(bits(packed), bits(ad.group.packed))


def _tensors(w):
    out = {"embed": w.embed, "norm": w.norm, "lm_head": w.lm_head}
    for key in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"):
        out[key] = getattr(w, key)
    for tn in ("dino", "siglip"):
        t = getattr(w, tn)
        out.update({f"{tn}.{f}": getattr(t, f) for f in ("patch_w", "patch_b", "pos", "prefix") if getattr(t, f) is not None})
        for i, b in enumerate(t.blocks):
            out.update({f"{tn}.{i}.{f}": v for f, v in vars(b).items() if v is not None})
    for i, l in enumerate(w.layers):
        out.update({f"layers.{i}.{f}": v for f, v in vars(l).items()})
    out.update({f"passthrough.{k}": v for k, v in w.passthrough.items()})
    return out


def test_adapted_view(tiny):
    w, lora, _ = tiny
    chosen = [ad.group for ad in lora.adapters]
    before = {k: t.data_ptr() for k, t in _tensors(w).items()}
    v = w.adapted_view(chosen)
    assert {k: t.data_ptr() for k, t in _tensors(w).items()} == before            # the base is not re-pointed
    replaced = {g.packed.data_ptr() for g in chosen}
    assert len(replaced) == len(chosen) == 27 and len(w.groups) == 30               # all but lm_head and the two patch embeddings
    tv = _tensors(v)
    lo, hi = v.adapted_arena.buf.data_ptr(), v.adapted_arena.buf.data_ptr() + v.adapted_arena.nbytes
    n_new = 0
    for key, t in _tensors(w).items():
        if t.data_ptr() in replaced:                                                # new storage inside the ONE new arena, same values
            n_new += 1
            assert lo <= tv[key].data_ptr() < hi and tv[key].shape == t.shape and torch.equal(tv[key], t), key
        else:                                                                       # shared
            assert tv[key].data_ptr() == t.data_ptr(), key
    assert n_new == len(chosen)
    assert v.lm_head.data_ptr() == w.lm_head.data_ptr() and v.dino.patch_w.data_ptr() == w.dino.patch_w.data_ptr()
    # groups / placements / dataclass fields agree, and belong to the view
    by_ptr = {t.data_ptr(): k for k, t in tv.items()}
    for gv, gw in zip(v.groups, w.groups):
        assert gv is not gw and (gv.n, gv.k, gv.members) == (gw.n, gw.k, gw.members) and gv.packed.data_ptr() in by_ptr
        for name in gv.members:
            assert v.placements[name].group is gv and w.placements[name].group is gw
    assert v.layers[1].gu_w.data_ptr() == v.placements["language_model.model.layers.1.mlp.up_proj.weight"].group.packed.data_ptr()
    assert v.siglip.blocks[0].fc2_w.data_ptr() == v.placements[f"{w.dims.siglip.prefix}.blocks.0.mlp.fc2.weight"].group.packed.data_ptr()
    for name, pl in w.placements.items():
        if pl.group is None:
            assert v.placements[name].dst.data_ptr() == pl.dst.data_ptr()
    assert "_fp8_layers" not in v.__dict__ and v.dims is w.dims
    # the view reads as the same model; writing one of its groups leaves the base alone
    sd_w, sd_v = w.state_dict(), v.state_dict()
    assert all(torch.equal(sd_w[k], sd_v[k]) for k in sd_w)
    gi = next(i for i, g in enumerate(w.groups) if g.packed.data_ptr() == w.layers[0].o_w.data_ptr())
    v.layers[0].o_w.zero_()
    assert float(w.layers[0].o_w.float().abs().max()) > 0 and float(v.groups[gi].packed.float().abs().max()) == 0
    # a subset by index
    v2 = w.adapted_view([0])
    assert v2.groups[0].packed.data_ptr() != w.groups[0].packed.data_ptr()
    assert all(a.packed.data_ptr() == b.packed.data_ptr() for a, b in zip(v2.groups[1:], w.groups[1:]))
    with pytest.raises(IndexError):
        w.adapted_view([len(w.groups)])
    # LoraAdapters builds its view once, over exactly its groups
    av = lora.adapted_weights()
    assert lora.adapted_weights() is av and av.lm_head.data_ptr() == w.lm_head.data_ptr()
    assert all(av.groups[i].packed.data_ptr() != g.packed.data_ptr() for i, g in enumerate(w.groups) if id(g) in {id(c) for c in chosen})


def _model(w_src=None):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device="cpu", dims=W.tiny_dims())


def test_load_adapter_round_trip_and_errors(tiny, tmp_path):
    from safetensors.torch import save_file
    _, lora, sd = tiny
    cfg = {"peft_type": "LORA", "r": 8, "lora_alpha": 4, "lora_dropout": 0.0, "target_modules": "all-linear",
           "init_lora_weights": "gaussian"}                                          # as training/finetune.py::save_checkpoint writes it
    d = tmp_path / "adapter"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in lora.state_dict().items()}, str(d / "adapter_model.safetensors"))
    (d / "adapter_config.json").write_text(json.dumps(cfg))
    model = _model()
    with pytest.raises(ValueError):
        model.engine(1, 8, use_adapters=True)                                        # nothing attached
    assert model.load_adapter(d) is model
    got = model._adapters
    assert (got.r, got.alpha, got.scaling) == (8, 4, 0.5) and got.w is model.weights
    back = got.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    for a, b in zip(got.adapters, lora.adapters):
        assert torch.equal(a.A, b.A) and torch.equal(a.B, b.B) and a.mode == b.mode
    model.fp8 = True
    with pytest.raises(NotImplementedError):
        model.engine(1, 8)                                                           # e4m3 copies would go stale on refresh
    model.fp8 = False
    model.detach_adapters()
    assert model._adapters is None
    with pytest.raises(ValueError):
        model.attach_adapters(lora)                                                  # built over another model's weights
    # a module this model has no group for / a missing module / a wrong shape / missing files
    extra = dict(lora.state_dict())
    extra["base_model.model.language_model.model.layers.7.mlp.down_proj.lora_A.weight"] = torch.zeros(8, 16)
    e = tmp_path / "extra"
    e.mkdir()
    save_file(extra, str(e / "adapter_model.safetensors"))
    (e / "adapter_config.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="no adapter group"):
        model.load_adapter(e)
    fewer = {k: v for k, v in lora.state_dict().items() if "layers.0.self_attn.k_proj" not in k}
    save_file(fewer, str(e / "adapter_model.safetensors"))
    with pytest.raises(ValueError, match="missing"):
        model.load_adapter(e)
    save_file({k: v.contiguous() for k, v in lora.state_dict().items()}, str(e / "adapter_model.safetensors"))
    (e / "adapter_config.json").write_text(json.dumps(dict(cfg, r=16)))
    with pytest.raises(ValueError):
        model.load_adapter(e)                                                        # shapes are r = 8
    with pytest.raises(FileNotFoundError):
        model.load_adapter(tmp_path / "nowhere")
    assert model._adapters is None
