"""The host side of e4m3 prefill under LoRA adapters, no kernel: the lane mapping of csrc/quantize_weight_fp8.hip between the
packed bf16 image and the packed e4m3 image (against fp8_ref64.weight_image and the bf16 packing of weights._pack), the
work-item count of the batched table, and `LoraAdapters.enable_fp8()` on CPU-allocated weights at llm_dim = 512, 4 heads of
128, llm_inter = 1536 (the dims of test_fp8_gpu.py's engine test — tiny_dims()).

test_lane_mapping_against_weight_image documents the mapping: it restates it in Python against the two layout definitions
and does not run the kernel's own index arithmetic — tests/test_weight_fp8_gpu.py pins that, bit for bit."""
import dataclasses

import pytest
import torch

import fp8_ref64 as F

NAMES = ("qkv_w", "o_w", "gu_w", "down_w")


def restate_kernel(packed_bf16: torch.Tensor, codes_of) -> torch.Tensor:
    """The kernel's data movement on the CPU: for every e4m3 fragment (nt, ks8) and lane L, the 16 bytes written are
    codes_of(the 8 bf16 of fragment (nt, 2·ks8 + (L >> 5)), lane (L & 15) + 32·((L >> 4) & 1)) followed by those of the lane
    16 above it. packed_bf16 [n/16, k/32, 64, 8]; codes_of maps bf16 [..., 8] to uint8 [..., 8]. Returns uint8
    [n/16, k/64, 64, 16]."""
    NT, KS = packed_bf16.shape[:2]
    L = torch.arange(64)
    src = (L & 15) + 32 * ((L >> 4) & 1)
    frag = packed_bf16.view(NT, KS // 2, 2, 64, 8)[:, :, L >> 5, :, :]            # [NT, KS/2, 64 (L), 64 (lanes), 8]
    lo = frag[:, :, L, src, :]                                                    # [NT, KS/2, 64, 8]
    hi = frag[:, :, L, src + 16, :]
    return torch.cat([codes_of(lo), codes_of(hi)], dim=-1)


@pytest.mark.parametrize("n,k", [(16, 128), (48, 384), (32, 4096), (16, 11008)])
def test_lane_mapping_against_weight_image(n, k):
    """Bytes that identify their own (row, column): the mapping must move code (r, c) of the row-major matrix to where
    weight_image puts it, for every byte — 16-bit column tags keep 4096 and 11008 columns distinct."""
    from bridgelang_amd import weights as W
    r, c = torch.arange(n)[:, None], torch.arange(k)[None, :]
    tag = ((r * 131 + c * 7) % 251).to(torch.uint8)                               # the "code" of element (r, c)
    ident = (r * k + c).to(torch.int32)                                           # carried through the bf16 image as two int16 halves
    img = torch.zeros(n // 16, k // 32, 64, 8, dtype=torch.bfloat16)
    got = torch.zeros(n * k, dtype=torch.int32)
    for shift in (0, 16):                                                         # low / high 16 bits of the identity, as bf16 bit patterns
        W._pack(((ident >> shift) & 0xFFFF).to(torch.int16).view(torch.bfloat16).contiguous(), img)
        part = restate_kernel(img, lambda t: t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF)
        got |= part.reshape(-1) << shift
    want_pos = F.packed_index(n, k)                                               # byte offset of code (r, c) in the image
    assert torch.equal(got[want_pos.reshape(-1)], ident.reshape(-1))
    # and with real codes: the image of the restated kernel equals weight_image of the row-major codes
    W._pack(tag.to(torch.int16).view(torch.bfloat16).contiguous(), img)
    image = restate_kernel(img, lambda t: t.contiguous().view(torch.int16).to(torch.uint8))
    F.assert_equal_bytes(image.reshape(-1), F.pack_image(tag), f"image {n}x{k}")
    F.assert_equal_bytes(image.reshape(-1).view(torch.bfloat16).view(n // 16, k // 64, 64, 8).view(torch.int16),
                         F.weight_image(tag).view(torch.int16), f"weight_image {n}x{k}")


def test_item_decomposition_and_table_entry():
    import ctypes as C
    from bridgelang_amd import _lib, train_ops as T
    assert [T.quantize_packed_items(n, k) for n, k in ((16, 128), (48, 384), (4608, 512), (12288, 4096))] == [1, 3, 288, 768]
    d = _lib.WeightQuantDesc
    assert C.sizeof(d) == 48 and d.first_item.offset == 40 and d.n.offset == 24 and d.n_items.offset == 32     # struct WeightQuantEntry
    assert {"bl_quantize_weight_fp8_packed", "bl_quantize_weight_fp8_packed_batched"} <= set(_lib.SIGNATURES)


def _model(dims=None):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    dims = W.tiny_dims() if dims is None else dims
    assert (dims.llm_dim, dims.llm_heads, dims.head_dim) == (512, 4, 128)
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device="cpu", dims=dims)


def test_enable_fp8_buffers_and_cache():
    from bridgelang_amd import engine
    from bridgelang_amd.training.lora import LoraAdapters
    model = _model()
    d = model.weights.dims
    assert d.llm_inter == 1536
    lora = LoraAdapters(model.weights, r=8)
    assert lora.fp8_enabled is False
    assert lora.enable_fp8() is lora and lora.fp8_enabled is True
    view = lora.adapted_weights()
    cache = engine._fp8_layers(view)
    assert isinstance(cache, list) and len(cache) == d.llm_layers and cache is view.__dict__["_fp8_layers"]
    D, I = d.llm_dim, d.llm_inter
    want = {"qkv_w": (3 * D, D), "o_w": (D, D), "gu_w": (2 * I, D), "down_w": (D, I)}
    seen = set()
    for lw, row in zip(view.layers, cache):
        assert tuple(row) == NAMES
        for name in NAMES:
            w8, s = row[name]
            n, k = want[name]
            assert tuple(getattr(lw, name).shape) == (n // 16, k // 32, 64, 8)
            assert w8.dtype == torch.bfloat16 and tuple(w8.shape) == (n // 16, k // 64, 64, 8) and w8.is_contiguous()
            assert s.dtype == torch.float32 and tuple(s.shape) == (n,) and s.is_contiguous()
            assert w8.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
            seen |= {w8.data_ptr(), s.data_ptr()}
    assert len(seen) == 8 * d.llm_layers                                          # one Arena, distinct slots
    base = lora._fp8_arena.buf.data_ptr()
    assert all(base <= p < base + lora._fp8_arena.nbytes for p in seen)
    assert "_fp8_layers" not in model.weights.__dict__                            # the base model's cache is its own
    assert lora.enable_fp8() is lora and engine._fp8_layers(view) is cache        # idempotent: same tensors
    # the model surface: the opt-in lifts the refusal (the refusal itself: test_plain_attach_still_refuses)
    model.attach_adapters(lora, fp8=True)
    assert model._adapters is lora


def test_enable_fp8_needs_multiples_of_128():
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.lora import LoraAdapters
    model = _model(dataclasses.replace(W.tiny_dims(), llm_inter=1600))
    lora = LoraAdapters(model.weights, r=8)
    with pytest.raises(ValueError):
        lora.enable_fp8()
    assert lora.fp8_enabled is False
    kept = LoraAdapters(model.weights, r=8)
    model.attach_adapters(kept)
    with pytest.raises(ValueError):
        model.attach_adapters(lora, fp8=True)
    assert model._adapters is kept                                                # a failed opt-in drops nothing that was attached


def test_enable_fp8_after_the_plan_was_handed_out_raises(monkeypatch):
    """TrainStep copies `refresh_ops()`: enabling fp8 afterwards would leave that copy refreshing bf16 only. The launch
    builders are stubbed (CPU tensors cannot make a launch); the hand-out and the guard are the real ones."""
    from bridgelang_amd import train_ops as T
    from bridgelang_amd.training.lora import LoraAdapters
    monkeypatch.setattr(T, "be_lora_merge", lambda *a, **k: ("merge-entry", ()))
    monkeypatch.setattr(T, "lora_merge_batched", lambda entries, device, run=False: ("merge", len(entries)))
    monkeypatch.setattr(T, "be_quantize_packed", lambda wp, w8, s: ((wp.data_ptr(), w8.data_ptr(), s.data_ptr()), ()))
    monkeypatch.setattr(T, "quantize_packed_batched", lambda entries, device, run=False: ("quantise", [e[0] for e in entries]))
    model = _model()
    late = LoraAdapters(model.weights, r=8)
    plan = late.refresh_ops()
    assert [p[0] for p in plan] == ["merge"]
    with pytest.raises(RuntimeError, match="before"):
        late.enable_fp8()
    assert late.fp8_enabled is False and late.refresh_ops() is plan
    early = LoraAdapters(model.weights, r=8).enable_fp8()
    plan = early.refresh_ops()
    assert [p[0] for p in plan] == ["merge", "quantise"] and plan[0][1] == len(early.adapters)
    view = early.adapted_weights()
    want = [(getattr(lw, n).data_ptr(), row[n][0].data_ptr(), row[n][1].data_ptr()) for lw, row in zip(view.layers, early._fp8) for n in NAMES]
    assert plan[1][1] == want                                                     # every layer's four weights, from the ADAPTED view
    assert early.enable_fp8() is early and early.refresh_ops() is plan            # already enabled: no error, same plan


def test_plain_attach_still_refuses():
    from bridgelang_amd.training.lora import LoraAdapters
    model = _model()
    lora = LoraAdapters(model.weights, r=8)
    model.attach_adapters(lora)
    model.fp8 = True
    with pytest.raises(NotImplementedError, match="enable_fp8"):
        model.engine(1, 8)
    assert model._resolve_adapters(False) is False                                # use_adapters=False: the base engine's route
