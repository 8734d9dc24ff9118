"""LoRA adapters for the fine-tuning loop of vla-scripts/finetune.py:174-189 (PEFT `LoraConfig(r, lora_alpha=min(r, 16),
lora_dropout=0.0, target_modules="all-linear", init_lora_weights="gaussian")`): every nn.Linear except lm_head gets
y = W x + (alpha / r) · B (A x), A ~ N(0, 1/r), B = 0, only A and B train (AdamW, finetune.py:188).

Device layout: one adapter per packed GEMM group of weights.py. Groups that fuse several nn.Linear (q‖k‖v, interleaved
gate/up) hold their members' adapters side by side — A_all [m·rp, K] stacks the members' A, B_all [N, m·rp] is block
structured (member j's rows only see columns j·rp …), and the off-block entries are kept at zero by masking their
gradients (bl_lora_block_mask_f32). The rank is zero-padded to rp = 64 (the GEMM kernels' K granularity); padded rows /
columns have zero gradients by construction and stay zero.

Forward of one linear (training/step.py::_lin): t = x·Aᵀ is written into spare columns of x's buffer and the layer is ONE
GEMM over K + R, y = bf16([x | t]·[W | s·B]ᵀ) — the rank-R update is accumulated in fp32 with the base product and rounded
once. PEFT under bf16 autocast rounds lora_B's output, its product with the scaling and the sum with the base result
separately; the two differ by at most one bf16 ulp of y, but the single rounding does not absorb updates that are below
half an ulp of the base output (right after initialisation, B ≈ 0, PEFT's order loses most of them). s·B is stored as
bf16(s·B) (exact for the reference's s = 0.5).
Backward: dt = dy·(s·B) into spare columns of dy's buffer, dx = [dy | dt]·[Wᵀ | Aᵀ]ᵀ as one GEMM; dB = (s·tᵀ·dy)ᵀ and
dA = dtᵀ·x through the small-output TN GEMM (bl_gemm_tn_small_bf16: dy / x read once, untransposed).
`lora_dropout` = p > 0 (round 4): t = dropout(x)·Aᵀ from a masked copy of x (bl_dropout_bf16: counter-based mask, recomputed in
the backward pass), dA = dtᵀ·dropout(x), and the fused input gradient dy·W + dt·A is corrected to dy·W + mask/(1-p) ⊙ (dt·A)
with u = dt·A from one more rank-R GEMM (bl_dropout_grad_fix_bf16). p = 0 plans are unchanged.

Inference under the adapters: merged weights (the reference deploys LoRA with `merge_and_unload()` into the bf16 base,
finetune.py:331-341). `merged_reference` is the definition, per packed group with logical [n, k] matrix W:
    sB      = bf16(fp32(s) · B_all)               the operand the learner multiplies by (be_pack(scale = s): fp32 product, one RNE)
    Δ[n,k]  = Σ_r sB[n,r] · A_all[r,k]            exact products, fp64 sum
    W'[n,k] = bf16_rne(W[n,k] + Δ[n,k])           ONE rounding;  W'[n,k] = W[n,k] (same bits) where Δ[n,k] == 0
  * B = 0 or s = 0 gives W' = W bit for bit (PEFT's initial state; the Δ == 0 rule also keeps a −0 of W).
  * An update below half a bf16 ulp of W is absorbed: inherent to merging, and the same as the reference's deployment — the
    learner's own forward (one rounding of the OUTPUT) still sees such an update, the merged model does not.
  * K-padding columns stay 0, because A's padding columns are 0.
`bl_lora_merge_bf16` (csrc/lora_merge.hip) computes it on the packed layout with Δ accumulated in fp32 on the MFMA and W + Δ
formed in fp32: identical where those sums are exact, else within the fp32 accumulation error of Δ plus a possible flip of
the final rounding next to a tie (tests/test_lora_merge_gpu.py states the bound). `adapted_weights()` is a second set of
packed weights beside the frozen base (`VLAWeights.adapted_view`), `refresh()` the ONE batched launch that rewrites it from
the live A / B; the base stays resident and untouched — an RL learner's reference policy.
`enable_fp8()` adds e4m3 copies of the adapted decoder-layer weights for the e4m3 prefill (`OpenVLAEngine(fp8=True)`); the
refresh then ends with one `bl_quantize_weight_fp8_packed_batched` launch (csrc/quantize_weight_fp8.hip) that rewrites them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..weights import Arena, PackedGroup, VLAWeights, _pack, _unpack

RP = 64          # padded rank
FP8_NAMES = ("qkv_w", "o_w", "gu_w", "down_w")     # the decoder-layer weights engine._fp8_layers keeps e4m3 copies of


@dataclass(eq=False)
class Adapter:
    group: PackedGroup
    modules: List[str]            # HF module paths of the fused members (without ".weight")
    mode: str                     # "single" | "concat" | "interleave"
    r: int
    A: torch.Tensor               # bf16 [m*RP, k] row-major (live compute copy, AdamW's bf16 output)
    B: torch.Tensor               # bf16 [n, m*RP]
    A_p: torch.Tensor             # packed
    B_p: torch.Tensor
    shapes: List[Tuple[int, int]] = field(default_factory=list)     # per member (out_features, in_features)
    index: int = 0

    @property
    def R(self) -> int:
        return self.A.shape[0]

    def member_rows(self, j: int) -> torch.Tensor:
        """Row indices of member j inside the group's logical [n, k] matrix."""
        m, out = len(self.modules), self.shapes[j][0]
        if self.mode == "interleave":
            return torch.arange(out) * m + j
        base = (self.group.n // m) * j if self.mode == "concat" else 0
        return torch.arange(out) + base


def bf16_rne_bits(x) -> np.ndarray:
    """fp64 → bf16 bit patterns (uint16) with ONE round-to-nearest-even (torch's double → bfloat16 goes through fp32: two
    roundings). Finite values inside the bf16 normal range."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert np.isfinite(x).all()
    as_f64 = lambda bits: bits.astype(np.uint32).view(np.float32).astype(np.float64)
    lo = np.ascontiguousarray(x.astype(np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)     # a bf16 value next to x …
    lo = np.where(np.abs(as_f64(lo)) > np.abs(x), lo - np.uint32(0x10000), lo).astype(np.uint32)   # … not above |x| (fp32 may round up)
    hi = (lo + np.uint32(0x10000)).astype(np.uint32)                                              # the next one away from zero
    d_lo, d_hi = np.abs(x - as_f64(lo)), np.abs(as_f64(hi) - x)                                  # both differences are exact
    up = (d_hi < d_lo) | ((d_hi == d_lo) & (((lo >> np.uint32(16)) & np.uint32(1)) == 1))
    return (np.where(up, hi, lo) >> np.uint32(16)).astype(np.uint16)


def merged_reference(W: torch.Tensor, A: torch.Tensor, B: torch.Tensor, s: float, exact: bool = False):
    """The definition of the merge for one group (module docstring): logical W [n, k], A_all [R, k], B_all [n, R] (bf16, any
    device) and s = alpha / r → W' bf16 [n, k] on the CPU; `exact=True` → (W', W + Δ in fp64, sB bf16)."""
    W, A, B = (t.detach().cpu() for t in (W, A, B))
    assert W.dtype == A.dtype == B.dtype == torch.bfloat16
    sB = (B.float() * float(np.float32(s))).to(torch.bfloat16)
    delta = sB.double() @ A.double()
    total = W.double() + delta
    bits = torch.from_numpy(bf16_rne_bits(total.numpy()).view(np.int16).copy())
    out = torch.where(delta == 0, W.contiguous().view(torch.int16), bits).view(torch.bfloat16)
    return (out, total, sB) if exact else out


class LoraAdapters:
    """All adapters of a model + their PEFT-named state dict."""

    def __init__(self, w: VLAWeights, r: int = 32, alpha: Optional[int] = None, seed: int = 0, dropout: float = 0.0):
        """`dropout` = PEFT's `lora_dropout` (finetune.py:101,177): in training the adapter branch sees nn.Dropout(p)(x). One mask
        per adapted GEMM and step: PEFT draws an independent mask for every module, here the modules fused into one GEMM
        (q / k / v; gate / up) share theirs — each module's own statistics are PEFT's, only the correlation between the
        fused modules' masks differs (training/step.py::_lin)."""
        if r > RP:
            raise ValueError(f"LoRA rank {r} exceeds the padded rank {RP}")
        if not (0.0 <= dropout < 1.0):
            raise ValueError(f"lora_dropout {dropout} outside [0, 1)")
        self.w, self.r, self.dropout = w, r, float(dropout)
        self.alpha = min(r, 16) if alpha is None else alpha
        self.scaling = self.alpha / r
        dev = w.embed.device
        specs = w._specs()
        self.adapters: List[Adapter] = []
        self.by_packed: Dict[int, Adapter] = {}
        z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
        for g in w.groups:
            first = g.members[0]
            if first == "language_model.lm_head.weight" or first.endswith("patch_embed.proj.weight"):
                continue                     # PEFT all-linear skips the output layer; the patch embedding is a Conv2d
            m = len(g.members)
            pl0 = w.placements[first]
            mode = "single" if m == 1 else ("interleave" if pl0.ld == m * pl0.cols else "concat")
            ad = Adapter(g, [n[:-len(".weight")] for n in g.members], mode, r, z(m * RP, g.k), z(g.n, m * RP),
                         z(m * RP // 16, g.k // 32, 64, 8), z(g.n // 16, m * RP // 32, 64, 8),
                         [tuple(specs[n].shape) for n in g.members])
            ad.index = len(self.adapters)
            self.adapters.append(ad)
            self.by_packed[g.packed.data_ptr()] = ad
        self._adapted: Optional[VLAWeights] = None       # adapted_weights(): built on first use
        self._refresh_ops: Optional[List[ops.Op]] = None
        self._plan_handed_out = False                    # refresh_ops() gave the plan to a caller who may keep a copy (TrainStep)
        self._fp8: Optional[List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]] = None   # enable_fp8(): the adapted view's e4m3 copies
        self._fp8_arena: Optional[Arena] = None
        self.init_gaussian(seed)

    def get(self, packed: torch.Tensor) -> Optional[Adapter]:
        return self.by_packed.get(packed.data_ptr())

    # ---- values ----
    def init_gaussian(self, seed: int = 0) -> "LoraAdapters":
        """PEFT init_lora_weights="gaussian": A ~ N(0, 1/r), B = 0."""
        gen = torch.Generator(device="cpu").manual_seed(seed)
        sd = {}
        for ad in self.adapters:
            for j, mod in enumerate(ad.modules):
                out, inp = ad.shapes[j]
                sd[f"base_model.model.{mod}.lora_A.weight"] = torch.randn(self.r, inp, generator=gen) / self.r
                sd[f"base_model.model.{mod}.lora_B.weight"] = torch.zeros(out, self.r)
        return self.load_state_dict(sd)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "LoraAdapters":
        for ad in self.adapters:
            A = torch.zeros(ad.A.shape, dtype=torch.float32)
            B = torch.zeros(ad.B.shape, dtype=torch.float32)
            for j, mod in enumerate(ad.modules):
                out, inp = ad.shapes[j]
                a, b = sd[f"base_model.model.{mod}.lora_A.weight"], sd[f"base_model.model.{mod}.lora_B.weight"]
                if tuple(a.shape) != (self.r, inp) or tuple(b.shape) != (out, self.r):
                    raise ValueError(f"{mod}: adapter shapes {tuple(a.shape)}, {tuple(b.shape)}")
                A[j * RP:j * RP + self.r, :inp] = a.float()
                B[ad.member_rows(j), j * RP:j * RP + self.r] = b.float()
            ad.A.copy_(A.to(torch.bfloat16))
            ad.B.copy_(B.to(torch.bfloat16))
        self.repack()
        return self

    def state_dict(self, masters: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """PEFT adapter-file names (`adapter_model`): base_model.model.<module>.lora_{A,B}.weight. `masters` (name →
        fp32 [m*RP, k] / [n, m*RP] from the ParamStore) replaces the live bf16 values when given."""
        out = {}
        for i, ad in enumerate(self.adapters):
            A = (masters[f"lora.{i}.A"] if masters else ad.A).float().cpu().view(ad.A.shape)
            B = (masters[f"lora.{i}.B"] if masters else ad.B).float().cpu().view(ad.B.shape)
            for j, mod in enumerate(ad.modules):
                o, inp = ad.shapes[j]
                out[f"base_model.model.{mod}.lora_A.weight"] = A[j * RP:j * RP + self.r, :inp].clone()
                out[f"base_model.model.{mod}.lora_B.weight"] = B[ad.member_rows(j), j * RP:j * RP + self.r].clone()
        return out

    def repack(self) -> None:
        for ad in self.adapters:
            _pack(ad.A, ad.A_p)
            _pack(ad.B, ad.B_p)

    def plain_units(self) -> List[Tuple[str, torch.Tensor, bool, str]]:
        """(name, live bf16 tensor, weight-decayed, bucket) for the ParamStore: finetune.py:188 builds one AdamW group
        (torch default weight_decay 0.01 on every adapter tensor)."""
        from .sharding import bucket_key
        out = []
        for i, ad in enumerate(self.adapters):
            bk = "lora." + bucket_key(ad.group.members[0])
            out.append((f"lora.{i}.A", ad.A.view(-1), True, bk))
            out.append((f"lora.{i}.B", ad.B.view(-1), True, bk))
        return out

    def n_params(self) -> int:
        return sum(self.r * (o + i) for ad in self.adapters for (o, i) in ad.shapes)

    def merged_state_dict(self) -> Dict[str, torch.Tensor]:
        """`merge_and_unload()` (finetune.py:331-341): HF-named base weights with W += scaling · B·A (export glue)."""
        sd = self.w.state_dict()
        ad_sd = self.state_dict()
        for ad in self.adapters:
            for mod in ad.modules:
                a = ad_sd[f"base_model.model.{mod}.lora_A.weight"].to(sd[mod + ".weight"].device)
                b = ad_sd[f"base_model.model.{mod}.lora_B.weight"].to(a.device)
                wt = sd[mod + ".weight"]
                sd[mod + ".weight"] = (wt.float() + self.scaling * (b @ a)).to(wt.dtype)
        return sd

    # ---- inference under the adapters: merged weights beside the frozen base (module docstring) ----
    def merged_reference(self, ad: Adapter) -> torch.Tensor:
        """W' bf16 [n, k] (CPU) of one adapter's group from the live A / B: the specification `refresh()` is tested against."""
        return merged_reference(_unpack(ad.group.packed), ad.A, ad.B, self.scaling)

    def adapted_weights(self) -> VLAWeights:
        """`self.w.adapted_view(<every adapted group>)`, built once: the weights of the model WITH the adapters. They hold
        copies of the base until the first `refresh()`."""
        if self._adapted is None:
            self._adapted = self.w.adapted_view([ad.group for ad in self.adapters])
        return self._adapted

    # ---- e4m3 prefill under the adapters: the adapted view's e4m3 copies, requantised with every refresh ----
    @property
    def fp8_enabled(self) -> bool:
        return self._fp8 is not None

    def enable_fp8(self) -> "LoraAdapters":
        """Give `adapted_weights()` e4m3 copies (+ per-channel scales) of every decoder layer's qkv_w / o_w / gu_w / down_w, in
        one Arena, installed as that view's `_fp8_layers` cache in the shape engine._fp8_layers returns ([{name:
        ops.Fp8Weight}] per layer), so `OpenVLAEngine(adapted, fp8=True)` reads them unchanged. They are filled here once and
        from then on rewritten IN PLACE by every refresh: `refresh_ops()` becomes the merge launch followed by ONE
        `bl_quantize_weight_fp8_packed_batched` launch (csrc/quantize_weight_fp8.hip: the kernels' quantiser specification —
        not bit-identical to the base model's load-time ops.quantize_weight_fp8, which divides by the scale).
        Call it BEFORE a `TrainStep(..., lora=self, refresh_adapted=True)` is built: the step copies `refresh_ops()`, and a
        copy made earlier would keep refreshing the bf16 weights only — so enabling after `refresh_ops()` has handed the
        plan out raises RuntimeError. llm_dim and llm_inter must be multiples of 128 (bl_gemm_fp8's K), else ValueError."""
        if self._fp8 is not None:
            return self
        if self._plan_handed_out:
            raise RuntimeError("enable_fp8() after refresh_ops() was handed out (a TrainStep(refresh_adapted=True) holds a copy that "
                               "refreshes the bf16 weights only): enable fp8 before building the step")
        d = self.w.dims
        if d.llm_dim % 128 or d.llm_inter % 128:
            raise ValueError("fp8 prefill needs llm_dim and llm_inter to be multiples of 128")
        view = self.adapted_weights()
        arena = Arena(self.w.embed.device)
        slots = []
        for lw in view.layers:
            row = {}
            for name in FP8_NAMES:
                wp = getattr(lw, name)
                n, k = wp.shape[0] * 16, wp.shape[1] * 32
                row[name] = (arena.reserve((n // 16, k // 64, 64, 8)), arena.reserve((2 * n,)))      # fp32 [n] as 2n bf16 slots
            slots.append(row)
        arena.commit()
        self._fp8 = [{name: ops.Fp8Weight(arena.view(a), arena.view(b).view(torch.float32)) for name, (a, b) in row.items()}
                     for row in slots]
        self._fp8_arena = arena
        view.__dict__["_fp8_layers"] = self._fp8
        self._refresh_ops = None                         # rebuilt with the quantise launch
        if self.w.embed.is_cuda:                         # a CPU-allocated model (layout tests) runs no kernel
            ops.run_all(self._plan()[1:])
        return self

    def _plan(self) -> List[ops.Op]:
        from .. import train_ops as T
        view = self.adapted_weights()
        if self._refresh_ops is None:
            index = {id(g): i for i, g in enumerate(self.w.groups)}
            dev = self.w.embed.device
            entries = [T.be_lora_merge(ad.group.packed, ad.A, ad.B, self.scaling, view.groups[index[id(ad.group)]].packed, RP,
                                       len(ad.modules), ad.mode == "interleave") for ad in self.adapters]
            plan = [T.lora_merge_batched(entries, dev, run=False)]
            if self._fp8 is not None:
                plan.append(T.quantize_packed_batched([T.be_quantize_packed(getattr(lw, name), *row[name])
                                                       for lw, row in zip(view.layers, self._fp8) for name in FP8_NAMES], dev, run=False))
            self._refresh_ops = plan
        return self._refresh_ops

    def refresh_ops(self) -> List[ops.Op]:
        """The prepared refresh (replayable, graph-capturable): ONE `bl_lora_merge_batched_bf16` launch over all adapted groups,
        followed — after `enable_fp8()` — by ONE `bl_quantize_weight_fp8_packed_batched` launch over the decoder layers' e4m3
        copies. A caller may keep the list (TrainStep does): from here on `enable_fp8()` raises."""
        plan = self._plan()
        self._plan_handed_out = True
        return plan

    def refresh(self) -> None:
        """Rewrite `adapted_weights()` from the live A / B and the frozen base: W' = bf16(W + bf16(s·B)·A) per group; after
        `enable_fp8()` also their e4m3 copies and scales.
        Ordering contract: this is an op on the CURRENT stream, ordered like any other launch there. Engines that read the
        adapted weights on that stream (`predict_action`, `sample_actions`, `score_actions`, `OpenVLAEngine`) see the new
        weights from their next run on; a `StaggeredDecodePipeline` has batches in flight across calls and must be
        `flush()`ed before the refresh. Captured engine graphs stay valid: the buffers are rewritten in place, no pointer
        changes. `TrainStep(..., lora=self, refresh_adapted=True)` runs it after every optimizer step."""
        ops.run_all(self._plan())
