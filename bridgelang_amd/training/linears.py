"""How one nn.Linear runs in the training step: forward, input gradient and weight gradient, in bf16, on the e4m3 MFMA path
or under a LoRA adapter, and the layouts of its weight that those GEMMs read (DESIGN.md "Training step")."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .. import ops, train_ops as T
from ..ops import (EPI_BIAS, EPI_BIAS_GELU_KEEP, EPI_F32, EPI_GELU_BWD, EPI_NONE, EPI_SWIGLU_BWD, EPI_SWIGLU_KEEP, Fp8Weight, Op)
from ..weights import VLAWeights, _unpack
from .param_store import ParamStore, Unit

# SwiGLU / GELU forward ("f") and backward ("b") as GEMM epilogues (BL_EPI_*_KEEP / BL_EPI_*_BWD) instead of separate
# elementwise passes. ON by default since the tile GEMMs' whole-tile epilogue (round 4, gemm_common.h::epilogue_tile): same box,
# alternating runs at 7B, B = 32: separate passes 409.8 ms / step, forward fused 408.7, backward fused 409.0, both 406.6. With the
# per-store epilogue of rounds 1-3 the fused forms LOST 2-4 ms (442.2 vs 444.5-446.2): one workgroup per CU, so the extra
# stores / exp / erf sat exposed in an epilogue that already cost more than the HBM-bound pass they remove.
# BL_TRAIN_FUSED_ACT=0 (or any string without "f" / "b") selects the separate passes. Bit-identical either way (tested).
_FA = os.environ.get("BL_TRAIN_FUSED_ACT", "fb")
UNFUSED_FWD, UNFUSED_BWD = "f" not in _FA, "b" not in _FA


def transposed_pack(packed: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Packed [n, k] weight → packed [k, n] (the dgrad operand)."""
    rm = _unpack(packed).contiguous()
    t = torch.empty(k, n, dtype=torch.bfloat16, device=packed.device)
    T.transpose_pad(rm, t, n)
    return ops.pack_weight(t)


@dataclass
class ScratchSet:
    """The scratch that ops bind when they are planned. Plans that run side by side need a set each."""
    ws: torch.Tensor                    # split-K workspace of the GEMMs
    col_ws: torch.Tensor                # partials of the column sums (bias / LayerScale gradients)
    norm_ws: torch.Tensor               # partials of the norm-weight gradients
    tn_ws: Optional[torch.Tensor]       # partials of the small-output TN GEMM (adapter gradients)

    def like(self) -> "ScratchSet":
        return ScratchSet(*(None if t is None else torch.empty_like(t) for t in (self.ws, self.col_ws, self.norm_ws, self.tn_ws)))


@dataclass
class Scratch:
    main: ScratchSet
    side: ScratchSet                    # the second vision tower's: its own when its plans run on a stream of their own, else `main`


@dataclass
class Adapted:
    """A linear under a LoRA adapter: the K-concatenated weights its single forward / dgrad GEMMs read."""
    ad: object                          # training.lora.Adapter
    Wext: torch.Tensor                  # packed [W | s·B]
    WText: torch.Tensor                 # packed [Wᵀ | Aᵀ]
    BsT: torch.Tensor                   # packed (s·B)ᵀ: the dt = dy·(sB) operand
    ATp: Optional[torch.Tensor] = None  # packed Aᵀ [k, R]: the u = dt·A operand (lora_dropout > 0)
    t: Optional[torch.Tensor] = None    # saved t = x·Aᵀ: set when the forward is planned


@dataclass
class Linear:
    """One nn.Linear's weight and whichever other layouts of it the step keeps."""
    packed: torch.Tensor
    wT: Optional[torch.Tensor] = None                       # transposed packed copy for dgrad
    w8: Optional[Tuple[Fp8Weight, Fp8Weight]] = None        # e4m3 (forward, dgrad) copies
    lora: Optional[Adapted] = None


class Linears:
    """The linears of one training step: one `Linear` record per weight, found by the packed weight's address, and the
    buffers that only their GEMMs use. The step owns the activations (and the `wide` map of those with spare adapter
    columns) and hands every planner call the `ScratchSet` its ops bind."""

    def __init__(self, w: VLAWeights, store: ParamStore, lora, B: int, Tn: int, wide: Dict[int, torch.Tensor], *,
                 fp8: bool, fp8_wgrad: bool, shard_params: bool):
        self.w, self.dims, self.store, self.lora, self.B, self.T = w, w.dims, store, lora, B, Tn
        self.device = w.embed.device
        self.fp8_wgrad, self.shard_params = fp8_wgrad, shard_params
        self.fp8_wgrad_gemms = [0, 0]          # planned weight-gradient GEMMs [on the e4m3 path, fallen back to bf16]
        self.pools = None                      # the step's UnitPools, when parameters are sharded
        self._wide = wide
        self._recs: Dict[int, Linear] = {}     # packed.data_ptr() → record
        self.adapter_ops: List[Op] = []        # refresh of the adapter parts (repack plan)

    def rec(self, packed: torch.Tensor) -> Linear:
        return self._recs.setdefault(packed.data_ptr(), Linear(packed))

    def allocate(self, n_t: int, fp8: bool, refresh_adapted: bool) -> None:
        """Everything here that takes device memory, after the step's activations: the token-padded transposed operands of
        the round-1 weight-gradient form (`n_t` elements each), the e4m3 state, the extended weights of the adapters."""
        self.tA, self.tB, self.tBp = (torch.zeros(n_t, dtype=torch.bfloat16, device=self.device) for _ in range(3))
        if fp8:
            self._setup_fp8()
        if self.lora is not None:
            self._build_extended_weights()
            if refresh_adapted:                 # after the adapter refresh in the re-pack plan: reads the written-back A / B
                plan = self.lora.refresh_ops()  # the merge launch; after lora.enable_fp8() also the e4m3 requantisation
                self.adapter_ops = self.adapter_ops + plan
                ops.run_all(plan)

    # ---- fp8 (e4m3) forward / dgrad GEMMs of the decoder layers ------------------------------------------------------
    def _setup_fp8(self) -> None:
        d, dev, Tn = self.dims, self.device, self.T
        D, I = d.llm_dim, d.llm_inter
        u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=dev)
        self._q8 = {D: u8(Tn, D), I: u8(Tn, I)}                          # quantised GEMM inputs (one linear at a time)
        self._q8_dy = u8(Tn, max(3 * D, 2 * I))                          # quantised output gradients
        self._sx, self._sdy = (torch.zeros(Tn, dtype=torch.float32, device=dev) for _ in range(2))
        if self.fp8_wgrad:                     # token-contiguous (transposed) operands of the e4m3 weight-gradient GEMM
            Tq = (Tn + 127) // 128 * 128       # its contraction length: tokens, padded with zero columns to the MFMA's K = 128
            nmx = max(3 * D, 2 * I)
            self._Tq = Tq
            self._wg_qA = u8(nmx * Tq)                                                 # dyᵀ codes [N, Tq] row-major
            self._wg_pB = u8(I * Tq)                                                   # xᵀ codes [K, Tq] in the fragment-major packing
            self._wg_sA = torch.zeros(nmx, dtype=torch.float32, device=dev)
            self._wg_sB = torch.zeros(I, dtype=torch.float32, device=dev)
            self._wg_amax = torch.zeros(nmx + I, dtype=torch.float32, device=dev)      # column |max| of dy (first N) and x (next K)
        self.fp8_scratch()
        if self.shard_params:                  # sharded layers are quantised in their gather (slots carry the e4m3 copies)
            return
        for _, _, gi, _ in self.w.unit_fields("layers"):
            g = self.w.groups[gi]
            rm = ops.unpack_weight(g.packed).contiguous()                # start-up only; later the optimizer's bf16 copy
            ops.run_all(self.fp8_weight_ops(rm, g.packed))
            del rm

    def fp8_scratch(self) -> None:
        if not hasattr(self, "_q_tmp"):
            D, I = self.dims.llm_dim, self.dims.llm_inter
            nmax = max(3 * D * D, 2 * I * D)
            self._q_tmp = torch.zeros(nmax, dtype=torch.uint8, device=self.device)
            self._t_tmp = torch.zeros(nmax, dtype=torch.bfloat16, device=self.device)

    def fp8_weight_ops(self, rm: torch.Tensor, packed: torch.Tensor) -> List[Op]:
        """Logical bf16 weight [n, k] → the e4m3 copies of `packed`'s record (made on first use): the forward copy (scale per
        output channel n) and the transposed copy for dgrad (scale per input channel k), both in the fragment-major packing
        bl_gemm_fp8 reads."""
        n, k = rm.shape
        r = self.rec(packed)
        if r.w8 is None:
            one = lambda rows, cols: Fp8Weight(torch.zeros(rows // 16, cols // 64, 64, 8, dtype=torch.bfloat16, device=self.device),
                                               torch.zeros(rows, dtype=torch.float32, device=self.device))
            r.w8 = (one(n, k), one(k, n))
        q = self._q_tmp[:n * k].view(n, k)
        qT = self._q_tmp[:n * k].view(k, n)
        t = self._t_tmp[:n * k].view(k, n)
        as_pairs = lambda c: c.view(torch.bfloat16)                    # e4m3 codes as 2-byte units: [r, c] → [r, c / 2]
        fwd, bwd = r.w8
        return [ops.quantize_rows_fp8(rm, q, fwd.scale, run=False)[2], T.pack(as_pairs(q), fwd.w8, run=False),
                T.transpose_pad(rm, t, n, run=False), ops.quantize_rows_fp8(t, qT, bwd.scale, run=False)[2],
                T.pack(as_pairs(qT), bwd.w8, run=False)]

    def unit_of(self, packed: torch.Tensor) -> Optional[Unit]:
        u = self.pools.unit_of(packed) if self.pools is not None else None      # slot views are shared by the units of a pool
        return u if u is not None else self.store.unit_of_packed(packed)

    def gemm(self, sc: ScratchSet, *a, **k) -> Op:
        """Prepared GEMM with the split-K scratch: training has no batch-slot invariance to keep (engine.py keeps it
        off for inference), so ragged last rounds of K >= 8192 GEMMs are split along K."""
        return ops.gemm(*a, workspace=sc.ws, run=False, **k)

    def wT(self, packed: torch.Tensor) -> torch.Tensor:
        """[K, N]-packed transposed copy of a packed [N, K] weight (built on first use, refreshed by repack)."""
        t = self.pools.transposed(packed) if self.pools is not None else None
        if t is not None:
            return t
        r = self.rec(packed)
        if r.wT is None:
            n, k = packed.shape[0] * 16, packed.shape[1] * 32
            r.wT = transposed_pack(packed, n, k)
        return r.wT

    def dgrad(self, sc: ScratchSet, dy: torch.Tensor, packed: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_NONE, **kw) -> Op:
        return self.gemm(sc, dy, self.wT(packed), out, epilogue, **kw)

    def wgrad_into(self, sc: ScratchSet, dy: torch.Tensor, x: torch.Tensor, gview: torch.Tensor, fp8: bool = False) -> List[Op]:
        """gview[N, K] (fp32) = dyᵀ[N, T] · x[T, K]: the TN GEMM reads dy and x where they lie (transposing LDS reads);
        shapes with N % 8 or K % 8 take the round-1 form — the NT GEMM over token-padded transposed copies.
        fp8=True: the e4m3 form (TrainStep(fp8_wgrad=True)) — transpose, quantise per channel, NT GEMM on bl_gemm_fp8."""
        Tn, N = dy.shape
        K = x.shape[1]
        assert tuple(gview.shape) == (N, K), (dy.shape, x.shape, gview.shape)
        if fp8:
            Tq = self._Tq
            qA = self._wg_qA[:N * Tq].view(N, Tq)
            pB = self._wg_pB[:K * Tq].view(torch.bfloat16).view(K // 16, Tq // 64, 64, 8)
            sA, sB = self._wg_sA[:N], self._wg_sB[:K]
            # two passes per operand: column |max| (2 B read), then one transposing quantise(-and-pack) (2 B read, 1 B written)
            am = self._wg_amax[:N + K]
            return [T.fill_zero(am, run=False), T.colamax(dy, am[:N], run=False), T.colamax(x, am[N:], run=False),
                    T.transpose_quantize_fp8(dy, am[:N], self._wg_qA[:N * Tq], sA, Tq, False, run=False),
                    T.transpose_quantize_fp8(x, am[N:], self._wg_pB[:K * Tq], sB, Tq, True, run=False),
                    ops.gemm_fp8(qA, sA, pB, sB, gview, EPI_F32, run=False)]
        if N % 8 == 0 and K % 8 == 0:
            return [T.gemm_tn(dy, x, gview, workspace=sc.ws, run=False)]
        Tp = (Tn + 63) // 64 * 64
        assert max(N, K) * Tp <= self.tA.numel()
        tA = self.tA[:N * Tp].view(N, Tp)
        tB = self.tB[:K * Tp].view(K, Tp)
        tBp = self.tBp[:K * Tp].view(K // 16, Tp // 32, 64, 8)
        if K % 64 == 0:                        # one pass: transpose straight into the packed operand layout
            prep = [T.transpose_pack(x, tBp, Tp, run=False)]
        else:
            prep = [T.transpose_pad(x, tB, Tp, run=False), T.pack(tB, tBp, run=False)]
        return [T.transpose_pad(dy, tA, Tp, run=False)] + prep + [self.gemm(sc, tA, tBp, gview, EPI_F32, algo_nk=(K, Tn))]

    def wgrad(self, sc: ScratchSet, dy: torch.Tensor, x: torch.Tensor, packed: torch.Tensor) -> List[Op]:
        """Weight gradient of a base linear; [] when the weight is frozen."""
        u = self.unit_of(packed)
        if u is None:
            return []
        want = self.fp8_wgrad and self.rec(packed).w8 is not None
        fp8 = want and dy.shape[1] % 16 == 0 and x.shape[1] % 16 == 0
        if want:                               # how many weight-gradient GEMMs really run on the e4m3 path (bench.py reports it)
            self.fp8_wgrad_gemms[0 if fp8 else 1] += 1
            if not fp8 and self.fp8_wgrad_gemms[1] == 1:
                import warnings
                warnings.warn(f"fp8_wgrad: a weight gradient of shape [{dy.shape[1]}, {x.shape[1]}] is not a multiple of 16 in both "
                              "dimensions and stays on the bf16 TN GEMM")
        return self.wgrad_into(sc, dy, x, self.store.grad_view(u), fp8=fp8)

    def _build_extended_weights(self) -> None:
        """LoRA: K-concatenated packed weights [W | s·B] (forward) and [Wᵀ | Aᵀ] (dgrad) per adapted linear. The frozen
        part is copied once; the adapter columns are (re)written by `adapter_ops` after every optimizer step."""
        lora, s = self.lora, self.lora.scaling
        dev = self.device
        zb = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16, device=dev)
        entries = []
        if lora.dropout > 0.0:
            rows = max([self.T, self.B * 256] + [self.B * tw.dims.tokens for tw in (self.w.dino, self.w.siglip)])
            kmax = max(ad.group.k for ad in lora.adapters)
            self._xd, self._ud = zb(rows, kmax), zb(rows, kmax)            # dropout(x) and u = dt·A of ONE adapted linear at a time
            self.drop_seed = torch.zeros(1, dtype=torch.int32, device=dev)      # bumped once per forward pass
        for ad in lora.adapters:
            packed, n, k, R = ad.group.packed, ad.group.n, ad.group.k, ad.R
            KT, NT = (k + R) // 32, (n + R) // 32
            We, WTe = zb(n // 16, KT, 64, 8), zb(k // 16, NT, 64, 8)
            We.view(n // 16, KT, 512)[:, :k // 32].copy_(packed.view(n // 16, k // 32, 512))
            WTe.view(k // 16, NT, 512)[:, :n // 32].copy_(transposed_pack(packed, n, k).view(k // 16, n // 32, 512))
            BsT = zb(R // 16, n // 32, 64, 8)
            self.rec(packed).lora = a = Adapted(ad, We, WTe, BsT)
            # the adapter columns of the extended weights, from the live adapter tensors: [W | s·B], (s·B)ᵀ, A, [Wᵀ | Aᵀ] — table
            # entries of ONE bl_batched_ops launch for all adapters (rounds 1-3: five launches per adapter, 1 650 per step)
            entries += [T.be_pack(ad.B, We, KT, k // 32, scale=s), T.be_transpose_pack(ad.B, BsT, n, scale=s),
                        T.be_pack(ad.A, ad.A_p), T.be_transpose_pack(ad.A, WTe, R, NT, n // 32)]
            if lora.dropout > 0.0:
                a.ATp = zb(k // 16, R // 32, 64, 8)
                entries.append(T.be_transpose_pack(ad.A, a.ATp, R))
        self.adapter_ops = [T.batched(entries, dev, run=False)]
        ops.run_all(self.adapter_ops)

    def forward(self, sc: ScratchSet, x: torch.Tensor, packed: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_NONE,
                **kw) -> List[Op]:
        """Forward of one nn.Linear. With an adapter: t = x·Aᵀ into the spare columns of x's buffer, then ONE GEMM
        y = [x | t]·[W | s·B]ᵀ over K + R."""
        r = self.rec(packed)
        if r.w8 is not None:                               # decoder-layer linear on the e4m3 MFMA path
            return ops.linear_fp8(x, self._q8[x.shape[1]], self._sx, *r.w8[0], out, epilogue, **kw)
        if r.lora is None:
            return [self.gemm(sc, x, packed, out, epilogue, **kw)]
        a, ad = r.lora, r.lora.ad
        K, R = x.shape[1], ad.R
        wide = self._wide[x.data_ptr()]
        assert wide.shape[1] >= K + R, "input buffer of an adapted linear lacks the adapter columns"
        a.t = t = wide[:, K:K + R]
        pre: List[Op] = []
        xa = x
        if self.lora.dropout > 0.0:            # PEFT: lora_A(dropout(x)); the base product below still reads the un-masked x
            xa = self._xd[:x.shape[0], :K]
            pre = [T.dropout(x, xa, self.lora.dropout, self.drop_seed, ad.index, run=False)]
        return pre + [self.gemm(sc, xa, ad.A_p, t, EPI_NONE), self.gemm(sc, wide[:, :K + R], a.Wext, out, epilogue, **kw)]

    def backward(self, sc: ScratchSet, dy: torch.Tensor, x: torch.Tensor, packed: torch.Tensor, dx: Optional[torch.Tensor],
                 epilogue: int = EPI_NONE, **kw) -> List[Op]:
        """Backward of one nn.Linear given dy: base wgrad (if trainable) and dx = dy·W (if wanted); with an adapter:
        dt = dy·(sB) into the spare columns of dy's buffer, dB = (s·tᵀ·dy)ᵀ and dA = dtᵀ·x through the small-output TN
        GEMM (dy / x read once, untransposed), and dx = [dy | dt]·[Wᵀ | Aᵀ]ᵀ as ONE GEMM."""
        r = self.rec(packed)
        if r.lora is None:
            plan = self.wgrad(sc, dy, x, packed)
            if dx is not None and r.w8 is not None:        # dx = dy · W on the e4m3 path (dy per token row, Wᵀ per input channel)
                plan += ops.linear_fp8(dy, self._q8_dy[:, :dy.shape[1]], self._sdy, *r.w8[1], dx, EPI_NONE)
            elif dx is not None:
                plan.append(self.dgrad(sc, dy, packed, dx, epilogue, **kw))
            return plan
        a, ad = r.lora, r.lora.ad
        i, st, s, R, N = ad.index, self.store, self.lora.scaling, ad.R, dy.shape[1]
        wide = self._wide[dy.data_ptr()]
        assert wide.shape[1] >= N + R, "gradient buffer of an adapted linear lacks the adapter columns"
        dt = wide[:, N:N + R]
        gB = st.grad_view(f"lora.{i}.B").view(ad.group.n, R)
        gA = st.grad_view(f"lora.{i}.A").view(R, ad.group.k)
        plan = [self.gemm(sc, dy, a.BsT, dt, EPI_NONE), T.gemm_tn_small(a.t, dy, gB, True, sc.tn_ws, alpha=s, run=False)]
        if len(ad.modules) > 1:
            plan.append(T.lora_block_mask(gB, R // len(ad.modules), len(ad.modules), ad.mode == "interleave", run=False))
        p = self.lora.dropout
        xa = x
        if p > 0.0:                            # the mask of the forward pass, recomputed (same device seed, same salt)
            xa = self._xd[:x.shape[0], :x.shape[1]]
            plan.append(T.dropout(x, xa, p, self.drop_seed, ad.index, run=False))
        plan.append(T.gemm_tn_small(dt, xa, gA, False, sc.tn_ws, run=False))
        if dx is not None:
            plan.append(self.gemm(sc, wide[:, :N + R], a.WText, dx, epilogue, **kw))
            if p > 0.0:                        # dx = dy·W + dt·A so far; dropout's backward masks the adapter's share
                assert epilogue == EPI_NONE, "activation-backward epilogues are not combined with lora_dropout"
                u = self._ud[:x.shape[0], :x.shape[1]]
                plan += [self.gemm(sc, dt, a.ATp, u, EPI_NONE), T.dropout_grad_fix(u, dx, p, self.drop_seed, ad.index, run=False)]
        return plan

    def forward_act(self, sc: ScratchSet, x, packed, pre, act, kind: str, **kw) -> List[Op]:
        """Linear + activation of the training forward with the PRE-activation kept (autograd's saved tensor): one GEMM
        whose epilogue writes both (`kind` "swiglu": gate/up interleaved → silu(g)·u; "gelu": bias + exact-erf GELU). The
        e4m3 path and BL_TRAIN_FUSED_ACT=0 (see above) keep the plain epilogue + an elementwise pass; both forms
        give the same bits."""
        fused = not UNFUSED_FWD and self.rec(packed).w8 is None
        if kind == "swiglu":
            if fused:
                return self.forward(sc, x, packed, pre, EPI_SWIGLU_KEEP, out2=act, **kw)
            return self.forward(sc, x, packed, pre, EPI_NONE, **kw) + [T.swiglu(pre, act, run=False)]
        if fused:
            return self.forward(sc, x, packed, pre, EPI_BIAS_GELU_KEEP, out2=act, **kw)
        return self.forward(sc, x, packed, pre, EPI_BIAS, **kw) + [T.gelu(pre, act, run=False)]

    def backward_act(self, sc: ScratchSet, dy, x, packed, pre, dpre, dact, kind: str) -> List[Op]:
        """Backward of `act(pre)` → Linear(packed) given dy of the linear: the input-gradient GEMM's epilogue applies the
        activation's backward with the saved pre-activation, so d act never travels through HBM (dact is only used by the
        unfused forms: e4m3 dgrad and BL_TRAIN_FUSED_ACT=0)."""
        r = self.rec(packed)
        fused = not UNFUSED_BWD and r.w8 is None
        if r.lora is not None and self.lora.dropout > 0.0:
            fused = False       # dropout's backward adds the masked adapter share to d act BEFORE the activation's backward
        if not fused:
            bwd = T.swiglu_backward(pre, dact, dpre, run=False) if kind == "swiglu" else T.gelu_backward(pre, dact, dpre, run=False)
            return self.backward(sc, dy, x, packed, dact) + [bwd]
        return self.backward(sc, dy, x, packed, dpre, epilogue=EPI_SWIGLU_BWD if kind == "swiglu" else EPI_GELU_BWD, res=pre)

    def repack_ops(self, rm: torch.Tensor, packed: torch.Tensor, entries: list) -> List[Op]:
        """After AdamW wrote the logical matrix `rm` of `packed`: refresh the dgrad layout (an entry of the batched launch
        where its shape allows) and the e4m3 copies; returns the ops that are launches of their own."""
        plan: List[Op] = []
        n, k = rm.shape
        r = self.rec(packed)
        if r.wT is not None:                                  # only weights that a dgrad GEMM actually reads
            if k % 64 == 0 and n % 32 == 0:
                entries.append(T.be_transpose_pack(rm, r.wT, n))
            else:
                plan.append(T.transpose_pack(rm, r.wT, n, run=False))
        if r.w8 is not None:                                  # e4m3 copies follow the updated weight
            plan += self.fp8_weight_ops(rm, packed)
        return plan
