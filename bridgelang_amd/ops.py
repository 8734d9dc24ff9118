"""Thin torch-tensor front end over the C ABI (bridgelang_amd/_lib.py → libbridgelang_hip.so).

PyTorch is plumbing only: tensors give device memory and the current HIP stream; every arithmetic operation is a
hand-written gfx950 kernel behind `bl_*`. Each builder returns an `Op` (a prepared C call whose descriptor structs are
built once); `Op.run()` enqueues it on the current stream. The engine keeps lists of Ops and replays them (directly or
under HIP-graph capture), so steady-state host cost is one ctypes call per kernel.
"""
from __future__ import annotations

import functools
import math

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (AttnDesc, GemmDesc, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_KEEP, EPI_BIAS_RES, EPI_F32, EPI_F32_BF16R, EPI_GELU_BWD,
                   EPI_NONE, EPI_SWIGLU_BWD, EPI_SWIGLU_KEEP,
                   EPI_RES, EPI_SWIGLU)

__all__ = ["Op", "gemm", "gemm_last_form", "gemm_form_name", "gemm_fp8", "linear_fp8", "Fp8Weight", "quantize_rows_fp8", "quantize_weight_fp8", "quantize_packed_weight_fp8", "pack_weight", "unpack_weight", "cross_entropy", "layernorm", "rmsnorm", "rmsnorm_skinny", "skinny_rows_supported", "attention", "attention_rope", "attention_decode", "attention_decode_rope", "attention_decode_rope_grouped", "attention_decode_rope_shared", "repeat_rows", "attention_probs", "gather_rows", "skinny_supported", "rope_kvcache", "embed_splice",
           "argmax", "sample", "score", "beam_step", "cache_table", "beam_reorder_kv", "im2col_patch14", "preprocess_u8", "resample_coeffs", "resize_bicubic_u8", "resize_u8", "crop_resize_bilinear_u8", "augment_frames_u8", "write_prefix_tokens", "fill_synth", "run_all",
           "EPI_NONE", "EPI_BIAS", "EPI_BIAS_GELU", "EPI_BIAS_RES", "EPI_RES", "EPI_SWIGLU", "EPI_F32", "EPI_F32_BF16R",
           "EPI_SWIGLU_KEEP", "EPI_BIAS_GELU_KEEP", "EPI_SWIGLU_BWD", "EPI_GELU_BWD"]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _bf16(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.bfloat16 or not t.is_cuda:
        raise TypeError(f"{what}: expected a CUDA/HIP bfloat16 tensor, got {t.dtype} on {t.device}")
    return t


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{what}: expected a CUDA/HIP float32 tensor, got {t.dtype} on {t.device}")
    return t


def _contig_bf16(fn: str, *pairs) -> None:
    """Every (tensor, name) pair is a contiguous bf16 device tensor."""
    for t, n in pairs:
        if not _bf16(t, n).is_contiguous():
            raise ValueError(f"{fn}: {n} must be contiguous")


def _dev(t, dtype: torch.dtype, shape, what: str) -> torch.Tensor:
    """`t` is a contiguous device tensor of `dtype` and `shape`: a tuple (None = any extent) or an element count."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda and t.is_contiguous()
    if ok and isinstance(shape, int):
        ok = t.numel() == shape
    elif ok:
        ok = t.dim() == len(shape) and all(w is None or w == s for s, w in zip(t.shape, shape))
    if not ok:
        raise TypeError(f"{what} must be a contiguous CUDA/HIP {dtype} tensor {list(shape) if isinstance(shape, tuple) else [shape]}")
    return t


def _rows(t: torch.Tensor, what: str) -> int:
    """Leading dimension (elements) of a 2-D view whose last dim is contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what}: expected a 2-D tensor with contiguous last dim, got shape {tuple(t.shape)} "
                         f"stride {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


class Op:
    """A prepared call into libbridgelang_hip.so. Keeps its tensors alive."""
    __slots__ = ("name", "fn", "args", "keep", "flops", "bytes")

    def __init__(self, name: str, fn, args: tuple, keep: tuple, flops: float = 0.0, nbytes: float = 0.0):
        self.name, self.fn, self.args, self.keep = name, fn, args, keep
        self.flops, self.bytes = flops, nbytes   # ALGORITHMIC work of this launch (bench.py roofline accounting)

    def run(self, stream: Optional[int] = None) -> None:
        rc = self.fn(*self.args, stream if stream is not None else _stream())
        if rc != 0:
            _lib.check(rc, self.name)


def _op(name: str, args: tuple, keep: tuple, run: bool, nbytes: float = 0.0, flops: float = 0.0) -> Op:
    op = Op(name, getattr(_lib.load(), name), args, keep, flops=flops, nbytes=nbytes)
    if run:
        op.run()
    return op


def glue(name: str, fn, keep: tuple = ()) -> Op:
    """A host-side index/copy step (torch data movement on the current stream, no arithmetic) wrapped as an Op so it can
    sit inside an op plan; `fn()` runs when the plan reaches it."""
    def call(stream):
        fn()
        return 0
    return Op(name, call, (), tuple(keep))


def run_all(ops: Sequence[Op]) -> None:
    s = _stream()
    for op in ops:
        rc = op.fn(*op.args, s)
        if rc != 0:
            _lib.check(rc, op.name)


# ---------------------------------------------------------------------------------------------------------------
def pack_weight(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Linear-layout weight [N, K] (last dim contiguous) → fragment-major [N/16, K/32, 64, 8] (bl_pack_weight_bf16).
    N % 16 == 0 and K % 32 == 0 (zero-pad first). Done once at load time."""
    _bf16(w, "w")
    N, K = w.shape
    if out is None:
        out = torch.empty(N // 16, K // 32, 64, 8, dtype=torch.bfloat16, device=w.device)
    _op("bl_pack_weight_bf16", (w.data_ptr(), _rows(w, "w"), N, K, _bf16(out, "out").data_ptr()), (w, out), True)
    return out


def unpack_weight(wp: torch.Tensor) -> torch.Tensor:
    """Inverse of pack_weight (torch glue; used only when exporting a state dict)."""
    nt, ks = wp.shape[0], wp.shape[1]
    return wp.view(nt, ks, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(nt * 16, ks * 32)


SKINNY_K = (512, 1024, 1536, 4096, 5120, 11008, 13824)
_SKINNY_EPI = (EPI_NONE, EPI_RES, EPI_SWIGLU, EPI_F32, EPI_F32_BF16R)


def skinny_supported(M: int, K: int, epilogue: int) -> bool:
    """Shapes the weight-streaming kernel is instantiated for (gemm_plan.h::BL_SKINNY_TABLE)."""
    return M <= 16 and K in SKINNY_K and epilogue in _SKINNY_EPI


def skinny_rows_supported(M: int, K: int, epilogue: int) -> bool:
    """Shapes bl_gemm_skinny_rows_bf16 takes: up to 128 stacked rows in the skinny kernel's summation order."""
    return M <= 128 and K in SKINNY_K and epilogue in _SKINNY_EPI


def _gemm_desc(A, lda, W, out, M, N, K, epilogue, bias, scale, res, res_row_mod, out_map, keep):
    """The bl_gemm_desc of gemm / gemm_fp8 and the tensors it points to, after those already in `keep`."""
    d = GemmDesc()
    d.A, d.lda = A.data_ptr(), lda
    d.W, d.ldw = W.data_ptr(), K
    d.C, d.ldc = out.data_ptr(), _rows(out, "out")
    d.M, d.N, d.K, d.epilogue = M, N, K, epilogue
    if bias is not None:
        d.bias = _bf16(bias, "bias").data_ptr(); keep.append(bias)
    if scale is not None:
        d.scale = _bf16(scale, "scale").data_ptr(); keep.append(scale)
    if res is not None:
        d.res, d.ldres = _bf16(res, "res").data_ptr(), _rows(res, "res"); keep.append(res)
    d.res_row_mod = res_row_mod
    if out_map is not None:
        d.out_group, d.out_stride, d.out_offset = out_map
    return d, keep


def gemm(A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_NONE, *,
         bias: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, res_row_mod: int = 0,
         out_map: Optional[Tuple[int, int, int]] = None,
         skinny: Optional[bool] = None, algo_nk: Optional[Tuple[int, int]] = None,
         a_norm: Optional[Tuple[torch.Tensor, float]] = None, workspace: Optional[torch.Tensor] = None,
         skinny_rows: bool = False, out2: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    """out = epilogue(A @ W.T).  A [M,K] row-major activations; W = PACKED weight [N/16, K/32, 64, 8] (pack_weight);
    out [rows, N] (N/2 for SWIGLU, 2N for SWIGLU_BWD; fp32 for F32*).

    Training forms: EPI_SWIGLU_KEEP / EPI_BIAS_GELU_KEEP write the pre-activation to `out` and the activation to `out2`
    ([rows, N/2] / [rows, N]); EPI_SWIGLU_BWD / EPI_GELU_BWD apply the activation's backward to the product, reading the
    saved pre-activation through `res` ([rows, 2N] gate/up pairs / [rows, N]).

    `out_map=(group, stride, offset)` remaps output rows (see bl_gemm_desc).
    `skinny=None` picks the weight-streaming kernel automatically for M <= 16 when it supports K.
    `algo_nk=(N, K)` gives the un-padded logical sizes for FLOP accounting when N or K carry zero padding.
    `a_norm=(weight, eps)` fuses HF LlamaRMSNorm on the rows of A (skinny kernel only: M <= 16).
    `workspace`: optional scratch tensor (>= 64 MiB) enabling the split-K tail of the 256x256 kernel.
    `skinny_rows=True`: bl_gemm_skinny_rows_bf16 — up to 128 rows in the skinny kernel's arithmetic (row results
    bit-identical to the M <= 16 kernel; the merged decode iteration of StaggeredDecodePipeline).
    """
    _bf16(A, "A"); _bf16(W, "W")
    if W.dim() != 4 or W.shape[2:] != (64, 8) or not W.is_contiguous():
        raise ValueError(f"gemm: W must be a packed weight [N/16, K/32, 64, 8] (ops.pack_weight), got {tuple(W.shape)}")
    M, K = A.shape
    N, Kw = W.shape[0] * 16, W.shape[1] * 32
    if Kw != K:
        raise ValueError(f"gemm: K mismatch A{tuple(A.shape)} W(packed) K={Kw}")
    want = torch.float32 if epilogue in (EPI_F32, EPI_F32_BF16R) else torch.bfloat16
    if out.dtype != want or not out.is_cuda:
        raise TypeError(f"gemm: out must be {want} on device")
    d, keep = _gemm_desc(A, _rows(A, "A"), W, out, M, N, K, epilogue, bias, scale, res, res_row_mod, out_map, [A, W, out])
    if epilogue in (EPI_SWIGLU_KEEP, EPI_BIAS_GELU_KEEP):
        if out2 is None:
            raise ValueError("gemm: the *_KEEP epilogues need out2")
        n2 = N // 2 if epilogue == EPI_SWIGLU_KEEP else N
        if out2.shape[1] < n2 or out2.shape[0] < M:
            raise ValueError(f"gemm: out2 {tuple(out2.shape)} too small for [{M}, {n2}]")
        d.C2, d.ldc2 = _bf16(out2, "out2").data_ptr(), _rows(out2, "out2"); keep.append(out2)
    elif out2 is not None:
        raise ValueError("gemm: out2 only with the *_KEEP epilogues")
    if epilogue in (EPI_SWIGLU_BWD, EPI_GELU_BWD) and (res is None or res.shape[0] < M or
                                                       res.shape[1] < (2 * N if epilogue == EPI_SWIGLU_BWD else N)):
        raise ValueError("gemm: the *_BWD epilogues read the saved pre-activation through res")
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        keep.append(workspace)
    n_out = N // 2 if epilogue == EPI_SWIGLU else 2 * N if epilogue == EPI_SWIGLU_BWD else N
    if out.shape[1] < n_out:
        raise ValueError(f"gemm: out has {out.shape[1]} columns, needs {n_out}")
    if out_map is None and out.shape[0] < M:
        raise ValueError(f"gemm: out has {out.shape[0]} rows, needs {M}")
    use_skinny = skinny
    if use_skinny is None:
        use_skinny = skinny_supported(M, K, epilogue)
    if a_norm is not None:
        if not use_skinny:
            raise ValueError("gemm: a_norm (fused RMSNorm) needs the skinny kernel (M <= 16 and a supported K)")
        d.a_norm_weight, d.a_norm_eps = _bf16(a_norm[0], "a_norm weight").data_ptr(), float(a_norm[1])
        keep.append(a_norm[0])
    if skinny_rows:
        if not skinny_rows_supported(M, K, epilogue) or a_norm is not None or out_map is not None:
            raise ValueError(f"gemm: skinny_rows needs M <= 128, K in {SKINNY_K}, no a_norm / out_map (M={M}, K={K})")
        name = "bl_gemm_skinny_rows_bf16"
    else:
        name = "bl_gemm_skinny_bf16" if use_skinny else "bl_gemm_bf16"
    # algorithmic work: logical FLOPs; bytes = each operand once + the output once
    esz = 4 if epilogue in (EPI_F32, EPI_F32_BF16R) else 2
    return _op(name, (C.byref(d),), (d, *keep), run,
               flops=2.0 * M * (algo_nk[0] if algo_nk else N) * (algo_nk[1] if algo_nk else K),
               nbytes=2.0 * (M * K + N * K) + esz * M * n_out)


_GF_TAIL = {0: "", 1: "+tail64x64", 2: "+tail128x64", 3: "+tail128x128"}


def gemm_form_name(code: int) -> str:
    """Name of a bl_gemm_last_form code (csrc/gemm_plan.h): the main kernel with its template form and K slices, then
    the tail treatment — e.g. "gemm128", "mid<4,4>/S8", "mid2<2,2>", "gemm256s_persistent+tail64x64",
    "gemm256s+splitk4", "rows_stream<8,4>+tree", "rows_mid<SK=2>+tree", "skinny<KS=43>", "tn+splitk2", "gemm256s_fp8"."""
    kind, a, b, S = code & 0xFF, (code >> 8) & 0xF, (code >> 12) & 0xF, (code >> 16) & 0x3F
    tail, tail_s = (code >> 22) & 0x7, (code >> 25) & 0x1F
    if kind == 0:
        return "none"
    sl = f"/S{S}" if S > 1 else ""
    main = {1: "gemm128", 2: "ring160x128", 3: f"ring128x128{sl}", 4: f"mid<{a},{b}>{sl}",
            5: f"mid2<{a},{b}>" if b else f"mid2<{a}>", 6: "gemm288s", 7: "gemm256s", 8: "gemm256s_persistent",
            10: f"rows_stream<{a},{b}>" + ("+tree" if b == 4 else ""), 11: f"rows_mid<SK={b}>" + ("+tree" if b == 2 else ""),
            12: f"skinny<KS={S}>" + ("+norm" if a else ""), 13: "tn", 14: "tn_persistent", 15: "tn_all_split", 16: "gemm256s_fp8"}.get(kind)
    if main is None:
        raise ValueError(f"gemm_form_name: unknown form code {code:#x}")
    return main + (f"+splitk{tail_s}" if tail == 4 else _GF_TAIL[tail])


def gemm_last_form() -> str:
    """The kernel form the calling thread's last GEMM launch took (bl_gemm_bf16, bl_gemm_skinny_bf16,
    bl_gemm_skinny_rows_bf16, bl_gemm_tn_bf16, bl_gemm_fp8), by name: a host-side record for tests, no part of dispatch."""
    return gemm_form_name(_lib.load().bl_gemm_last_form())


# ---- FP8 (e4m3) GEMM family — BASELINE configs[4]; no reference counterpart -----------------------------------------
FP8_MAX = 448.0
FP8_AMAX_MIN = 2.0 ** -100     # a row whose amax lies below this is quantised as a zero row (csrc/gemm_fp8.hip)


def quantize_weight_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """nn.Linear weight [N, K] (bf16, N % 16 == 0, K % 128 == 0) → (packed e4m3 weight, fp32 scale [N]): per output
    channel scale = amax / 448 (1 for a channel with amax < 2^-100, whose codes are all zero: the kernels' zero-row rule),
    RNE cast, then the fragment-major packing of pack_weight on the bytes viewed as bf16 pairs (bl_gemm_fp8 reads the
    same byte layout as bl_gemm_bf16). Load-time work, torch ops."""
    N, K = w.shape
    if N % 16 or K % 128:
        raise ValueError("quantize_weight_fp8: N % 16 == 0 and K % 128 == 0")
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax >= FP8_AMAX_MIN, amax / FP8_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn)
    packed = pack_weight(q.view(torch.uint8).view(N, K // 2, 2).view(torch.bfloat16).reshape(N, K // 2).contiguous())
    return packed, scale.contiguous()


def quantize_packed_weight_fp8(wp: torch.Tensor, w8: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                               run: bool = True):
    """Packed bf16 weight [N/16, K/32, 64, 8] (pack_weight; K % 128 == 0) → (packed e4m3 weight as bf16 [N/16, K/64, 64, 8], fp32
    scale [N]) in the shapes quantize_weight_fp8 returns, on the device and without a row-major copy
    (bl_quantize_weight_fp8_packed): the kernels' quantiser specification per output channel — it multiplies by
    fl32(448 / amax) where quantize_weight_fp8 divides by the scale, so a few codes per 10^5 differ between the two; the
    scales are equal. Writes every byte of w8 / scale in place (replayable; captured graphs that read them stay valid).
    Returns (w8, scale, op)."""
    _bf16(wp, "wp")
    if wp.dim() != 4 or wp.shape[2:] != (64, 8) or not wp.is_contiguous():
        raise ValueError("quantize_packed_weight_fp8: wp must come from pack_weight")
    N, K = wp.shape[0] * 16, wp.shape[1] * 32
    if N == 0 or K == 0 or K % 128:
        raise ValueError("quantize_packed_weight_fp8: N % 16 == 0 and K % 128 == 0")
    if w8 is None:
        w8 = torch.empty(N // 16, K // 64, 64, 8, dtype=torch.bfloat16, device=wp.device)
    if scale is None:
        scale = torch.empty(N, dtype=torch.float32, device=wp.device)
    if not w8.is_contiguous() or w8.numel() * w8.element_size() != N * K or not w8.is_cuda:
        raise ValueError(f"quantize_packed_weight_fp8: w8 must hold the {N * K} bytes of [N/16, K/64, 64, 16]")
    if scale.dtype != torch.float32 or scale.numel() != N or not scale.is_contiguous() or not scale.is_cuda:
        raise ValueError(f"quantize_packed_weight_fp8: scale fp32 [{N}]")
    return w8, scale, _op("bl_quantize_weight_fp8_packed", (wp.data_ptr(), N, K, w8.data_ptr(), scale.data_ptr()),
                          (wp, w8, scale), run, nbytes=3.0 * N * K)


def quantize_rows_fp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
                      run: bool = True):
    """Activations bf16 [rows, cols] → (e4m3 codes uint8 [rows, cols], fp32 scale per row = amax / 448)
    (bl_quantize_rows_fp8). Returns (q, scales, op)."""
    _bf16(x, "x")
    rows, cols = x.shape
    if q is None:
        q = torch.empty(rows, cols, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(rows, dtype=torch.float32, device=x.device)
    return q, scales, _op("bl_quantize_rows_fp8", (x.data_ptr(), _rows(x, "x"), rows, cols, q.data_ptr(), q.stride(0),
                                                   scales.data_ptr()), (x, q, scales), run, nbytes=3.0 * rows * cols)


def gemm_fp8(A8: torch.Tensor, scale_a: torch.Tensor, W8: torch.Tensor, scale_w: torch.Tensor, out: torch.Tensor,
             epilogue: int = EPI_NONE, *, bias: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
             res: Optional[torch.Tensor] = None, res_row_mod: int = 0, out_map: Optional[Tuple[int, int, int]] = None,
             run: bool = True) -> Op:
    """out = epilogue(scale_a[m] · scale_w[n] · (A8 @ W8.T)) on the fp8 MFMA path (bl_gemm_fp8). A8 uint8 e4m3 codes
    [M, K]; W8 = quantize_weight_fp8(...)[0]. `scale` (LayerScale, EPI_BIAS_RES), `res_row_mod` and `out_map` as in gemm."""
    if A8.dtype != torch.uint8 or not A8.is_cuda or A8.stride(1) != 1:
        raise TypeError("gemm_fp8: A8 must be a CUDA/HIP uint8 matrix of e4m3 codes")
    if W8.dim() != 4 or W8.shape[2:] != (64, 8) or not W8.is_contiguous():
        raise ValueError("gemm_fp8: W8 must come from quantize_weight_fp8")
    M, K = A8.shape
    N, Kw = W8.shape[0] * 16, W8.shape[1] * 64
    if Kw != K:
        raise ValueError(f"gemm_fp8: K mismatch A{tuple(A8.shape)} W K={Kw}")
    want = torch.float32 if epilogue in (EPI_F32, EPI_F32_BF16R) else torch.bfloat16
    if out.dtype != want or scale_a.dtype != torch.float32 or scale_w.dtype != torch.float32:
        raise TypeError("gemm_fp8: out dtype / fp32 scales")
    if scale_a.numel() < M or scale_w.numel() != N:
        raise ValueError("gemm_fp8: scale_a [M], scale_w [N]")
    d, keep = _gemm_desc(A8, A8.stride(0), W8, out, M, N, K, epilogue, bias, scale, res, res_row_mod, out_map,
                         [A8, W8, out, scale_a, scale_w])
    n_out = N // 2 if epilogue == EPI_SWIGLU else N
    esz = 4 if epilogue in (EPI_F32, EPI_F32_BF16R) else 2
    return _op("bl_gemm_fp8", (C.byref(d), scale_a.data_ptr(), scale_w.data_ptr()), (d, *keep), run,
               flops=2.0 * M * N * K, nbytes=1.0 * (M * K + N * K) + esz * M * n_out)


class Fp8Weight(NamedTuple):
    """One weight's e4m3 copy as bl_gemm_fp8 reads it: the packed codes and the fp32 scale per output channel."""
    w8: torch.Tensor
    scale: torch.Tensor


def linear_fp8(x: torch.Tensor, q: torch.Tensor, sx: torch.Tensor, w8: torch.Tensor, sw: torch.Tensor, out: torch.Tensor,
               epilogue: int = EPI_NONE, **kw) -> List[Op]:
    """The e4m3 linear as a plan fragment (nothing runs): quantise the rows of x into q / sx, then
    out = epilogue(sx[m] · sw[n] · (q @ w8.T)); `kw` as gemm_fp8's (bias, scale, res, …)."""
    return [quantize_rows_fp8(x, q, sx, run=False)[2], gemm_fp8(q, sx, w8, sw, out, epilogue, run=False, **kw)]


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, eps: float = 1e-6,
              run: bool = True) -> Op:
    _bf16(x, "x"); _bf16(out, "out")
    rows, dim = x.shape
    return _op("bl_layernorm_bf16", (x.data_ptr(), _rows(x, "x"), _bf16(w, "w").data_ptr(), _bf16(b, "b").data_ptr(),
                                     out.data_ptr(), _rows(out, "out"), rows, dim, float(eps)), (x, w, b, out), run)


def _rmsnorm(name: str, x, w, out, eps, run, nbytes_per_elem: float) -> Op:
    _bf16(x, "x"); _bf16(out, "out")
    rows, dim = x.shape
    return _op(name, (x.data_ptr(), _rows(x, "x"), _bf16(w, "w").data_ptr(), out.data_ptr(), _rows(out, "out"), rows, dim,
                      float(eps)), (x, w, out), run, nbytes=nbytes_per_elem * rows * dim)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, eps: float = 1e-6, run: bool = True) -> Op:
    return _rmsnorm("bl_rmsnorm_bf16", x, w, out, eps, run, 0.0)


def rmsnorm_skinny(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, eps: float = 1e-6, run: bool = True) -> Op:
    """HF LlamaRMSNorm in the arithmetic of the skinny GEMM's fused a_norm (bl_rmsnorm_skinny_bf16); dim in SKINNY_K."""
    return _rmsnorm("bl_rmsnorm_skinny_bf16", x, w, out, eps, run, 4.0)


def _attn_desc(q, k, v, o, B, H, Sq, Skv, hd, q_str, k_str, v_str, o_str, causal, scale, key_mask):
    d = AttnDesc()
    d.q, (d.q_bs, d.q_hs, d.q_rs) = _bf16(q, "q").data_ptr(), q_str
    d.k, (d.k_bs, d.k_hs, d.k_rs) = _bf16(k, "k").data_ptr(), k_str
    if v is not None:            # attention_probs reads q and k alone: v and o stay null
        d.v, (d.v_bs, d.v_hs, d.v_rs) = _bf16(v, "v").data_ptr(), v_str
        d.o, (d.o_bs, d.o_hs, d.o_rs) = _bf16(o, "o").data_ptr(), o_str
    if key_mask is not None:
        if key_mask.dtype != torch.uint8 or key_mask.dim() != 2 or key_mask.stride(1) != 1:
            raise TypeError("key_mask must be a [B, Skv] uint8 tensor")
        d.key_mask, d.mask_bs = key_mask.data_ptr(), key_mask.stride(0)
    d.B, d.H, d.Sq, d.Skv, d.head_dim, d.causal, d.scale = B, H, Sq, Skv, hd, int(causal), float(scale)
    return d


def attention(q, k, v, o, *, B: int, H: int, Sq: int, Skv: int, head_dim: int, q_strides, k_strides, v_strides,
              o_strides, causal: bool, scale: Optional[float] = None, key_mask: Optional[torch.Tensor] = None,
              run: bool = True) -> Op:
    """Flash attention over strided [batch, head, row, head_dim] views; strides are (batch, head, row) in elements."""
    scale = head_dim ** -0.5 if scale is None else scale
    d = _attn_desc(q, k, v, o, B, H, Sq, Skv, head_dim, q_strides, k_strides, v_strides, o_strides, causal, scale,
                   key_mask)
    return _op("bl_attention_bf16", (C.byref(d),), (d, q, k, v, o, key_mask), run)


def attention_rope(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, o: torch.Tensor, cos: torch.Tensor,
                   sin: torch.Tensor, *, B: int, S: int, H: int, head_dim: int, pos0: int = 0, scale: Optional[float] = None,
                   key_mask: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    """Prefill attention over fused, un-rotated qkv rows [B*S, 3*H*hd] with RoPE and the KV-cache write fused in
    (bl_attention_rope_bf16): caches [B, H, cache_len, hd] receive rotated k and v at positions pos0.., o [B*S, H*hd]."""
    D = H * head_dim
    _contig_bf16("attention_rope", (qkv, "qkv"), (k_cache, "k_cache"), (v_cache, "v_cache"), (cos, "cos"), (sin, "sin"))
    cache_len = k_cache.shape[2]
    scale = head_dim ** -0.5 if scale is None else scale
    st = (S * 3 * D, head_dim, 3 * D)
    d = _attn_desc(qkv, qkv[:, D:], qkv[:, 2 * D:], o, B, H, S, S, head_dim, st, st, st, (S * D, head_dim, D), True, scale, key_mask)
    return _op("bl_attention_rope_bf16",
               (C.byref(d), cos.data_ptr(), sin.data_ptr(), pos0, k_cache.data_ptr(), v_cache.data_ptr(), cache_len),
               (d, qkv, k_cache, v_cache, o, cos, sin, key_mask), run)


def attention_decode(q, k, v, o, *, B: int, H: int, Skv: int, head_dim: int, q_strides, k_strides, v_strides,
                     o_strides, scale: Optional[float] = None, key_mask: Optional[torch.Tensor] = None,
                     run: bool = True) -> Op:
    scale = head_dim ** -0.5 if scale is None else scale
    d = _attn_desc(q, k, v, o, B, H, 1, Skv, head_dim, q_strides, k_strides, v_strides, o_strides, False, scale,
                   key_mask)
    return _op("bl_attention_decode_bf16", (C.byref(d),), (d, q, k, v, o, key_mask), run)


def attention_decode_rope(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, o: torch.Tensor,
                          cos: torch.Tensor, sin: torch.Tensor, *, B: int, H: int, head_dim: int, pos: int,
                          scale: Optional[float] = None, key_mask: Optional[torch.Tensor] = None,
                          rope_pos: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    """One decode step's attention with RoPE and the KV-cache append fused: qkv [B, 3*H*hd] is the step's fused
    projection (q | k | v), caches [B, H, cache_len, hd]; rotates q and k at `pos`, writes k', v to cache row `pos`,
    attends over keys 0..pos, writes o [B, H*hd]."""
    D = H * head_dim
    _contig_bf16("attention_decode_rope", (qkv, "qkv"), (k_cache, "k_cache"), (v_cache, "v_cache"), (cos, "cos"), (sin, "sin"))
    cache_len = k_cache.shape[2]
    if pos >= cache_len or pos >= cos.shape[0]:
        raise ValueError("attention_decode_rope: position outside the cache / rope table")
    scale = head_dim ** -0.5 if scale is None else scale
    cs = (H * cache_len * head_dim, cache_len * head_dim, head_dim)
    d = _attn_desc(qkv, k_cache, v_cache, o, B, H, 1, pos + 1, head_dim, (3 * D, head_dim, 3 * D), cs, cs,
                   (D, head_dim, D), False, scale, key_mask)
    name, args, keep = "bl_attention_decode_rope_bf16", (C.byref(d), cos.data_ptr(), sin.data_ptr(), pos), \
        (d, qkv, k_cache, v_cache, o, cos, sin, key_mask)
    if rope_pos is not None:     # right-padded prompts: per-sequence rotation position (int32 [B]), shared cache row
        _dev(rope_pos, torch.int32, B, "attention_decode_rope: rope_pos")
        name, args, keep = "bl_attention_decode_rope_pos_bf16", args + (rope_pos.data_ptr(),), keep + (rope_pos,)
    return _op(name, args, keep, run)


def attention_probs(q: torch.Tensor, k: torch.Tensor, *, B: int, H: int, Sq: int, Skv: int, head_dim: int, q_strides, k_strides,
                    causal: bool, scale: Optional[float] = None, key_mask: Optional[torch.Tensor] = None,
                    cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None, pos0: int = 0,
                    rope_pos: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None,
                    seg: Optional[torch.Tensor] = None, seg_bounds: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    """The attention probabilities of q against ROTATED keys k (a KV-cache view), read-only (bl_attention_probs_f32).
    q / k are strided [batch, head, row, head_dim] views, strides (batch, head, row) in elements. With cos / sin, q is
    un-rotated and is rotated on load at pos0 + row (rope_pos[b] + row with an int32 [B] device tensor); without, q is
    rotated in memory. probs: fp32 [B, H, Sq, p_cols >= Skv] view with a contiguous last dim — columns past Skv are zeroed;
    seg: contiguous fp32 [B, H, Sq, n_seg] with seg_bounds int32 [B, n_seg + 1]. Either output may be None."""
    scale = head_dim ** -0.5 if scale is None else scale
    d = _attn_desc(q, k, None, None, B, H, Sq, Skv, head_dim, q_strides, k_strides, None, None, causal, scale, key_mask)
    if (cos is None) != (sin is None):
        raise ValueError("attention_probs: cos and sin come together")
    rope_rows = 0
    if cos is not None:
        for t, n in ((cos, "cos"), (sin, "sin")):
            _bf16(t, n)
            if not t.is_contiguous() or t.dim() != 2 or t.shape[1] != head_dim // 2:
                raise ValueError(f"attention_probs: {n} must be a contiguous [positions, head_dim/2] table")
        rope_rows = min(cos.shape[0], sin.shape[0])
    if rope_pos is not None:
        _dev(rope_pos, torch.int32, B, "attention_probs: rope_pos")
    p_ptr, p_str, p_cols = None, (0, 0, 0), 0
    if probs is not None:
        if probs.dtype != torch.float32 or not probs.is_cuda or probs.dim() != 4 or probs.stride(3) != 1 \
                or tuple(probs.shape[:3]) != (B, H, Sq):
            raise TypeError("attention_probs: probs must be a CUDA/HIP fp32 [B, H, Sq, cols] view with a contiguous last dim")
        p_ptr, p_str, p_cols = probs.data_ptr(), probs.stride()[:3], probs.shape[3]
    s_ptr, b_ptr, n_seg = None, None, 0
    if seg is not None:
        n_seg = _dev(seg, torch.float32, (B, H, Sq, None), "attention_probs: seg").shape[3]
        s_ptr, b_ptr = seg.data_ptr(), _dev(seg_bounds, torch.int32, (B, n_seg + 1), "attention_probs: seg_bounds").data_ptr()
    return _op("bl_attention_probs_f32",
               (C.byref(d), None if cos is None else cos.data_ptr(), None if sin is None else sin.data_ptr(), rope_rows, pos0,
                None if rope_pos is None else rope_pos.data_ptr(), p_ptr, p_str[0], p_str[1], p_str[2], p_cols, s_ptr, b_ptr, n_seg),
               (d, q, k, key_mask, cos, sin, rope_pos, probs, seg, seg_bounds), run,
               flops=2.0 * B * H * Sq * Skv * head_dim,
               nbytes=2.0 * B * H * (Sq + Skv) * head_dim + 4.0 * B * H * Sq * (p_cols + n_seg))


def rope_kvcache(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, *, B: int, S: int, H: int, head_dim: int, pos0: int, run: bool = True) -> Op:
    """qkv [B*S, 3*H*hd] (q rotated in place); caches [B, H, cache_len, hd]; cos/sin [max_pos, hd/2] bf16."""
    _contig_bf16("rope_kvcache", (qkv, "qkv"), (cos, "cos"), (sin, "sin"), (k_cache, "k_cache"), (v_cache, "v_cache"))
    cache_len = k_cache.shape[2]
    if pos0 + S > cos.shape[0]:
        raise ValueError("rope_kvcache: position exceeds the cos/sin table")
    return _op("bl_rope_kvcache_bf16", (qkv.data_ptr(), B, S, H, head_dim, cos.data_ptr(), sin.data_ptr(), pos0,
                                        k_cache.data_ptr(), v_cache.data_ptr(), cache_len), (qkv, cos, sin, k_cache, v_cache), run)


def embed_splice(ids: torch.Tensor, table: torch.Tensor, dst: torch.Tensor, n_patches: int, run: bool = True) -> Op:
    """dst[b,0] = table[ids[b,0]]; dst[b, 1+n_patches+j] = table[ids[b,1+j]].  ids int64 [B,L]; dst [B, L+n_patches, D]."""
    if ids.dtype != torch.int64 or not ids.is_contiguous():
        raise TypeError("ids must be a contiguous int64 tensor")
    B, L = ids.shape
    dim = table.shape[1]
    if tuple(dst.shape) != (B, L + n_patches, dim) or not dst.is_contiguous():
        raise ValueError(f"embed_splice: dst must be contiguous [{B}, {L + n_patches}, {dim}]")
    return _op("bl_embed_splice_bf16", (ids.data_ptr(), B, L, _bf16(table, "table").data_ptr(), dim, n_patches,
                                        _bf16(dst, "dst").data_ptr()), (ids, table, dst), run)


def argmax(logits: torch.Tensor, out: torch.Tensor, run: bool = True) -> Op:
    if logits.dtype != torch.float32 or out.dtype != torch.int64:
        raise TypeError("argmax: logits fp32 [rows, n], out int64 [rows]")
    rows, n = logits.shape
    return _op("bl_argmax_f32", (logits.data_ptr(), _rows(logits, "logits"), rows, n, out.data_ptr()), (logits, out), run)


def _warp_head(fn: str, logits, temperature, top_k, top_p, *own) -> tuple:
    """What sample and score share: fp32 logits [rows, n] (any row stride) and the per-row device settings are checked, then
    the caller's `own` tensors as (tensor, dtype, extents after [rows], name); returns the leading arguments of the call."""
    rows, n = logits.shape
    _f32(logits, f"{fn}: logits")
    for t, dtype, tail, name in ((temperature, torch.float32, (), "temperature"), (top_k, torch.int32, (), "top_k"),
                                 (top_p, torch.float32, (), "top_p")) + own:
        _dev(t, dtype, (rows,) + tail, f"{fn}: {name}")
    return (logits.data_ptr(), _rows(logits, "logits"), rows, n, temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr())


def sample(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
           step: int, ids: torch.Tensor, wt: torch.Tensor, run: bool = True, vocab: Optional[Tuple[int, int]] = None) -> Op:
    """One seeded draw per row of fp32 logits [rows, n] (bl_sample_f32; specification: sampling.sample_rows). Per-row
    DEVICE settings: temperature fp32 (0 = greedy), top_k int32 (0 = off), top_p fp32 (>= 1 = off), seed int64; `step` is
    the Philox counter. Writes ids int64 [rows] and wt int64 [rows, 2] = (weight of the token, kept total).
    vocab=(first, count) restricts the policy to that token range (bl_sample_range_f32)."""
    head = _warp_head("sample", logits, temperature, top_k, top_p,
                      (seed, torch.int64, (), "seed"), (ids, torch.int64, (), "ids"), (wt, torch.int64, (2,), "wt"))
    return _op("bl_sample_f32" if vocab is None else "bl_sample_range_f32",
               head + (seed.data_ptr(), int(step), ids.data_ptr(), wt.data_ptr()) + (() if vocab is None else (int(vocab[0]), int(vocab[1]))),
               (logits, temperature, top_k, top_p, seed, ids, wt), run)


def score(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, tokens: torch.Tensor,
          wt: torch.Tensor, range_first: int = 0, range_wt: Optional[torch.Tensor] = None, run: bool = True,
          vocab: Optional[Tuple[int, int]] = None) -> Op:
    """The score of a given token per row of fp32 logits [rows, n] under `sample`'s warped distribution (bl_score_f32;
    specification: sampling.score_rows). Settings as `sample`, without a seed; tokens int64 [rows] on the DEVICE (each in
    [0, n): the caller's to guarantee — a token outside scores weight 0). Writes wt int64 [rows, 2] = (kept weight of the
    token, kept total) and, given range_wt int32 [rows, count], the kept weights of tokens range_first … range_first +
    count - 1. vocab=(first, count) restricts the policy to that token range (bl_score_range_f32); range_first keeps its
    full-vocabulary numbering and the report range must lie inside `vocab`."""
    own = [(tokens, torch.int64, (), "tokens"), (wt, torch.int64, (2,), "wt")]
    if range_wt is not None:
        own.append((range_wt, torch.int32, (None,), "range_wt"))
    head = _warp_head("score", logits, temperature, top_k, top_p, *own)
    count = 0 if range_wt is None else range_wt.shape[1]
    return _op("bl_score_f32" if vocab is None else "bl_score_range_f32",
               head + (tokens.data_ptr(), wt.data_ptr(), int(range_first), count, range_wt.data_ptr() if count else None)
               + (() if vocab is None else (int(vocab[0]), int(vocab[1]))),
               (logits, temperature, top_k, top_p, tokens, wt) + ((range_wt,) if count else ()), run)


def beam_step(logits: torch.Tensor, W: int, scores_in: torch.Tensor, tokens: torch.Tensor, parents: torch.Tensor,
              wt: torch.Tensor, scores_out: torch.Tensor, run: bool = True, vocab: Optional[Tuple[int, int]] = None) -> Op:
    """One beam-search step over fp32 logits [rows, n] (any row stride; bl_beam_step_f32, specification: beam.beam_step):
    every W consecutive rows are the beams of one prompt, scores_in fp32 [rows] their scores so far. Writes, per prompt and
    best first, tokens int64 [rows], parents int32 [rows] (in [0, W)), wt int64 [rows, 2] and scores_out fp32 [rows].
    vocab=(first, count) ranks the continuations inside that token range only."""
    rows, n = _f32(logits, "beam_step: logits").shape
    if W < 1 or rows % W:
        raise ValueError(f"beam_step: {rows} rows are no whole number of prompts of {W} beams")
    for t, dtype, tail, name in ((scores_in, torch.float32, (), "scores_in"), (tokens, torch.int64, (), "tokens"),
                                 (parents, torch.int32, (), "parents"), (wt, torch.int64, (2,), "wt"),
                                 (scores_out, torch.float32, (), "scores_out")):
        _dev(t, dtype, (rows,) + tail, f"beam_step: {name}")
    first, count = (0, n) if vocab is None else (int(vocab[0]), int(vocab[1]))
    return _op("bl_beam_step_f32", (logits.data_ptr(), _rows(logits, "logits"), rows // W, int(W), n, scores_in.data_ptr(),
                                    tokens.data_ptr(), parents.data_ptr(), wt.data_ptr(), scores_out.data_ptr(), first, count),
               (logits, scores_in, tokens, parents, wt, scores_out), run)


def cache_table(caches: Sequence[torch.Tensor]) -> torch.Tensor:
    """The device table of base pointers `beam_reorder_kv` takes: int64 [len(caches)], built once per engine. The caller
    keeps the caches alive (the Op built over the table does)."""
    return torch.tensor([c.data_ptr() for c in caches], dtype=torch.int64, device=caches[0].device)


def beam_reorder_kv(table: torch.Tensor, caches: Sequence[torch.Tensor], W: int, parents: torch.Tensor, row0, n_rows: int,
                    run: bool = True) -> Op:
    """In every cache of `caches` (contiguous bf16 [rows, H, cache_len, hd], all of one shape; `table` = cache_table(caches)),
    batch row g·W + k takes cache rows row0 … row0 + n_rows - 1 of batch row g·W + parents[g·W + k], in place
    (bl_beam_reorder_kv_bf16: one launch for all caches). parents int32 [rows] on the device; row0: a host int, or an int32
    device tensor [rows] with every batch row's own first row (right-padded prompts)."""
    fn = "beam_reorder_kv"
    _contig_bf16(fn, *[(c, "cache") for c in caches])
    shape = tuple(caches[0].shape)
    if len(shape) != 4 or any(tuple(c.shape) != shape for c in caches):
        raise ValueError(f"{fn}: all caches must share one shape [rows, H, cache_len, hd]")
    rows, H, cache_len, hd = shape
    _dev(table, torch.int64, len(caches), f"{fn}: table")
    _dev(parents, torch.int32, (rows,), f"{fn}: parents")
    per_row = isinstance(row0, torch.Tensor)
    if per_row:
        _dev(row0, torch.int32, (rows,), f"{fn}: row0")
    return _op("bl_beam_reorder_kv_bf16", (table.data_ptr(), len(caches), rows, int(W), H, cache_len, hd, parents.data_ptr(),
                                           0 if per_row else int(row0), row0.data_ptr() if per_row else None, int(n_rows)),
               (table, list(caches), parents, row0), run, nbytes=4.0 * len(caches) * rows * H * n_rows * hd)


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor, row_loss: torch.Tensor, mean_and_count: torch.Tensor,
                  ignore_index: int = -100, run: bool = True) -> Op:
    """Per-row CE over fp32 logits [rows, n] against int64 targets [rows] (already shifted); mean over valid rows."""
    if logits.dtype != torch.float32 or targets.dtype != torch.int64 or row_loss.dtype != torch.float32:
        raise TypeError("cross_entropy: logits/row_loss fp32, targets int64")
    rows, n = logits.shape
    return _op("bl_cross_entropy_f32", (logits.data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
                                        row_loss.data_ptr(), mean_and_count.data_ptr()), (logits, targets, row_loss, mean_and_count), run)


def im2col_patch14(pixel_values: torch.Tensor, chan0: int, out: torch.Tensor, run: bool = True) -> Op:
    """pixel_values [B,6,224,224] bf16 → out [B*256, ld>=588] patch rows of channels chan0..chan0+2."""
    _bf16(pixel_values, "pixel_values"); _bf16(out, "out")
    if tuple(pixel_values.shape[1:]) != (6, 224, 224) or not pixel_values.is_contiguous():
        raise ValueError("im2col_patch14: pixel_values must be contiguous [B, 6, 224, 224]")
    B = pixel_values.shape[0]
    return _op("bl_im2col_patch14_bf16", (pixel_values.data_ptr(), B, chan0, out.data_ptr(), _rows(out, "out")),
               (pixel_values, out), run)


def write_prefix_tokens(prefix: torch.Tensor, x: torch.Tensor, B: int, T: int, run: bool = True) -> Op:
    n_prefix, dim = prefix.shape
    return _op("bl_write_prefix_tokens_bf16", (_bf16(prefix, "prefix").data_ptr(), n_prefix, dim, _bf16(x, "x").data_ptr(), B, T),
               (prefix, x), run)


def attention_decode_rope_grouped(qkv: torch.Tensor, k_caches: Sequence[torch.Tensor], v_caches: Sequence[torch.Tensor],
                                  o: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, B: int, H: int, head_dim: int,
                                  pos: Optional[Sequence[int]] = None, rope_pos: Optional[Sequence[torch.Tensor]] = None,
                                  run: bool = True) -> Op:
    """G decode iterations of different batches in one launch: rows g*B.. of qkv [G*B, 3*H*hd] / o [G*B, H*hd] use
    caches k_caches[g] / v_caches[g]. Exactly one of `pos` / `rope_pos` gives the positions: `pos[g]`, one host int for
    the whole group (bl_attention_decode_rope_grouped_bf16), or `rope_pos[g]`, a contiguous int32 device tensor [B] with
    every sequence's own position (right-padded batches, bl_attention_decode_rope_pos_grouped_bf16)."""
    fn = "attention_decode_rope_grouped"
    if (pos is None) == (rope_pos is None):
        raise ValueError(f"{fn}: give exactly one of pos / rope_pos")
    G, D = len(pos if rope_pos is None else rope_pos), H * head_dim
    if not (1 <= G <= 8) or len(k_caches) != G or len(v_caches) != G:
        raise ValueError(f"{fn}: 1..8 groups, one cache pair and position each")
    _contig_bf16(fn, (qkv, "qkv"), (cos, "cos"), (sin, "sin"), *[(t, "cache") for t in list(k_caches) + list(v_caches)])
    cache_len = k_caches[0].shape[2]
    if any(tuple(t.shape) != tuple(k_caches[0].shape) for t in list(k_caches) + list(v_caches)):
        raise ValueError(f"{fn}: all caches must share one shape")
    if qkv.shape[0] != G * B or o.shape[0] != G * B:
        raise ValueError(f"{fn}: row count != G*B")
    cs = (H * cache_len * head_dim, cache_len * head_dim, head_dim)
    kp = (C.c_void_p * G)(*[t.data_ptr() for t in k_caches])
    vp = (C.c_void_p * G)(*[t.data_ptr() for t in v_caches])
    if rope_pos is not None:     # the positions: a table of device pointers and the key count cache_len ...
        for t in rope_pos:
            _dev(t, torch.int32, B, f"{fn}: each rope_pos[g]")
        if tuple(k_caches[0].shape[:2]) != (B, H) or cache_len > cos.shape[0]:
            raise ValueError(f"{fn}: caches must be [B, H, cache_len, hd] with cache_len inside the rope table")
        name, Skv = "bl_attention_decode_rope_pos_grouped_bf16", cache_len
        tab = (C.c_void_p * G)(*[t.data_ptr() for t in rope_pos])
        tail, held = (tab, cache_len), (list(rope_pos),)
    else:                        # ... or a table of host ints
        if max(pos) >= cache_len or max(pos) >= cos.shape[0]:
            raise ValueError(f"{fn}: position outside the cache / rope table")
        name, Skv = "bl_attention_decode_rope_grouped_bf16", pos[0] + 1
        tab = (C.c_int32 * G)(*[int(x) for x in pos])
        tail, held = (tab,), ()
    d = _attn_desc(qkv, k_caches[0], v_caches[0], o, B, H, 1, Skv, head_dim, (3 * D, head_dim, 3 * D), cs, cs,
                   (D, head_dim, D), False, head_dim ** -0.5, None)
    return _op(name, (C.byref(d), cos.data_ptr(), sin.data_ptr(), G, kp, vp) + tail,
               (d, qkv, o, cos, sin, kp, vp, tab, list(k_caches), list(v_caches)) + held, run)


def attention_decode_rope_shared(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_gen: torch.Tensor,
                                 v_gen: torch.Tensor, o: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, group: int, H: int,
                                 head_dim: int, prefix_len: int, pos: int, scale: Optional[float] = None,
                                 gq: Optional[int] = None, run: bool = True) -> Op:
    """One decode step's attention for rows that share a prompt (bl_attention_decode_rope_shared_bf16): qkv [R, 3*H*hd] is
    the step's fused projection of R = P*group rows, row r belongs to prompt r // group. k_cache / v_cache [P, H, cache_len,
    hd] hold the prompts' rows 0 .. prefix_len-1 and are only read; k_gen / v_gen [R, H, gen_len, hd] hold every row's own
    generated tokens: rows 0 .. pos-prefix_len-1 are keys prefix_len .. pos-1, and the step's k', v are appended at row
    pos - prefix_len. o [R, H*hd]. Per row the bits of attention_decode_rope on replicated caches. gq (2, 4, 8): the rows
    per workgroup, None = the library's choice."""
    fn = "attention_decode_rope_shared"
    D = H * head_dim
    _contig_bf16(fn, (qkv, "qkv"), (k_cache, "k_cache"), (v_cache, "v_cache"), (k_gen, "k_gen"), (v_gen, "v_gen"), (o, "o"),
                 (cos, "cos"), (sin, "sin"))
    if k_cache.dim() != 4 or tuple(v_cache.shape) != tuple(k_cache.shape) or tuple(k_cache.shape[1::2]) != (H, head_dim):
        raise ValueError(f"{fn}: prompt caches must both be [P, {H}, cache_len, {head_dim}]")
    P, cache_len = k_cache.shape[0], k_cache.shape[2]
    R = P * int(group)
    if not 1 <= group <= 16 or tuple(qkv.shape) != (R, 3 * D) or tuple(o.shape) != (R, D):
        raise ValueError(f"{fn}: group in 1 .. 16, qkv [{R}, {3 * D}] and o [{R}, {D}] for {P} prompts of {group} rows")
    if k_gen.dim() != 4 or tuple(v_gen.shape) != tuple(k_gen.shape) or (k_gen.shape[0], k_gen.shape[1], k_gen.shape[3]) != (R, H, head_dim):
        raise ValueError(f"{fn}: gen caches must both be [{R}, {H}, gen_len, {head_dim}]")
    gen_len = k_gen.shape[2]
    if not 1 <= prefix_len <= cache_len or not prefix_len <= pos < prefix_len + gen_len or pos >= cos.shape[0]:
        raise ValueError(f"{fn}: prefix_len {prefix_len} / pos {pos} outside the prompt cache ({cache_len} rows), the gen cache "
                         f"({gen_len} rows) or the rope table")
    scale = head_dim ** -0.5 if scale is None else scale
    cs = (H * cache_len * head_dim, cache_len * head_dim, head_dim)
    d = _attn_desc(qkv, k_cache, v_cache, o, R, H, 1, pos + 1, head_dim, (3 * D, head_dim, 3 * D), cs, cs, (D, head_dim, D),
                   False, scale, None)
    args = (C.byref(d), cos.data_ptr(), sin.data_ptr(), pos, int(group), prefix_len, k_gen.data_ptr(), v_gen.data_ptr(), gen_len)
    keep = (d, qkv, k_cache, v_cache, k_gen, v_gen, o, cos, sin)
    if gq is None:
        return _op("bl_attention_decode_rope_shared_bf16", args, keep, run)
    return _op("bl_attention_decode_rope_shared_gq_bf16", args + (int(gq),), keep, run)


def repeat_rows(src: torch.Tensor, dst: torch.Tensor, group: int, run: bool = True) -> Op:
    """dst[r * group + j] = src[r] (bl_repeat_rows_bf16): src [rows, W] with contiguous rows (any row stride), dst contiguous
    [rows * group, W]. A pure 16-byte copy, no allocation: usable inside a captured graph."""
    _bf16(src, "src"); _bf16(dst, "dst")
    if src.dim() != 2 or src.stride(1) != 1 or group < 1 or tuple(dst.shape) != (src.shape[0] * group, src.shape[1]) or not dst.is_contiguous():
        raise ValueError(f"repeat_rows: src [rows, W] with contiguous rows, dst contiguous [rows * {group}, W]; got "
                         f"{tuple(src.shape)} stride {src.stride()} -> {tuple(dst.shape)}")
    rows, Wd = src.shape
    return _op("bl_repeat_rows_bf16", (src.data_ptr(), _rows(src, "src"), dst.data_ptr(), Wd, rows, Wd, int(group)), (src, dst), run,
               nbytes=2.0 * rows * Wd * (1 + group))


def gather_rows(src: torch.Tensor, row_index: torch.Tensor, dst: torch.Tensor, run: bool = True) -> Op:
    """dst[b] = src[b, row_index[b]] (bl_gather_rows_bf16): src [B, R, W] with contiguous rows (any row stride), row_index
    int64 device [B], dst contiguous [B, W]. A pure 16-byte copy, no allocation: usable inside a captured graph."""
    _bf16(src, "src"); _bf16(dst, "dst")
    if src.dim() != 3 or src.stride(2) != 1 or src.stride(0) != src.shape[1] * src.stride(1):
        raise ValueError(f"gather_rows: src must be [B, R, W] with contiguous rows and batch stride R * row stride, got stride {src.stride()}")
    B, R, Wd = src.shape
    if tuple(dst.shape) != (B, Wd) or not dst.is_contiguous():
        raise ValueError(f"gather_rows: dst must be contiguous [{B}, {Wd}]")
    _dev(row_index, torch.int64, B, "gather_rows: row_index")
    return _op("bl_gather_rows_bf16", (src.data_ptr(), row_index.data_ptr(), R, src.stride(1), Wd, dst.data_ptr(), B),
               (src, row_index, dst), run)


_FRAMES = (None, None, None, 3)      # uint8 frames [B, H, W, 3]


def preprocess_u8(frames: torch.Tensor, mean_std: torch.Tensor, out: torch.Tensor, run: bool = True) -> Op:
    """uint8 frames [B, H, W, 3] already at the model resolution → pixel_values [B, 6, H, W] bf16 (bl_preprocess_u8_bf16)."""
    B, H, W, _ = _dev(frames, torch.uint8, _FRAMES, "preprocess_u8: frames").shape
    if tuple(out.shape) != (B, 6, H, W) or not out.is_contiguous() or mean_std.dtype != torch.float32 or mean_std.numel() != 12:
        raise ValueError("preprocess_u8: out must be contiguous [B, 6, H, W] bf16, mean_std 12 floats")
    return _op("bl_preprocess_u8_bf16", (frames.data_ptr(), B, H, W, mean_std.data_ptr(), _bf16(out, "out").data_ptr()),
               (frames, mean_std, out), run, nbytes=B * H * W * (3 + 12.0))


def _bicubic(x: float) -> float:
    """Pillow's bicubic kernel (a = -0.5, support 2)."""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x: float) -> float:
    """Pillow's Lanczos-3 kernel (Resample.c lanczos_filter: truncated sinc, support 3)."""
    def sinc(v: float) -> float:
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTERS = {"bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


@functools.lru_cache(maxsize=64)
def resample_coeffs(in_size: int, out_size: int, filter: str = "bicubic"):
    """Pillow's coefficient table for one axis of an 8-bit separable resize (libImaging/Resample.c precompute_coeffs +
    normalize_coeffs_8bpc, whole-image box) with the bicubic (a = -0.5, support 2) or Lanczos-3 filter: (bounds int32
    [out, 2] = first tap / tap count, coefs int32 [out, ksize], ksize). Doubles throughout, in Pillow's operation order;
    22-bit fixed point, rounded half away from zero."""
    kernel, base_support = _FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = base_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = torch.zeros(out_size, 2, dtype=torch.int32)
    coefs = torch.zeros(out_size, ksize, dtype=torch.int32)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [kernel((x + xmin - center + 0.5) * inv) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx, 0], bounds[xx, 1] = xmin, xmax
        for x, v in enumerate(w):
            coefs[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
    return bounds, coefs, ksize


_COEF_DEV: dict = {}


def resize_u8(frames: torch.Tensor, out_h: int, out_w: int, filter: str = "bicubic") -> torch.Tensor:
    """uint8 frames [B, H, W, 3] on the GPU → [B, out_h, out_w, 3], bit-identical to PIL `Image.resize((out_w, out_h),
    BICUBIC | LANCZOS)` per frame: horizontal pass, uint8 intermediate, vertical pass (a pass whose size does not change
    is skipped, as in Pillow)."""
    B, H, W, _ = _dev(frames, torch.uint8, _FRAMES, "resize_u8: frames").shape
    cur = frames

    def tables(n_in, n_out):
        key = (n_in, n_out, filter, frames.device)
        if key not in _COEF_DEV:
            b, c, ks = resample_coeffs(n_in, n_out, filter)
            _COEF_DEV[key] = (b.to(frames.device), c.to(frames.device), ks)
        return _COEF_DEV[key]

    if W != out_w:
        b, c, ks = tables(W, out_w)
        dst = torch.empty(B, H, out_w, 3, dtype=torch.uint8, device=frames.device)
        _op("bl_resample_pass_u8", (cur.data_ptr(), dst.data_ptr(), B, H, W, out_w, 1, b.data_ptr(), c.data_ptr(), ks),
            (cur, dst, b, c), True)
        cur = dst
    if H != out_h:
        b, c, ks = tables(H, out_h)
        dst = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=frames.device)
        _op("bl_resample_pass_u8", (cur.data_ptr(), dst.data_ptr(), B, out_w, H, out_h, 0, b.data_ptr(), c.data_ptr(), ks),
            (cur, dst, b, c), True)
        cur = dst
    return cur


def resize_bicubic_u8(frames: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    return resize_u8(frames, out_h, out_w, "bicubic")


def crop_resize_bilinear_u8(frames: torch.Tensor, y_base: float, y_step: float, x_base: float, x_step: float,
                            out_h: int, out_w: int, out: Optional[torch.Tensor] = None, run: bool = True):
    """tf.image.crop_and_resize (+ the uint8 ↔ float32 conversions around it) of the eval-time centre crop
    (experiments/robot/openvla_utils.py:81-155) on uint8 frames [B, H, W, 3] in HBM; the four fp32 sampling constants
    come from the caller (vla/eval_preprocess.py computes them exactly as its host restatement does)."""
    B, H, W, _ = _dev(frames, torch.uint8, _FRAMES, "crop_resize_bilinear_u8: frames").shape
    if out is None:
        out = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=frames.device)
    elif tuple(out.shape) != (B, out_h, out_w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"crop_resize_bilinear_u8: out must be contiguous uint8 [{B}, {out_h}, {out_w}, 3]")
    op = _op("bl_crop_resize_bilinear_u8",
             (frames.data_ptr(), out.data_ptr(), B, H, W, out_h, out_w, float(y_base), float(y_step), float(x_base), float(x_step)),
             (frames, out), run, nbytes=B * (H * W + out_h * out_w) * 3.0)
    return out if run else op


def augment_frames_u8(frames: torch.Tensor, params: torch.Tensor, out: Optional[torch.Tensor] = None,
                      pixel_values: Optional[torch.Tensor] = None, mean_std: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    """OpenVLA's training-time image augmentation (vla/image_augment.py::augment_frame, bit-identical) on uint8 frames
    [B, H, W, 3] in HBM with the host-drawn parameter table params [B, 8] fp32 on the device (bl_augment_frames_u8).
    Writes `out` (uint8 [B, H, W, 3]) and / or, fused, `pixel_values` ([B, 6, H, W] bf16 with the 12-float `mean_std` of
    preprocess_u8: equal to preprocess_u8 of `out`). `workspace`: int64 [B, 3], zeroed inside the call."""
    B, H, W, _ = _dev(frames, torch.uint8, _FRAMES, "augment_frames_u8: frames").shape
    if H < 2 or W < 2:
        raise ValueError("augment_frames_u8: H and W must be at least 2")
    if (params.dtype != torch.float32 or params.device != frames.device or tuple(params.shape) != (B, 8)
            or not params.is_contiguous()):
        raise ValueError(f"augment_frames_u8: params must be a contiguous fp32 tensor [{B}, 8] on the frames' device")
    if out is None and pixel_values is None:
        raise ValueError("augment_frames_u8: give out, pixel_values or both")
    if out is not None and (tuple(out.shape) != (B, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous()
                            or out.device != frames.device or out.data_ptr() == frames.data_ptr()):
        raise ValueError(f"augment_frames_u8: out must be another contiguous uint8 tensor [{B}, {H}, {W}, 3] on the frames' device")
    if pixel_values is not None:
        if (tuple(pixel_values.shape) != (B, 6, H, W) or not pixel_values.is_contiguous() or pixel_values.device != frames.device
                or mean_std is None or mean_std.dtype != torch.float32 or mean_std.numel() != 12 or mean_std.device != frames.device):
            raise ValueError("augment_frames_u8: pixel_values must be contiguous [B, 6, H, W] bf16 with mean_std 12 floats")
        _bf16(pixel_values, "pixel_values")
    if workspace is None:
        workspace = torch.empty(B, 3, dtype=torch.int64, device=frames.device)
    elif (workspace.dtype != torch.int64 or workspace.numel() < B * 3 or not workspace.is_contiguous()
          or workspace.device != frames.device):
        raise ValueError(f"augment_frames_u8: workspace must be a contiguous int64 tensor of at least {B * 3} elements")
    return _op("bl_augment_frames_u8",
               (frames.data_ptr(), B, H, W, params.data_ptr(), workspace.data_ptr(), out.data_ptr() if out is not None else None,
                pixel_values.data_ptr() if pixel_values is not None else None, mean_std.data_ptr() if pixel_values is not None else None),
               (frames, params, workspace, out, pixel_values, mean_std), run,
               nbytes=B * H * W * (3.0 + (3 if out is not None else 0) + (12 if pixel_values is not None else 0)))


def fill_synth(dst: torch.Tensor, seed: int, mean: float, scale: float, *, rows: Optional[int] = None,
               cols: Optional[int] = None, ld: Optional[int] = None, run: bool = True) -> Op:
    """Deterministic synthetic fill (see oracle/synth.py for the CPU restatement of the same generator)."""
    _bf16(dst, "dst")
    if rows is None:
        rows, cols, ld = 1, dst.numel(), dst.numel()
    return _op("bl_fill_synth_bf16_2d", (dst.data_ptr(), rows, cols, ld, seed & 0xFFFFFFFF, float(mean), float(scale)), (dst,), run)
