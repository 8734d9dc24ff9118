"""Exact reference for the e4m3 GEMM family (csrc/gemm_fp8.hip): bl_gemm_fp8, bl_quantize_rows_fp8, bl_colamax_bf16 and
bl_transpose_quantize_fp8, with per-element checks. The counterpart of gemm_ref64.py, whose epilogue references, operand
generators and comparators it imports; nothing here calls into bridgelang_amd.

Composition. No exact end-to-end weight-gradient case exists: lossless quantisation (values that are e4m3 numbers times a
scale) and exact summation (small integers) cannot hold together on useful data. Exact codes, scales and layouts from the
quantisers, plus an exact GEMM on arbitrary codes, compose to it, and that is what tests/test_fp8_ref_gpu.py checks.

e4m3 (OCP e4m3fn) from the format definition
--------------------------------------------
code = s eeee mmm, bias 7: e = 0 → ±m·2^-9 (subnormal), else ±(1 + m/8)·2^(e-7); 0x7F / 0xFF are NaN, there are no
infinities, the largest finite value is 0x7E = 448. `DECODE` is that table; `FINITE` lists the 254 finite codes.
`encode_rne` returns the nearest finite code of an fp32 value, ties to the even code (the even mantissa, also across a
binade boundary), saturating at ±448; the sign bit is kept, so -0.0 and a negative value that rounds to zero give 0x80.
torch's cast is not the definition (it returns NaN above 464); tests/test_fp8_ref_cpu.py shows the two equal on [-448, 448].

Quantiser specification (`quantize_spec`; csrc/gemm_fp8.hip)
-------------------------------------------------------------
amax = max |x| of the row. live = amax >= AMAX_MIN = 2^-100. scale = fl32(amax / 448), inv = fl32(448 / amax) for a live
row, scale = inv = 1 otherwise (the zero row, and the tiny-amax rule: below 448 / FLT_MAX ≈ 1.3e-36 the division gives
+inf and 0·inf = NaN codes; 2^-100 is a power of two 2^18 above that range). code = encode_rne(fl32(x·inv)): all codes of
a row that is not live are signed zeros. The fp32 steps are torch float32 on the CPU, the encoding is the table.
For every finite bf16 input: no NaN code, scale finite and positive, |decode·scale| <= 2·amax (`check_quantised`).

Layouts, from the kernels' docstrings (`packed_index`)
------------------------------------------------------
Weight-side image of [C, Tq] codes (Tq % 64 == 0, C % 16 == 0): [C/16][Tq/64][64 lanes][16 B] with lane
ch % 16 + 16·((tok % 64) / 16) and byte tok % 16. The image bl_gemm_fp8 takes as W8 is the same packing of the [N, K]
codes (channel = n, token = k), viewed as bf16 [N/16, K/64, 64, 8] (`weight_image`).

GEMM value
----------
acc = Σ_k decode(A8[m, k])·decode(W8[n, k]) in fp64; dequantised in the order the kernel documents and performs,
x = fl32(fl32(acc·sw[n])·sa[m]) — two fp32 multiplies (`dequant`). Epilogues: gemm_ref64.linear_ref / check_epilogue on x.

Three instruments
-----------------
* Integer. Codes of integers |a| <= 8, |w| <= 6 — the range tools/micro/fp8_mfma_check.hip has shown exact on this MFMA.
  Every partial sum is an integer below 48·K, an fp32 value in any order for K <= 2^24 / 48 (`assert_integer_exact`), so
  acc is exact and x is exactly the two-multiply value. With power-of-two scales 2^p, -7 <= p <= -3, x is a multiple of
  2^-7 below 2^17 - 4 and every linear epilogue is exact in fp32 as for the dyadic bf16 cases; with arbitrary fp32 scales
  (real amax / 448 values) the epilogue's fp32 adds round, and linear_ref rounds them to fp32 exactly there.
* Selector. A8 holds all 254 finite codes (row m, column k: FINITE[(7m + 3k) mod 254]); W8 is one-hot, row n holds the
  code of 2^j(n), j = n mod 15 - 6, at column π(n) = (37n + 11) mod K. C[m, n] = decode(A8[m, π(n)])·2^j(n) is a single
  product, exact for any summation hardware: it pins the k-permutation inside the 128-wide step, the stage parity and
  the decode of every code, subnormals and both zeros included.
* Gaussian. Codes and scales of Gaussian bf16 data on both sides, K <= 1536. This MFMA's adder tree is not fp32-exact, and
  no bound per magnitude follows from its definition; the worst err / mag against the fp64 value, mag = sa·sw·Σ|a||w|,
  was measured once on the device (GAUSS_ERR_MAG_MEASURED, over the EPI_F32 cases of tests/test_fp8_ref_gpu.py) and 4× that
  is asserted (GAUSS_ERR_MAG_BOUND; the margin covers other seeds). The bound must stay at or below 1 / (8·K) for the
  largest Gaussian K so that one dropped or duplicated average product (mag / K) fails; `assert_gauss_bound_sharp`.
"""
from __future__ import annotations

import torch

import gemm_ref64 as G
import train_ref64 as T64
from gemm_ref64 import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_RES,  # noqa: F401
                        EPI_SWIGLU)
from train_ref64 import E, near_tie, rb64, ulp_bf16

FP8_MAX = 448.0
AMAX_MIN = 2.0 ** -100
A_IMAX, W_IMAX = 8, 6
GAUSS_KMAX = 1536
# measured on an MI355X over the six Gaussian cases (1x16x128 3.6e-6, 256x256x256 7.8e-6, 300x528x384 7.3e-6, 257x272x640
# 5.2e-6, 2344x512x128 1.556e-5, 768x1024x1152 4.0e-6); asserted 4× the worst = 6.224e-5 <= 1 / (8·1152) = 1.085e-4
GAUSS_ERR_MAG_MEASURED = 1.556e-5
GAUSS_ERR_MAG_BOUND = 4.0 * GAUSS_ERR_MAG_MEASURED


# ---- e4m3 ------------------------------------------------------------------------------------------------------------------
def _decode_table() -> torch.Tensor:
    t = torch.empty(256, dtype=torch.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if s else v
    return t


DECODE = _decode_table()
FINITE = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)      # 254 codes, both zeros
_POS = DECODE[:127].clone()                                                                # 0 … 448, ascending with the code


def decode(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes → fp64 values (NaN for 0x7F / 0xFF), on the codes' device."""
    return DECODE.to(codes.device)[codes.long()]


def encode_rne(x: torch.Tensor) -> torch.Tensor:
    """fp32 (finite) → nearest finite e4m3 code, ties to the even code, saturating at ±448; the sign bit is kept."""
    assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    pos = _POS.to(x.device)
    a = x.double().abs()
    i = (torch.searchsorted(pos, a.contiguous(), right=True) - 1).clamp(0, 126)          # largest i with pos[i] <= a
    j = (i + 1).clamp(max=126)
    d_lo, d_hi = a - pos[i], pos[j] - a                                                   # exact in fp64
    up = (j > i) & ((d_hi < d_lo) | ((d_hi == d_lo) & (i % 2 == 1)))
    code = torch.where(up, j, i)
    sign = torch.signbit(x).long() << 7
    return (code | sign).to(torch.uint8)


# ---- quantiser specification -------------------------------------------------------------------------------------------------
def scales_spec(amax: torch.Tensor):
    """fp32 amax → (scale, inv, live) by the specification; fp32 divisions on the CPU."""
    amax = amax.detach().float().cpu()
    live = amax >= AMAX_MIN
    safe = torch.where(live, amax, torch.ones_like(amax))
    scale = torch.where(live, safe / torch.full_like(amax, FP8_MAX), torch.ones_like(amax))
    inv = torch.where(live, torch.full_like(amax, FP8_MAX) / safe, torch.ones_like(amax))
    return scale, inv, live


def quantize_spec(x: torch.Tensor, amax: torch.Tensor = None):
    """bf16 [rows, cols] → (codes uint8 [rows, cols], scale fp32 [rows], live [rows]) on the CPU. amax: the per-row maximum
    where it is given from outside (the transposing quantiser reads it)."""
    xf = x.detach().cpu().float()
    if amax is None:
        amax = xf.abs().amax(dim=1)
    scale, inv, live = scales_spec(amax)
    return encode_rne(xf * inv[:, None]), scale, live


def transpose_quantize_spec(x: torch.Tensor, amax: torch.Tensor, ldq: int):
    """bf16 [tokens, channels] → row-major codes [channels, ldq] (token tail zero), scale [channels]."""
    T_, C_ = x.shape
    codes, scale, live = quantize_spec(x.detach().cpu().t().contiguous(), amax)
    out = torch.zeros(C_, ldq, dtype=torch.uint8)
    out[:, :T_] = codes
    return out, scale, live


# ---- layouts -----------------------------------------------------------------------------------------------------------------
def packed_index(C_: int, Tq: int) -> torch.Tensor:
    """Byte offset of code (ch, tok) in the weight-side image, [C_, Tq] int64."""
    assert C_ % 16 == 0 and Tq % 64 == 0
    ch = torch.arange(C_)[:, None]
    tok = torch.arange(Tq)[None, :]
    lane = ch % 16 + 16 * ((tok % 64) // 16)
    return (((ch // 16) * (Tq // 64) + tok // 64) * 64 + lane) * 16 + tok % 16


def pack_image(codes: torch.Tensor) -> torch.Tensor:
    """[C, Tq] codes → the packed image as flat uint8, on the codes' device."""
    C_, Tq = codes.shape
    idx = packed_index(C_, Tq).to(codes.device)
    out = torch.empty(C_ * Tq, dtype=torch.uint8, device=codes.device)
    out[idx.reshape(-1)] = codes.reshape(-1)
    return out


def weight_image(codes: torch.Tensor) -> torch.Tensor:
    """[N, K] weight codes → the W8 operand of bl_gemm_fp8 (bf16 view [N/16, K/64, 64, 8])."""
    N, K = codes.shape
    return pack_image(codes).view(torch.bfloat16).view(N // 16, K // 64, 64, 8)


# ---- GEMM value ----------------------------------------------------------------------------------------------------------------
def acc64(A8: torch.Tensor, W8: torch.Tensor) -> torch.Tensor:
    return decode(A8) @ decode(W8).t()


def acc_mag(A8, W8):
    return decode(A8).abs() @ decode(W8).abs().t()


def dequant(acc: torch.Tensor, sa: torch.Tensor, sw: torch.Tensor) -> torch.Tensor:
    """x = fl32(fl32(acc·sw[n])·sa[m]) as fp64. acc must be an fp32 value (the exact accumulator): then acc·sw is exact in
    fp64 and its rounding to fp32 is the fp32 product."""
    t = (acc * sw.double()[None, :]).float().double()
    return (t * sa.double()[:, None]).float().double()


# ---- instruments ---------------------------------------------------------------------------------------------------------------
def assert_integer_exact(K: int, pmin: int = None, pmax: int = None) -> None:
    """Every partial sum of K integer products |a·w| <= 48 is an fp32 integer; with power-of-two scales 2^p, pmin <= p <= pmax,
    x and x plus one bias / residual addend lie on the 2^-7 grid below 2^17."""
    assert A_IMAX * W_IMAX * K <= 2 ** 24, f"K = {K}: the integer product is not exact in fp32"
    if pmin is not None:
        assert pmin >= -G.ADD_FRAC and (A_IMAX * W_IMAX * K * 2.0 ** pmax + G.ADD_MAX) * 2.0 ** G.ADD_FRAC <= 2.0 ** 24


def integer_codes(shape, seed: int, imax: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-imax, imax + 1, tuple(shape), generator=g, dtype=torch.int32).float()
    codes = encode_rne(v)
    assert torch.equal(decode(codes), v.double())
    return codes


POW2_A, POW2_W = (-3, -1), (-4, -2)          # exponents of the power-of-two scales: sa·sw = 2^p, -7 <= p <= -3


def pow2_scales(n: int, seed: int, lo: int, hi: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=g).float())


def real_scales(n: int, seed: int, spread: float) -> torch.Tensor:
    """amax / 448 of n rows of 64 Gaussian bf16 values: arbitrary fp32 significands, all distinct in practice."""
    amax = G.gauss((n, 64), seed, spread).abs().amax(dim=1)
    return amax / torch.full_like(amax, FP8_MAX)


def selector_pi(N: int, K: int) -> torch.Tensor:
    return (torch.arange(N) * 37 + 11) % K


def selector_j(N: int) -> torch.Tensor:
    return torch.arange(N) % 15 - 6


def selector_case(M: int, N: int, K: int):
    """(A8 [M, K], W8 [N, K]) of the selector instrument."""
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    A8 = FINITE[(m * 7 + k * 3) % 254]
    W8 = torch.zeros(N, K, dtype=torch.uint8)
    W8[torch.arange(N), selector_pi(N, K)] = encode_rne(torch.pow(2.0, selector_j(N).float()))
    return A8, W8


def assert_selector_exact(M: int, N: int, K: int) -> None:
    pi = selector_pi(N, K)
    assert set((pi % 128).tolist()) == set(range(128)) and set((pi // 128).tolist()) == set(range(K // 128))
    assert set(selector_j(N).tolist()) == set(range(-6, 9))
    A8, W8 = selector_case(M, N, K)
    assert M == 254 and all(set(A8[:, c].tolist()) == set(FINITE.tolist()) for c in range(K))   # every column sees every code
    assert bool((decode(W8) != 0).sum(1).eq(1).all())                                           # one product per element
    x = acc64(A8, W8)
    assert torch.equal(x.float().double(), x)                                                   # each an fp32 value


def assert_gauss_bound_sharp(K: int) -> None:
    assert K <= GAUSS_KMAX and GAUSS_ERR_MAG_BOUND is not None and GAUSS_ERR_MAG_BOUND <= 1.0 / (8 * K)


# ---- checkers ------------------------------------------------------------------------------------------------------------------
def check_gemm(what: str, epi: int, A8, W8, sa, sw, got, bias=None, scale=None, res=None, res_row_mod: int = 0, rows=None,
               x=None) -> None:
    """An epilogue's logical output against the exact accumulator: integer and selector instruments. rows: the logical rows
    that `got` (and a gathered `res`) hold, under an out_map. x: dequant(acc64(A8, W8), sa, sw) where the caller has it."""
    x = dequant(acc64(A8, W8), sa, sw) if x is None else x
    if rows is not None:
        x = x[rows]
    G.check_epilogue(what, epi, x, got, bias=bias, scale=scale, res=res, res_row_mod=res_row_mod)


def gauss_err_mag(A8, W8, sa, sw, got) -> float:
    """Worst |got − acc·sw·sa| / mag of an EPI_F32 output (the figure GAUSS_ERR_MAG_MEASURED records)."""
    s = sa.double()[:, None] * sw.double()[None, :]
    return float(((got.double() - acc64(A8, W8) * s).abs() / (acc_mag(A8, W8) * s)).max().item())


def check_gauss(what: str, epi: int, A8, W8, sa, sw, got, bias=None, res=None, bound: float = None) -> None:
    """EPI_F32: |got − x| <= bound·mag. EPI_BIAS_RES: the same term through the epilogue's two adds, its two fp32 roundings
    and the dequantisation's two (c = bound / e + 4), with the near-tie term of the inner bf16 rounding, as
    gemm_ref64.check_gauss."""
    bound = GAUSS_ERR_MAG_BOUND if bound is None else bound
    K = A8.shape[1]
    assert K <= GAUSS_KMAX and bound is not None
    with T64.on_device():
        s = sa.double()[:, None] * sw.double()[None, :]
        x, mag = acc64(A8, W8) * s, acc_mag(A8, W8) * s
        if epi == EPI_F32:
            T64.assert_f32_close(got, x, mag, bound / E, what)
            return
        assert epi == EPI_BIAS_RES
        b, r = bias.double(), res.double()[:x.shape[0], :x.shape[1]]
        t = x + b
        ulp = ulp_bf16(t)
        near, _ = near_tie(t, (bound / E + 3) * E * (mag + b.abs()) / ulp)
        tie = torch.where(near, ulp, torch.zeros_like(ulp))
        T64.assert_bf16_close(got, rb64(t) + r, mag + b.abs() + r.abs(), bound / E + 4, what, tie=tie)


def assert_equal_bytes(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bad = got != want
    n = int(bad.sum())
    G.EXACT[what] = G.EXACT.get(what, 0) + got.numel()
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), bad.shape))
        raise AssertionError(f"{what}: {n} of {got.numel()} differ; first at {idx}: got {got.reshape(-1)[i].item()!r}, "
                             f"want {want.reshape(-1)[i].item()!r}")


def check_quantised(what: str, x, codes, scale, amax=None) -> None:
    """What must hold of any quantiser output for finite bf16 input: no NaN code, a finite positive scale,
    |decode·scale| <= 2·amax; for live rows the dequantisation bound |x|·2^-4 + amax·2^-9 (three mantissa bits)."""
    xf, codes, scale = x.detach().cpu().double(), codes.cpu(), scale.cpu()
    amax = xf.abs().amax(dim=1) if amax is None else amax.cpu().double()
    assert bool((codes & 0x7F != 0x7F).all()), f"{what}: {int((codes & 0x7F == 0x7F).sum())} NaN codes"
    assert bool((torch.isfinite(scale) & (scale > 0)).all()), f"{what}: scale not finite and positive"
    back = decode(codes) * scale.double()[:, None]
    assert bool((back.abs() <= 2.0 * amax[:, None]).all()), f"{what}: |decode·scale| > 2·amax"
    live = amax >= AMAX_MIN
    err = (back - xf).abs()[live]
    assert bool((err <= xf.abs()[live] * 2.0 ** -4 + amax[live][:, None] * 2.0 ** -9 + 1e-30).all()), f"{what}: dequantisation bound"


def check_quantize_rows(what: str, x, codes, scale) -> None:
    """bl_quantize_rows_fp8's logical outputs against the specification, bit for bit."""
    want_q, want_s, _ = quantize_spec(x)
    assert_equal_bytes(scale.cpu().view(torch.int32), want_s.view(torch.int32), f"{what} scales")
    assert_equal_bytes(codes, want_q, f"{what} codes")
    check_quantised(what, x, codes, scale)


def check_colamax(what: str, x, amax) -> None:
    assert_equal_bytes(amax.cpu().view(torch.int32), x.detach().cpu().float().abs().amax(dim=0).view(torch.int32), what)


def check_transpose_quantize(what: str, x, amax, q, scale, ldq: int, packed: bool) -> None:
    """bl_transpose_quantize_fp8's q (flat, channels·ldq bytes) and scales against the specification and the independent
    layout definition; the token tail must hold code 0."""
    T_, C_ = x.shape
    want, want_s, _ = transpose_quantize_spec(x, amax, ldq)
    assert_equal_bytes(scale.cpu().view(torch.int32), want_s.view(torch.int32), f"{what} scales")
    q = q.cpu().reshape(-1)
    assert q.numel() == C_ * ldq
    rows = q[packed_index(C_, ldq)] if packed else q.view(C_, ldq)          # code (ch, tok) wherever the layout puts it
    assert_equal_bytes(rows[:, T_:], want[:, T_:], f"{what} token tail")
    assert_equal_bytes(rows, want, f"{what} codes")
    check_quantised(what, x.detach().cpu().t(), rows[:, :T_], scale, amax=amax.cpu().double())
