"""fp64 reference for the bf16 GEMM family (csrc/gemm_bf16.hip, gemm_skinny.hip, gemm_common.h) and the norm forward
kernels that feed it (csrc/norm.hip, bl_rmsnorm_skinny_bf16), with per-element checks.

A helper module in the manner of train_ref64.py: written from the definitions in fp64 torch, sharing nothing with
oracle/restate.py. A rounding enters a reference only where a kernel comment makes it specification — gemm_common.h:48
`bf16(silu(g))·u`, train.hip:392 / gemm_common.h:93-103 `bf16(bf16(acc·ls) + res)`, norm.hip:56 HF RMSNorm's two roundings
`w·bf16(x·rstd)` — and is then applied to the fp64 value directly (train_ref64.rb64). The functions work on whatever
device their arguments live on (the product through torch's fp64 matmul, which shares no code with this project's
kernels); tests/test_gemm_ref_gpu.py checks once that the CPU and the device evaluation of the same case agree exactly.

Dyadic inputs — the main instrument
-----------------------------------
Activations are i/8 with integer |i| <= 16 (A_FRAC = 3, A_IMAX = 16: |a| <= 2), weights j/16 with |j| <= 16 (W_FRAC = 4:
|w| <= 1); bias, residual and table residual are bf16 multiples of 2^-7 with |·| <= 4 (ADD_MAX); LayerScale is any normal bf16
value with 2^-20 <= |ls| <= 4. All come from a seeded generator (`dyadic`).

Every product a·w is a multiple of 2^-7 and every partial sum of at most K of them lies below K·2, so it is a multiple
of 2^-7 below 2^24·2^-7 = 2^17 and therefore an fp32 value, whatever the order: MFMA-internal order, K slices, split-K
slabs and tree reductions all produce the exact product. `assert_dyadic_exact` asserts the condition
(K·amax·wmax + ADD_MAX)·2^(fa + fw) <= 2^24 — the ADD_MAX term extends it to the first epilogue add — for the K and the
value set of a case; nothing assumes it. The accumulator is the exact product x, no summation order enters any bound,
and the check is as sharp at K = 13 824 as at K = 64 (the worst-case bound K·e·|A||W|ᵀ is several bf16 ulps of a typical
output at K = 4096 and says nothing there).

Bit-exact outputs (`linear_ref`; every element, no tolerance). x is the exact product; b, r multiples of 2^-7, |·| <= 4:
* EPI_F32            out = x: an fp32 value, stored as is.
* EPI_F32_BF16R      out = bf16(x): one rounding of an exact value, the same from fp32 and from fp64.
* EPI_NONE           out = bf16(x), likewise.
* EPI_BIAS           x + b is a multiple of 2^-7 below 2^17 (the asserted condition): the fp32 add is exact; out = bf16(x + b).
                     (The reference rounds the sum to fp32 first, as the kernel's fp32 add does: the identity here.)
* EPI_RES            t = bf16(x) is a multiple of 2^-7 (rounding a multiple of 2^-7 to fewer bits keeps it one) with
                     |t| <= 2^17 - 4; t + r is a multiple of 2^-7 below 2^17: exact; out = bf16(t + r).
* EPI_BIAS_RES       t = bf16(x + b) as above, t + r exact as for EPI_RES.
  with LayerScale    t·ls is a product of two 8-bit significands: exact in fp32 (no under- or overflow for the ls range),
                     s = bf16(t·ls) is the rounding of the exact product. s + r is exact in fp32 when the two operands'
                     bits span at most 24 positions (|ls| >= 2^-8 or so); below that it is the correctly rounded fp32
                     sum. The kernel's comment makes that fp32 add the specification, so the reference forms s + r in
                     fp64 (exact: the span is at most 2^2 … 2^-42) and rounds it to fp32 once (`.float()`), which is what an
                     IEEE fp32 add returns; out = bf16 of that. For the exact-add cases the fp32 rounding is the identity.
* res_row_mod / out_map move rows only (`res_rows`, `out_rows`).
* The pre-activation output C of EPI_SWIGLU_KEEP is bf16(x), of EPI_BIAS_GELU_KEEP bf16(x + b): as NONE / BIAS.

Bounded outputs use the references, comparators and constants of train_ref64.py by import, on an argument that is exact
(so no near-tie term arises on the argument itself):
* EPI_BIAS_GELU, C2 of EPI_BIAS_GELU_KEEP   gelu_forward(bf16(x + b)): c = 4, extra = 0.5·|t|·E_ERF.
* EPI_SWIGLU, C2 of EPI_SWIGLU_KEEP         swiglu_forward(bf16(x) as gate/up pairs): c = 2, silu's near-tie and tail terms.
* EPI_SWIGLU_BWD                            swiglu_backward(res, bf16(x)): check_swiglu_backward.
* EPI_GELU_BWD                              gelu_backward(res, bf16(x)): c = 4 and its extra term.

Full-mantissa inputs — the second instrument
--------------------------------------------
Dyadic values use five significand bits; a fragment path that dropped low mantissa bits would pass them. Seeded Gaussian
bf16 operands at K <= 1536 (`GAUSS_KMAX`) close that: |got − ref| <= u·|ref| + (K + c)·e·mag + tie, mag = |A|·|W|ᵀ
(+ |b| + |r|). bf16·bf16 products are exact in fp32. Every form sums the K products of an element in SOME binary tree
of fp32 adds — the MFMA's k-steps in sequence, K slices and split-K slabs combined in slice order, the skinny kernel's
and the rows forms' balanced tree over eight slices — and in any such tree a product passes through at most K − 1 adds, so
the sum's error is at most (K − 1)·e·mag for every form: the slice, slab and tree adds are already counted in K. That
leaves c for the epilogue: EPI_F32 c = 1 (the cross term); EPI_BIAS_RES (no LayerScale) adds the bias add (1), the
residual add (1) and the cross term: c = 3 (`C_GAUSS_F32`, `C_GAUSS_BIAS_RES`). The intermediate t = bf16(acc + b) is
an fp32 value rounded to bf16 before further use: where the fp64 t lies within δ = (K + 1)·e·mag / ulp_bf16(t) ulps of a
rounding boundary the two may round apart, and ulp_bf16(t) is added to `tie` for exactly those elements (near_tie).

Norm forward (norm.hip norm_rows_kernel, gemm_skinny.hip rmsnorm_fragments)
---------------------------------------------------------------------------
norm_rows_kernel reduces a row exactly like train.hip's backward (a lane adds NCH·8 <= 80 values, six butterfly levels):
train_ref64's K_SUM, C_XHAT_RMS = 47 and C_XHAT_LN = 136 apply unchanged.
* RMSNorm  y = bf16(w·bf16(x·rstd)): w·bf16(x̂) is exact in fp32, so y is the rounding of an exact product and EQUALS
  bf16(w·bf16(x̂_fp64)) wherever the two bf16(x̂) agree; where x̂ is within DELTA_XHAT of a rounding boundary the product
  moves by |w|·ulp_bf16(x̂) and the two products' own roundings may add one more output ulp: tie = |w|·ulp_bf16(x̂) +
  ulp_bf16(y) on exactly those elements. No other slack (check_rmsnorm).
* LayerNorm y = bf16((x − μ)·rstd·w + b): x̂'s C_XHAT_LN against xa = rstd·(|x| + mean|x|), the product with w, the add of
  b and the cross term: c = C_XHAT_LN + 3 against mag = xa·|w| + |b|. A constant row (x̂ = 0, var = 0) and a row with a
  large common offset are covered by the same companion: μ's error K_SUM·e·mean|x| enters x̂ through xa. The test keeps
  offset / spread <= 2^5, where the second-order term (K_SUM·e·offset/spread)² in the variance stays below e.
* bl_rmsnorm_skinny_bf16 / the fused a_norm sum the squares by FMA over the lane's 8·KS positions, two shuffles and the
  eight waves in order: a chain of 8·KS + 10 adds, longer than K_SUM for KS > 9 (K >= 4096), where the first-order
  worst case of x̂ would be 4·KS + 8. The check is nevertheless held at train_ref64's C_XHAT_RMS and DELTA_XHAT for every K.

A run that exceeds a bound is a finding about the kernel, not a reason to widen the bound.
"""
from __future__ import annotations

import torch

import train_ref64 as T64
from train_ref64 import E, U, rb64, near_tie, ulp_bf16

A_FRAC, A_IMAX = 3, 16
W_FRAC, W_IMAX = 4, 16
ADD_FRAC, ADD_MAX = 7, 4.0
LS_MIN, LS_MAX = 2.0 ** -20, 4.0
GAUSS_KMAX = 1536
C_GAUSS_F32 = 1
C_GAUSS_BIAS_RES = 3

(EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_RES, EPI_SWIGLU, EPI_F32, EPI_F32_BF16R, EPI_SWIGLU_KEEP,
 EPI_BIAS_GELU_KEEP, EPI_SWIGLU_BWD, EPI_GELU_BWD) = range(12)          # enum bl_epilogue (include/bridgelang_hip.h)
EPI_NAMES = ["none", "bias", "bias_gelu", "bias_res", "res", "swiglu", "f32", "f32_bf16r", "swiglu_keep", "bias_gelu_keep",
             "swiglu_bwd", "gelu_bwd"]
LINEAR = (EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_BIAS, EPI_RES, EPI_BIAS_RES)
HAS_BIAS = (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_BIAS_GELU_KEEP)
HAS_RES = (EPI_RES, EPI_BIAS_RES)
SKINNY_EPIS = (EPI_NONE, EPI_RES, EPI_SWIGLU, EPI_F32, EPI_F32_BF16R)

EXACT: dict = {}          # label → elements compared bit for bit (every one equal, or the check raised)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def dyadic(shape, seed: int, frac_bits: int, imax: int) -> torch.Tensor:
    """Seeded CPU fp32 tensor of i / 2^frac_bits, integer |i| <= imax."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-imax, imax + 1, tuple(shape), generator=g, dtype=torch.int32).float() * (2.0 ** -frac_bits)


def dyadic_a(shape, seed):
    return dyadic(shape, seed, A_FRAC, A_IMAX)


def dyadic_w(shape, seed):
    return dyadic(shape, seed, W_FRAC, W_IMAX)


def dyadic_add(shape, seed):
    """Bias / residual / table residual: bf16 values that are multiples of 2^-7 with |·| <= 4 (a drawn i/128 rounded to
    bf16's eight bits stays a multiple of 2^-7)."""
    return dyadic(shape, seed, ADD_FRAC, int(ADD_MAX * 2 ** ADD_FRAC)).to(torch.bfloat16).float()


def layerscale(n: int, seed: int) -> torch.Tensor:
    """Any bf16 value in the supported range: Gaussian around 0.1, with 1, a value below 2^-8 (inexact fp32 residual add),
    the range's ends and a negative value planted in the first columns."""
    g = torch.Generator().manual_seed(seed)
    ls = (torch.randn(n, generator=g) * 0.1).to(torch.bfloat16).float()
    ls = torch.where(ls.abs() < LS_MIN, torch.full_like(ls, 0.25), ls)
    plant = torch.tensor([1.0, 1e-5, LS_MIN, -LS_MAX, -0.3, 3.0], dtype=torch.bfloat16).float()
    ls[:min(n, plant.numel())] = plant[:n]
    assert bool(((ls.abs() >= LS_MIN) & (ls.abs() <= LS_MAX)).all())
    return ls


def gauss(shape, seed: int, scale: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * scale).to(torch.bfloat16).float()


def assert_dyadic_exact(K: int, amax: float = A_IMAX * 2.0 ** -A_FRAC, wmax: float = W_IMAX * 2.0 ** -W_FRAC,
                        fa: int = A_FRAC, fw: int = W_FRAC, addmax: float = ADD_MAX) -> None:
    """Every partial sum of at most K products, and that sum plus one bias / residual addend, is an fp32 value."""
    assert fa + fw <= ADD_FRAC or addmax == 0.0, "the addends must lie on the products' grid"
    assert (K * amax * wmax + addmax) * 2.0 ** (fa + fw) <= 2.0 ** 24, f"K = {K}: the dyadic product is not exact in fp32"


def check_dyadic_values(t: torch.Tensor, frac_bits: int, vmax: float) -> None:
    s = t.double() * 2.0 ** frac_bits
    assert bool((s == s.round()).all()) and float(t.abs().max()) <= vmax


# ---- the product ----------------------------------------------------------------------------------------------------------
def product(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """A [M, K] · W [N, K]ᵀ in fp64, on the arguments' device."""
    return A.double() @ W.double().t()


def product_mag(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    return A.double().abs() @ W.double().abs().t()


def product_tn(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Aᵀ·B over the token rows: A [T, M], B [T, N] → [M, N] (bl_gemm_tn_bf16)."""
    return A.double().t() @ B.double()


# ---- row maps -------------------------------------------------------------------------------------------------------------
def res_rows(M: int, res_row_mod: int, device) -> torch.Tensor:
    m = torch.arange(M, device=device)
    return m % res_row_mod if res_row_mod else m


def out_rows(M: int, out_map, device):
    """(kept logical rows, their output rows) under out_map = (group, stride, offset); rows mapped outside a group's
    stride are dropped (bl_gemm_desc)."""
    m = torch.arange(M, device=device)
    if out_map is None:
        return m, m
    group, stride, offset = out_map
    g = m // group
    r = m - g * group + offset
    keep = (r >= 0) & (r < stride)
    return m[keep], (g * stride + r)[keep]


# ---- references -------------------------------------------------------------------------------------------------------------
def _f32(v: torch.Tensor) -> torch.Tensor:
    """The fp32 add of the specification: one rounding of the exact fp64 sum, which is what an IEEE fp32 add returns. The
    identity for the dyadic cases (their sums are fp32 values); it matters where x is an arbitrary fp32 value (fp8_ref64.py)."""
    return v.float().double()


def linear_ref(epi: int, x, bias=None, scale=None, res=None, res_row_mod: int = 0) -> torch.Tensor:
    """The six linear epilogues on the exact product x (fp64), as fp64 values that are bf16 (fp32 for EPI_F32) numbers."""
    if epi == EPI_F32:
        return x
    if epi in (EPI_F32_BF16R, EPI_NONE):
        return rb64(x)
    t = _f32(x + bias.double()) if epi in HAS_BIAS else x
    t = rb64(t)
    if epi == EPI_BIAS:
        return t
    assert epi in HAS_RES
    if scale is not None:
        assert epi == EPI_BIAS_RES
        t = rb64(t * scale.double())
    r = res.double()[res_rows(x.shape[0], res_row_mod, x.device)][:, :x.shape[1]]
    return rb64((t + r).float().double())        # the fp32 add of the specification: one rounding of the exact sum


def preact_ref(epi: int, x, bias=None) -> torch.Tensor:
    """Pre-activation kept by the *_KEEP forms, and the argument of every activation epilogue: bf16(x [+ b])."""
    return rb64(_f32(x + bias.double())) if epi in HAS_BIAS else rb64(x)


def assert_exact(got: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    """Every element of got equals the reference value (−0 == +0), none excluded."""
    got = got.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = ~(got == ref)                                  # NaN in got counts as a mismatch
    n = int(bad.sum().item())
    EXACT[what] = EXACT.get(what, 0) + got.numel()
    print(f"gemm_ref64: {what}: {got.numel()} elements bit-exact" if n == 0 else f"gemm_ref64: {what}: {n} MISMATCHES")
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0].item())
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), bad.shape))
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ from the exact reference; first at {idx}: got "
                             f"{got.reshape(-1)[i].item():.9g}, ref {ref.reshape(-1)[i].item():.9g}")


def check_epilogue(what: str, epi: int, x, got, got2=None, bias=None, scale=None, res=None, res_row_mod: int = 0) -> None:
    """One epilogue's logical output(s) against the exact product x: bit for bit where linear, else train_ref64's bounds.
    got / got2: the logical [M, n_out] outputs (got2 = C2 of the *_KEEP forms); res for the *_BWD forms is the saved
    pre-activation."""
    with T64.on_device():
        if epi in LINEAR:
            assert_exact(got, linear_ref(epi, x, bias, scale, res, res_row_mod), what)
            return
        t = preact_ref(epi, x, bias)
        if epi in (EPI_SWIGLU_KEEP, EPI_BIAS_GELU_KEEP):
            assert_exact(got, t, f"{what} pre-activation")
            got = got2
        if epi in (EPI_BIAS_GELU, EPI_BIAS_GELU_KEEP):
            r = T64.gelu_forward(t)
            T64.assert_bf16_close(got, r["y"], r["mag"], 4, what, extra=r["extra"])
        elif epi in (EPI_SWIGLU, EPI_SWIGLU_KEEP):
            r = T64.swiglu_forward(t)
            T64.assert_bf16_close(got, r["act"], r["mag"], 2, what, tie=r["tie"], extra=r["extra"])
        elif epi == EPI_SWIGLU_BWD:
            T64.check_swiglu_backward(what, T64.swiglu_backward(res.double()[:x.shape[0], :2 * x.shape[1]], t), got)
        elif epi == EPI_GELU_BWD:
            r = T64.gelu_backward(res.double()[:x.shape[0], :x.shape[1]], t)
            T64.assert_bf16_close(got, r["dx"], r["mag"], 4, what, extra=r["extra"])
        else:
            raise ValueError(epi)


def check_gauss(what: str, epi: int, A, W, got, bias=None, res=None) -> None:
    """Full-mantissa operands: EPI_F32 or EPI_BIAS_RES (no LayerScale) against the fp64 product with the derived bound."""
    K = A.shape[1]
    assert K <= GAUSS_KMAX
    with T64.on_device():
        x, mag = product(A, W), product_mag(A, W)
        if epi == EPI_F32:
            T64.assert_f32_close(got, x, mag, K + C_GAUSS_F32, what)
            return
        assert epi == EPI_BIAS_RES
        b, r = bias.double(), res.double()[:x.shape[0], :x.shape[1]]
        t = x + b
        ulp = ulp_bf16(t)
        near, _ = near_tie(t, (K + 1) * E * (mag + b.abs()) / ulp)
        tie = torch.where(near, ulp, torch.zeros_like(ulp))
        ref = rb64(t) + r
        T64.assert_bf16_close(got, ref, mag + b.abs() + r.abs(), K + C_GAUSS_BIAS_RES, what, tie=tie)


# ---- norm forward -----------------------------------------------------------------------------------------------------------
def rmsnorm_ref(x, w, eps: float):
    """HF LlamaRMSNorm y = bf16(w·bf16(x·rstd)) before its last rounding, its companion and near-tie term."""
    x, w = x.double(), w.double()
    xh = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    xr = rb64(xh)
    near, ulp = near_tie(xh, T64.DELTA_XHAT)
    y = w * xr
    return dict(y=y, mag=y.abs(), tie=torch.where(near, w.abs() * ulp + ulp_bf16(y), torch.zeros_like(ulp)), xhat=xh)


def layernorm_ref(x, w, b, eps: float):
    x, w, b = x.double(), w.double(), b.double()
    xc = x - x.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xa = rstd * (x.abs() + x.abs().mean(-1, keepdim=True))
    return dict(y=xc * rstd * w + b, mag=xa * w.abs() + b.abs())


def check_rmsnorm(what: str, got, x, w, eps: float, cols=None) -> None:
    """y = bf16(w·bf16(x̂)) per element: equal to the reference's rounding except where x̂ is a near tie (then within
    |w|·ulp plus one output ulp). Serves the norm kernels' output and the fused a_norm's activations, read out exactly through a
    0/1 weight (`cols`: the columns that weight selects)."""
    with T64.on_device():
        r = rmsnorm_ref(x, w, eps)
        ref, tie = rb64(r["y"]), r["tie"]
        if cols is not None:
            ref, tie = ref[:, cols], tie[:, cols]
        T64._compare(got, ref, tie + T64.FLOOR, what)


def check_gauss_norm(what: str, got, x, nw, eps: float, W) -> None:
    """EPI_F32 of the skinny GEMM with the fused a_norm, full-mantissa weight W [N, K]: the fp64 product of the reference's
    normalised activations with W, the summation bound (K + 1)·e·mag, and Σ_k tie_k·|W_nk| for the activations that are
    near ties of the norm's inner rounding."""
    K = x.shape[1]
    assert K <= GAUSS_KMAX
    with T64.on_device():
        r = rmsnorm_ref(x, nw, eps)
        xn = rb64(r["y"])
        ref, mag = product(xn, W), product_mag(xn, W)
        T64.assert_f32_close(got, ref, mag, K + C_GAUSS_F32, what, tie=r["tie"] @ W.double().abs().t())


def check_layernorm(what: str, got, x, w, b, eps: float) -> None:
    with T64.on_device():
        r = layernorm_ref(x, w, b, eps)
        T64.assert_bf16_close(got, r["y"], r["mag"], T64.C_XHAT_LN + 3, what)


# ---- close_bf16, as a predicate (the older yardstick of tests/test_ops_gpu.py; evidence only) ----------------------------------
def close_bf16_accepts(got: torch.Tensor, ref: torch.Tensor, min_exact: float = 0.98) -> bool:
    """close_bf16 of tests/test_ops_gpu.py as a predicate: every element within 2^-6·|ref| + 2^-8·max|ref|, and at least
    98 % of the elements equal."""
    got, ref = got.double(), ref.double()
    tol = 2.0 ** -6 * ref.abs() + 2.0 ** -8 * (float(ref.abs().max()) + 1e-30)
    return bool(((got - ref).abs() <= tol).all()) and float((got == ref).double().mean()) >= min_exact
