"""fp64 reference for the training-step kernels (bridgelang_amd/csrc/train.hip) and per-element error bounds.

A helper module, not a test module: tests import it as `from train_ref64 import ...`. Every function is written from
the mathematical definition of its op with fp64 torch and shares nothing with oracle/restate.py, which restates the
kernels' own rounding choices and so cannot catch a kernel that shares one of them by mistake. A rounding enters a
reference only where the kernel's header comment makes it part of the specification (train.hip:72 `dw = Σ dy ⊙ bf16(x̂)`,
bl_common.h:61 `act = bf16(silu(g))·u`, train.hip:392 `y = bf16(bf16(u·ls) + res)`); it is then applied to the fp64 value
(`rb64`, a direct fp64 → bf16 round-to-nearest-even, never through fp32).

Every reference returns the value, its magnitude companion `mag` (the same expression with every term replaced by its
absolute value) and, where the kernel rounds an fp32 intermediate to bf16 before a product, a near-tie companion `tie`.
References work in row slices of at most 2^21 elements, so the largest case (8200 x 2560) holds a few hundred MB.

Comparators (per element, every element, nothing excluded); u = 2^-8 (bf16), e = 2^-24 (fp32):

    bf16 outputs:  |got − ref| <= u·|ref| + c·e·mag + tie + extra + FLOOR          (assert_bf16_close)
    fp32 outputs:  |got − ref| <=           c·e·mag + tie + extra + FLOOR          (assert_f32_close)

u·|ref| is the final rounding of the output (its cross term with the error before it, u·c·e·mag, is below e·mag and is
counted as +1 in every c). `extra` carries the documented error of an approximation as an explicit absolute term.

Near ties. Where the kernel computes bf16(t) from an fp32 t whose relative error is at most r·e, and the fp64 t lies
within δ = r·2^-16 bf16 ulps of a rounding boundary (ulp_bf16(t) >= 2^-8·|t|, so r·e·|t| <= r·2^-16 ulp), the fp32 and the
fp64 value may legitimately round to different sides: the term moves by |other factor|·ulp_bf16(t), which is added to
`tie` for exactly those terms (near_tie). Everywhere else the two roundings agree and t's fp32 error does not enter.

Constants, term by term (first-order worst-case bounds, not statistical ones; fp32 add / mul / fma / correctly rounded
division and sqrtf — the build has no fast-math flag, csrc/Makefile:5 — each contribute at most 1·e relative):

* Wave reduction over a row (train.hip:136-190): a lane adds at most NCH·8 <= 80 values in sequence, wave_sum adds 6
  butterfly levels (bl_common.h:31): 86 adds, +1 for the product inside, +1 for ·inv_dim: K_SUM = 88.
* rstd = 1/sqrtf(mean + eps) (train.hip:168): (K_SUM + 1 [+eps]) / 2 + 0.5 [sqrtf] + 0.5 [division] + 1 [x − μ] <= 47.
  LayerNorm's μ has absolute error K_SUM·e·mean|x|; Σ(x − μ) = 0, so the variance does not see it to first order.
* x̂ (train.hip:207): RMSNorm 47·e·|x̂| → C_XHAT_RMS = 47. LayerNorm adds rstd·K_SUM·e·mean|x| + 1: relative to the
  companion xa = rstd·(|x| + mean|x|) that is 47 + 88 + 1 → C_XHAT_LN = 136. RMSNorm's companion is xa = |x̂|.
* dot = mean(g·x̂) (train.hip:184-188): x̂'s error + 3 products + K_SUM + 1 = 228 (LN) relative to mean(|g|·xa);
  gsum = mean(g): K_SUM + 2 = 90 relative to mean|g|.
* dx = rstd·(g − gsum − x̂·dot) [+ dres] (train.hip:208): the g term 47 + 4 = 51, the gsum term 47 + 90 + 3 = 140, the
  x̂·dot term 136 + 228 + 47 + 3 = 414, dres 1; +1 for the cross term → C_NORM_DX = 420 against
  mag = rstd·(|g| + mean|g| [LN] + xa·mean(|g|·xa)) + |dres|.
* Row reductions dw / db / dscale / colsum: a thread adds `chain` rows in sequence, the block adds its 4 waves (3 adds,
  train.hip:232, :299), reduce_partials_kernel (train.hip:244-265) adds ceil(nblocks/32) partials per chain, 3 adds for
  the 8 chains and 2 for the 4 row groups: depth = chain + 3 + ceil(nblocks/32) + 5 (reduce_depth). chain = rpb/4 for the
  norm backward (a wave owns every fourth row or RPW-group) and for colsum (a row group owns every fourth row), and rpb
  for LayerScale (one thread walks the whole block, train.hip:421; no 4-wave add, counted anyway).
  - RMSNorm dw = Σ dy·bf16(x̂): the product 1 + depth + 1; x̂'s own error enters through `tie` alone, with
    δ = DELTA_XHAT = 2^-10 ulp (47·2^-16 rounded up to a power of two).
  - LayerNorm dw = Σ dy·x̂ (unrounded): C_XHAT_LN + 1 + depth against Σ|dy|·xa.  db = Σ dy, colsum: depth.
  - dscale = Σ dy·u: bf16·bf16 is exact in fp32: depth.   du = dy·ls is exact before its rounding: c = 1.
* scale_residual y = bf16(bf16(u·ls) + res) (train.hip:406): u·ls is exact in fp32, so the inner rounding is the
  rounding of the exact product, the same in fp32 and fp64; the fp32 sum is 1·e: c = 2. In practice bit-exact.
* SwiGLU forward (train.hip:312, silu_f bl_common.h:60): __expf(−g) = v_exp_f32(−g·log2e): the product's rounding
  moves the exponent by |g|·e, the instruction is 1 ulp = 2e; 1 + ·: 1; v_rcp_f32 1 ulp = 2; g·: 1 → silu's relative
  error <= (|g| + 6)·e, used as δ = (|g| + 8)·2^-16 ulp for the rounding bf16(silu(g)); the product with u and the cross
  term: c = 2. Tail: v_exp_f32 overflows to +inf above 2^128 (g < −88.7) and v_rcp_f32 flushes a denormal result
  (1 + e^-g > 2^126, g < −87.3), so below g = −87 silu_f may return 0 where the value is |g|·e^g <= |g|·2^-125.5:
  `extra` = |g|·2^-125·|u| for g < −87 (SILU_TAIL_G, an explicit term, not folded into c).
* SwiGLU backward (swiglu_bwd_pair, bl_common.h:63-67: ocml expf, 1 ulp, and a true division): σ has relative error
  <= 5·e. 1 − σ cancels for g > 0: its absolute error is at most 3·2^-25 while 1 − σ >= 2^-26 (g <= 18) and its own size
  beyond, so g·(1 − σ) is off by at most 18·1.5·e = 27·e relative to 1 <= the factor's companion σ·(1 + |g|·(1 − σ))/σ;
  σ 5, three products 3, cross 1 → C_SWIGLU_DG = 40 against |d·u|·σ·(1 + |g|·(1 − σ)).
  d up = d·bf16(g·σ): c = 2 and δ = 8·2^-16 ulp (g·σ: 5 + 1, rounded up). Tail as in the forward: expf overflows for
  g < −88.7, σ = 0 there: `extra` = |d·u|·(1 + |g|)·2^-125 resp. |d|·|g|·2^-125 for g < −87.
* erf_as (bl_common.h:49-55, Abramowitz & Stegun 7.1.26, the formula's own |error| <= A_S = 1.5e-7). Its fp32 evaluation adds:
  the five coefficients' representation and the five fma roundings of a Horner chain whose partial sums stay below 1.5
  (Σ|coefficient| = 4.48, partials <= 3 in all: 7.5·e at t = 1), the argument's product x·0.7071 (z·erf'(z) <= 0.48: 0.5),
  __expf(−z²) (z²·e^-z² <= 0.37 times 1.5, + 2: 1), the reciprocal and 1 − p (1.5) → C_ERF_FP32 = 11 and
  E_ERF = A_S + 11·e = 8.1e-7, an ABSOLUTE error of erf. GELU forward (bl_common.h:56): `extra` = 0.5·|x|·E_ERF — it
  decides the far negative tail, where the value 0.5·x·(1 + erf) vanishes and u·|ref| with it — and c = 4 for the
  products against mag = 0.5·|x|·(1 + |erf|). GELU backward (bl_common.h:69): dx = dy·(Φ(x) + x·φ(x)); `extra` =
  |dy|·(0.5·E_ERF + (0.75·x² + 3)·e·|x|·φ(x)) (the second term is __expf(−x²/2)'s argument rounding and ulp), c = 4 against
  |dy|·(0.5·(1 + |erf|) + |x|·φ(x)).
* RoPE backward (train.hip:385): two exact bf16 products and one fp32 add: c = 2 against |d1·c| + |d2·s|.
* scale (train.hip:495): bf16(s·x), s the fp32 value the kernel receives: c = 2.
* Cross-entropy backward (train.hip:29-69): the row maximum is exact; Σ exp: a thread adds n/1024 groups of 4 (<= 126
  adds at n = 32064), 6 + 3 for the wave and block sums, expf 2, l − max 1: 138; inv 2; expf(l − max) again 2 and its
  argument's rounding |l − max|·e <= 100·e for logits within 100 of the maximum; the product and the subtraction 2;
  cross 1 → C_CE = 256 against mag = (p + onehot)/n_valid (p − 1 cancels at a confident target).
  Forward (glue.hip:172-224): row loss = logf(Σ) + max − l_t: Σ's relative error 138·e is an absolute error of the log,
  logf 2, two adds 2; the mean adds rows/256 + 9 values (<= 16 here): C_CE_MEAN = 160 against
  mean over valid rows of (1 + |log Σ| + |max| + |l_t|).
* gemm_tn_small (train.hip:707-797): products of bf16 values are exact, the MFMA adds T of them in fp32: the plain
  γ_T; the split sum (reduce_partials over <= 4 splits) and alpha: c = T + 8 (C_TN_EXTRA) against |alpha|·|P|ᵀ|Q|.
* embed_backward (train.hip:856-871): a float atomicAdd per hit: γ_n over the n hits of a row plus its previous
  content: c = n_hits + 1 against |dw0| + Σ|dx|.
* sumsq_partial (train.hip:801-821): a thread squares and adds ceil(n / (4·256·nblocks)) vectors (+ up to 3 tail
  elements), adds its 4 chains (2), the wave (6) and the block (3); the caller adds the partials: c = chain + 16 against
  Σ g². clip_coef (train.hip:823-837) sums the partials in fp64: norm = fp32(sqrt(·)): c = 1; coef = min(1, max_norm /
  (norm + 1e-6)): the norm 1, the add 1, the division 1, cross 1: c = 4.
* AdamW (train.hip:839-853), against the fp64 step on the kernel's fp32 inputs and fp32 hyper-parameters: 1 − β is
  exact (Sterbenz); powf(β, step) is exact at step 1 and leaves 1 − β^step with relative error <= 2·e at step 1000.
  m: g·coef 1, two products and the add 3 → C_ADAM_M = 4 against |β1·m| + |(1 − β1)·g·coef|. v: one product more →
  C_ADAM_V = 6. The update (lr/bc1)·m/(√v/bc2s + eps): m 4, √v 3 + 0.5, bc2s 2 + 1, + eps 1, the division 1, lr/bc1 2 + 1:
  15.5; p·(1 − lr·wd) 3 and the subtraction 1 → C_ADAM_P = 20 against |p| + the update's companion.

FLOOR = 2^-116: a flushed fp32 denormal (below 2^-126) times operands below 2^10; it also covers outputs that are
themselves bf16 denormals.

These constants are the ones derived above. A GPU run that exceeds a bound is a finding about the kernel, not a reason
to widen it.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

U = 2.0 ** -8
E = 2.0 ** -24
FLOOR = 2.0 ** -116
A_S = 1.5e-7
C_ERF_FP32 = 11
E_ERF = A_S + C_ERF_FP32 * E
K_SUM = 88
C_XHAT_RMS = 47
C_XHAT_LN = 136
C_NORM_DX = 420
DELTA_XHAT = 2.0 ** -10
C_SWIGLU_DG = 40
SILU_TAIL_G = -87.0
SILU_TAIL = 2.0 ** -125
C_CE = 256
C_CE_MEAN = 160
C_TN_EXTRA = 8
C_ADAM_M, C_ADAM_V, C_ADAM_P = 4, 6, 20

RATIOS: Dict[str, float] = {}      # label → largest err / bound seen (printed by every comparator call)

_SLICE_ELEMS = 1 << 21


_ON_DEVICE = [False]


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().double() if _ON_DEVICE[0] else t.detach().cpu().double()


class on_device:
    """Context: the element-wise references and the comparators stay on the device their arguments live on (same fp64
    arithmetic; used by tests/gemm_ref64.py, whose largest outputs hold 4·10^7 elements). Default: everything on the CPU."""

    def __enter__(self):
        self.was, _ON_DEVICE[0] = _ON_DEVICE[0], True

    def __exit__(self, *exc):
        _ON_DEVICE[0] = self.was


def _slices(rows: int, cols: int):
    step = max(1, _SLICE_ELEMS // max(1, cols))
    for r0 in range(0, rows, step):
        yield slice(r0, min(rows, r0 + step))


# ---- bf16 rounding of fp64 values -------------------------------------------------------------------------------------
def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 around the fp64 value v (8-bit significand; denormal spacing 2^-133 below 2^-126)."""
    # |v| = m·2^ex, m in [0.5, 1): ex and 2^(ex − 8) straight from / to the fp64 exponent field — integer work, exact on every
    # device (a device ldexp / frexp may go through exp2 and miss the power of two by an ulp)
    ex = ((v.contiguous().view(torch.int64) >> 52) & 0x7FF) - 1022
    return ((torch.clamp(ex - 8, min=-133) + 1023) << 52).view(torch.float64)


def rb64(v: torch.Tensor) -> torch.Tensor:
    """fp64 → nearest bf16 value (ties to even), returned as fp64: one rounding, not fp64 → fp32 → bf16."""
    ulp = ulp_bf16(v)
    return torch.round(v / ulp) * ulp            # torch.round is half-to-even; v / ulp is exact (power of two)


def near_tie(v: torch.Tensor, delta_ulps):
    """(mask, ulp): v lies within delta_ulps bf16 ulps of a rounding boundary (the midpoint of two bf16 neighbours)."""
    ulp = ulp_bf16(v)
    t = v.abs() / ulp
    return ((t - torch.floor(t)) - 0.5).abs() <= delta_ulps, ulp


# ---- the launchers' blocking rules (needed for the reduction depth and for sizing the workspaces) -----------------------
def norm_bwd_blocking(rows: int, dim: int, ws_floats: int, ln: bool):
    """(rows_per_block, nblocks) of norm_backward (train.hip:901-910); None when the launcher must reject."""
    rpb = 16
    while ((rows + rpb - 1) // rpb) * dim * (2 if ln else 1) > ws_floats:
        rpb *= 2
        if rpb > 4096:
            return None
    nch = (dim // 8 + 63) // 64
    if nch >= 5 and (rows + rpb - 1) // rpb > 512:
        rpb = max(rpb, ((rows + 511) // 512 + 3) // 4 * 4)
    return rpb, (rows + rpb - 1) // rpb


def rows_blocking(rows: int, cols: int, ws_floats: int, rpb0: int):
    """(rows_per_block, nblocks) of bl_layerscale_backward_bf16 (rpb0 = 16, train.hip:964-969) and bl_colsum_bf16
    (rpb0 = 64, train.hip:1066-1071)."""
    rpb = rpb0
    while ((rows + rpb - 1) // rpb) * cols > ws_floats:
        rpb *= 2
    return rpb, (rows + rpb - 1) // rpb


def tn_splits(T: int, R: int, N: int, ws_floats: int) -> int:
    """Split count of bl_gemm_tn_small_bf16 (train.hip:1186-1190)."""
    slabs, splits = N // 64, 1
    while slabs * splits < 256 and (T + splits * 2 - 1) // (splits * 2) >= 256 and ws_floats and splits * 2 * R * N <= ws_floats:
        splits *= 2
    return splits


def reduce_depth(chain: int, nblocks: int) -> int:
    return chain + 3 + (nblocks + 31) // 32 + 5


# ---- references -----------------------------------------------------------------------------------------------------
def norm_backward(x, w, dy, eps: float, dres=None, ln: bool = False):
    """RMSNorm / LayerNorm backward (train.hip:71-74). Returns dx, m_dx, dw, m_dw, tie_dw (RMSNorm) and db, m_db (LN)."""
    x, w, dy = f64(x), f64(w), f64(dy)
    dres = None if dres is None else f64(dres)
    rows, dim = x.shape
    out = dict(dx=torch.empty_like(x), m_dx=torch.empty_like(x))
    for k in ("dw", "m_dw", "tie_dw", "db", "m_db"):
        out[k] = torch.zeros(dim, dtype=torch.float64)
    for s in _slices(rows, dim):
        xs, ds = x[s], dy[s]
        if ln:
            xc = xs - xs.mean(-1, keepdim=True)
            xabs = xs.abs() + xs.abs().mean(-1, keepdim=True)
        else:
            xc, xabs = xs, xs.abs()
        rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
        xh, xa = xc * rstd, xabs * rstd
        g = w * ds
        dot = (g * xh).mean(-1, keepdim=True)
        gsum = g.mean(-1, keepdim=True) if ln else torch.zeros_like(dot)
        dx = rstd * (g - gsum - xh * dot)
        m = rstd * (g.abs() + (g.abs().mean(-1, keepdim=True) if ln else 0.0) + xa * (g.abs() * xa).mean(-1, keepdim=True))
        if dres is not None:
            dx, m = dx + dres[s], m + dres[s].abs()
        out["dx"][s], out["m_dx"][s] = dx, m
        if ln:
            out["dw"] += (ds * xh).sum(0)
            out["m_dw"] += (ds.abs() * xa).sum(0)
            out["db"] += ds.sum(0)
            out["m_db"] += ds.abs().sum(0)
        else:
            xr = rb64(xh)
            near, ulp = near_tie(xh, DELTA_XHAT)
            out["dw"] += (ds * xr).sum(0)
            out["m_dw"] += (ds.abs() * xr.abs()).sum(0)
            out["tie_dw"] += torch.where(near, ds.abs() * ulp, torch.zeros_like(ulp)).sum(0)
    return out


def scale_residual(u, ls, res):
    """y = bf16(bf16(u ⊙ ls) + res) before its last rounding, and its companion (train.hip:392)."""
    u, ls, res = f64(u), f64(ls), f64(res)
    t = rb64(u * ls)
    return t + res, t.abs() + res.abs()


def layerscale_backward(dy, u, ls):
    """du = dy ⊙ ls; dscale = Σ_rows dy ⊙ u (train.hip:393)."""
    dy, u, ls = f64(dy), f64(u), f64(ls)
    du = dy * ls
    return dict(du=du, m_du=du.abs(), dscale=(dy * u).sum(0), m_dscale=(dy * u).abs().sum(0))


def colsum(a):
    a = f64(a)
    return a.sum(0), a.abs().sum(0)


def _sigmoid(g):
    return torch.sigmoid(g)


def swiglu_forward(gu):
    """act = bf16(silu(gate))·up on interleaved gate/up (train.hip:303, bl_common.h:61). Returns act, mag, tie, extra."""
    gu = f64(gu)
    g, up = gu[:, 0::2], gu[:, 1::2]
    s = g * _sigmoid(g)
    sr = rb64(s)
    near, ulp = near_tie(s, (g.abs() + 8.0) * 2.0 ** -16)
    tie = torch.where(near, up.abs() * ulp, torch.zeros_like(s))
    extra = torch.where(g < SILU_TAIL_G, g.abs() * SILU_TAIL * up.abs(), torch.zeros_like(s))
    act = sr * up
    return dict(act=act, mag=act.abs(), tie=tie, extra=extra)


def swiglu_backward(gu, dact):
    """d gate = d·up·σ(g)·(1 + g·(1 − σ(g))), d up = d·bf16(g·σ(g)), interleaved like gu (bl_common.h:63-67)."""
    gu, d = f64(gu), f64(dact)
    g, up = gu[:, 0::2], gu[:, 1::2]
    sg, omsg = _sigmoid(g), _sigmoid(-g)
    tailm = g < SILU_TAIL_G
    zero = torch.zeros_like(g)
    dg = d * up * (sg * (1.0 + g * omsg))
    m_dg = (d * up).abs() * sg * (1.0 + g.abs() * omsg)
    x_dg = torch.where(tailm, (d * up).abs() * (1.0 + g.abs()) * SILU_TAIL, zero)
    s = g * sg
    near, ulp = near_tie(s, 8.0 * 2.0 ** -16)
    du = d * rb64(s)
    t_du = torch.where(near, d.abs() * ulp, zero)
    x_du = torch.where(tailm, d.abs() * g.abs() * SILU_TAIL, zero)

    def il(a, b):
        o = torch.empty_like(gu)
        o[:, 0::2], o[:, 1::2] = a, b
        return o
    c = il(torch.full_like(g, float(C_SWIGLU_DG)), torch.full_like(g, 2.0))
    return dict(dgu=il(dg, du), mag=il(m_dg, du.abs()), tie=il(zero, t_du), extra=il(x_dg, x_du), c=c)


_RSQRT2 = 1.0 / math.sqrt(2.0)
_RSQRT2PI = 1.0 / math.sqrt(2.0 * math.pi)


def gelu_forward(x):
    x = f64(x)
    er = torch.erf(x * _RSQRT2)
    return dict(y=0.5 * x * (1.0 + er), mag=0.5 * x.abs() * (1.0 + er.abs()), extra=0.5 * x.abs() * E_ERF)


def gelu_backward(x, dy):
    x, dy = f64(x), f64(dy)
    er = torch.erf(x * _RSQRT2)
    xphi = x * _RSQRT2PI * torch.exp(-0.5 * x * x)
    dx = dy * (0.5 * (1.0 + er) + xphi)
    mag = dy.abs() * (0.5 * (1.0 + er.abs()) + xphi.abs())
    extra = dy.abs() * (0.5 * E_ERF + (0.75 * x * x + 3.0) * E * xphi.abs())
    return dict(dx=dx, mag=mag, extra=extra)


def rope_backward(dqkv, cos, sin, B: int, S: int, H: int, hd: int, pos0: int):
    """Transpose of the rotation on the q and k thirds of [B·S, 3·H·hd]; the v third untouched (train.hip:366-389)."""
    d = f64(dqkv)[:, :3 * H * hd].reshape(B, S, 3, H, hd)
    half = hd // 2
    c = f64(cos)[pos0:pos0 + S].view(1, S, 1, 1, half)
    s = f64(sin)[pos0:pos0 + S].view(1, S, 1, 1, half)
    d1, d2 = d[:, :, :2, :, :half], d[:, :, :2, :, half:]
    out, mag = d.clone(), d.abs()
    out[:, :, :2, :, :half], out[:, :, :2, :, half:] = d1 * c + d2 * s, d2 * c - d1 * s
    mag[:, :, :2, :, :half], mag[:, :, :2, :, half:] = (d1 * c).abs() + (d2 * s).abs(), (d2 * c).abs() + (d1 * s).abs()
    return out.reshape(B * S, 3 * H * hd), mag.reshape(B * S, 3 * H * hd)


def cross_entropy(logits, targets, ignore_index: int = -100):
    """dlogits = (softmax − onehot)/n_valid (0 on ignored rows) with mag = (p + onehot)/n_valid, and the forward's mean
    loss over the valid rows with its companion, and the count; `loss` / `lmag` are the per-row terms that mean and
    m_mean average (0 on ignored rows)."""
    lg, tg = f64(logits), targets.detach().cpu().long()
    rows, n = lg.shape
    valid = tg != ignore_index
    nv = int(valid.sum().item())
    dl, mag = torch.zeros_like(lg), torch.zeros_like(lg)
    loss = torch.zeros(rows, dtype=torch.float64)
    lmag = torch.zeros(rows, dtype=torch.float64)
    for s in _slices(rows, n):
        l, t, v = lg[s], tg[s], valid[s]
        mx = l.amax(-1, keepdim=True)
        ex = torch.exp(l - mx)
        sm = ex.sum(-1, keepdim=True)
        p = ex / sm
        oh = torch.zeros_like(p)
        tc = torch.where(v, t, torch.zeros_like(t))
        oh.scatter_(1, tc.view(-1, 1), 1.0)
        vv = v.view(-1, 1).double()
        dl[s], mag[s] = vv * (p - oh) / max(nv, 1), vv * (p + oh) / max(nv, 1)
        lt = l.gather(1, tc.view(-1, 1))
        loss[s] = (v.double() * (torch.log(sm) + mx - lt).squeeze(-1))
        lmag[s] = (v.double() * (1.0 + torch.log(sm).abs() + mx.abs() + lt.abs()).squeeze(-1))
    return dict(dl=dl, mag=mag, mean=loss.sum() / max(nv, 1), m_mean=lmag.sum() / max(nv, 1), count=nv, loss=loss, lmag=lmag)


def gemm_tn(P, Q, alpha: float):
    """alpha·PᵀQ [R, N] and |alpha|·|P|ᵀ|Q| (alpha is the fp32 value the kernel receives)."""
    P, Q = f64(P), f64(Q)
    a = float(torch.tensor(alpha, dtype=torch.float32))
    return a * (P.t() @ Q), abs(a) * (P.abs().t() @ Q.abs())


def embed_backward(ids, dx, dw0, n_patches: int):
    """dW[ids[b, j]] += dx[b, row(j)], row(0) = 0, row(j) = j + n_patches (train.hip:855). Returns dw, mag, hits per row."""
    ids, dx, dw = ids.detach().cpu().long(), f64(dx), f64(dw0).clone()
    B, L = ids.shape
    rowsel = torch.tensor([0] + [j + n_patches for j in range(1, L)])
    src = dx[:, rowsel].reshape(B * L, -1)
    mag = dw.abs()
    dw.index_add_(0, ids.reshape(-1), src)
    mag.index_add_(0, ids.reshape(-1), src.abs())
    hits = torch.zeros(dw.shape[0], dtype=torch.float64).index_add_(0, ids.reshape(-1), torch.ones(B * L, dtype=torch.float64))
    return dw, mag, hits


def sumsq(g):
    """Σ g² (its own magnitude companion: every term is non-negative)."""
    return (f64(g) ** 2).sum()


def clip_coef(norm: float, max_norm: float) -> float:
    return min(1.0, float(torch.tensor(max_norm, dtype=torch.float32)) / (norm + float(torch.tensor(1e-6, dtype=torch.float32))))


def adamw_step(p, m, v, g, step: int, lr: float, beta1: float, beta2: float, eps: float, wd: float, coef: float = 1.0,
               coupled: bool = False):
    """One torch.optim.AdamW step (decoupled weight decay) in fp64 on the fp32 hyper-parameters the kernel receives.
    `coupled` adds wd·p to the gradient instead (the WRONG algorithm of the CPU test). Returns p, m, v and companions."""
    f = lambda a: float(torch.tensor(a, dtype=torch.float32))
    lr, beta1, beta2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    p, m, v, g = f64(p), f64(m), f64(v), f64(g)
    gi = g * coef
    if coupled:
        gi = gi + wd * p
    p0 = p if coupled else p * (1.0 - lr * wd)
    mn = beta1 * m + (1.0 - beta1) * gi
    m_m = (beta1 * m).abs() + ((1.0 - beta1) * gi).abs()
    vn = beta2 * v + (1.0 - beta2) * gi * gi
    bc1, bc2s = 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)
    denom = torch.sqrt(vn) / bc2s + eps
    pn = p0 - (lr / bc1) * (mn / denom)
    m_p = p.abs() + (lr / bc1) * (m_m / denom)
    return dict(p=pn, m=mn, v=vn, m_p=m_p, m_m=m_m, m_v=vn)


# ---- comparators ------------------------------------------------------------------------------------------------------
def _log(what: str, ratio: float, n: int) -> None:
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print(f"train_ref64: {what}: max err/bound {ratio:.4f} over {n} elements")


def _compare(got, ref, bound, what: str) -> float:
    got = f64(got)
    ref = ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio_t = err / bound
    ratio = float(ratio_t.max().item()) if err.numel() else 0.0
    _log(what, ratio, err.numel())
    bad = ratio_t > 1.0
    if bool(bad.any()):
        i = int(torch.argmax(ratio_t.reshape(-1)).item())
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio_t.shape)) if ratio_t.dim() else ()
        raise AssertionError(f"{what}: {int(bad.sum().item())} of {err.numel()} elements out of bound; worst at {idx}: got "
                             f"{got.reshape(-1)[i].item():.9g}, ref {ref.reshape(-1)[i].item():.9g}, bound "
                             f"{bound.reshape(-1)[i].item():.4g}, err/bound {ratio:.4g}")
    return ratio


def _bound(ref, mag, c, tie, extra, rel: float):
    b = rel * ref.abs() + c * E * mag + FLOOR
    if tie is not None:
        b = b + tie
    if extra is not None:
        b = b + extra
    return b


def assert_bf16_close(got, ref, mag, c, what: str, tie=None, extra=None) -> float:
    """|got − ref| <= u·|ref| + c·e·mag + tie + extra + FLOOR on every element (c a number or a tensor)."""
    return _compare(got, ref, _bound(ref.double(), mag.double(), c, tie, extra, U), what)


def assert_f32_close(got, ref, mag, c, what: str, tie=None, extra=None) -> float:
    """|got − ref| <= c·e·mag + tie + extra + FLOOR on every element."""
    return _compare(got, ref, _bound(ref.double(), mag.double(), c, tie, extra, 0.0), what)


def grad_close_accepts(got, ref, tol: float = 2e-2) -> bool:
    """The whole-tensor yardstick of tests/test_train_ops_gpu.py (max|got − ref| <= tol·max|ref|), as a predicate."""
    got, ref = f64(got), ref.double()
    return bool((got - ref).abs().max().item() <= tol * (ref.abs().max().item() + 1e-30))


# ---- whole-op checks shared by the CPU and the GPU tests ------------------------------------------------------------------
def check_norm_backward(what: str, ref, ln: bool, rpb: int, nblk: int, dx=None, dw=None, db=None) -> None:
    depth = reduce_depth(rpb // 4, nblk)
    if dx is not None:
        assert_bf16_close(dx, ref["dx"], ref["m_dx"], C_NORM_DX, f"{what} dx")
    if dw is not None:
        if ln:
            assert_f32_close(dw, ref["dw"], ref["m_dw"], C_XHAT_LN + 1 + depth, f"{what} dw")
        else:
            assert_f32_close(dw, ref["dw"], ref["m_dw"], 2 + depth, f"{what} dw", tie=ref["tie_dw"])
    if db is not None:
        assert_f32_close(db, ref["db"], ref["m_db"], depth, f"{what} db")


def check_swiglu_backward(what: str, ref, dgu) -> None:
    assert_bf16_close(dgu, ref["dgu"], ref["mag"], ref["c"], what, tie=ref["tie"], extra=ref["extra"])
