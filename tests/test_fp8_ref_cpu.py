"""The e4m3 reference and its checks (tests/fp8_ref64.py) tell right from wrong, on the CPU.

* The case tables and input builders of tests/test_fp8_ref_gpu.py live here (the GPU module imports them); the exactness
  condition of every integer and selector case is asserted.
* The encoder equals torch's e4m3fn cast on [-448, 448] (every midpoint between adjacent finite values and its fp32
  neighbours, every bf16 value, random fp32 values), the decode table equals torch's on every finite code, and the layout
  definition agrees with ops.unpack_weight on bf16 pairs (tests/test_fp8_ref_gpu.py states the same of ops.pack_weight).
* A torch emulation of the kernels' arithmetic passes every checker; each wrong algorithm of WRONG_GEMM / WRONG_QUANT,
  run through the same emulation against the same checkers, is rejected.
"""
import pytest
import torch

import fp8_ref64 as F
import gemm_ref64 as G
from fp8_ref64 import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_RES, EPI_SWIGLU
from test_gemm_ref_cpu import _erf_gelu, rbf

f32 = torch.float32
BF16_MAX = 3.3895313892515355e38

# ---- the GPU module's cases ------------------------------------------------------------------------------------------------
INT_SHAPES = [
    (1, 16, 128),          # smallest problem
    (256, 256, 256),       # one interior tile: straight-line epilogue, 16-byte stores
    (300, 528, 384),       # ragged both ways, 3 K-tiles, a 2 x 3 tile grid
    (257, 272, 640),       # one row and one column group into the second tile, 5 K-tiles
    (2344, 512, 128),      # 10 tile rows (a full group of 8 and a group of 2); 20 workgroups, not a multiple of 8
    (768, 1024, 1152),     # all-interior, 12 workgroups, 9 K-tiles
    (256, 256, 11008),     # 86 K-tiles, the down-projection depth
]
SCALE_KINDS = ("pow2", "real")
SELECTOR_SHAPES = [(254, 256, 256), (254, 272, 384)]
GAUSS_SHAPES = [s for s in INT_SHAPES if s[2] <= F.GAUSS_KMAX]
QROWS_COLS = (8, 520, 4096, 4104, 5632, 5640, 12288, 12296, 13824, 13832, 22016, 22024, 27648, 27656)
QROWS_ROWS = 6
COLAMAX_ROWS = (1, 3, 4, 13, 16, 17, 255, 256, 257, 529)
COLAMAX_COLS = (8, 504, 520)
TQ_TOKENS = (1, 63, 64, 65, 255, 257, 300)
TQ_COLS = (16, 48, 64, 80, 208)
TQ_ZERO_CH, TQ_TINY_CH = 5, 9
TINY_AMAX = (1e-37, 2.0 ** -130, 2.0 ** -101, 2.0 ** -100)     # 448 / amax = inf; a bf16 subnormal; just below / at the threshold


def gemm_operands(M, N, K, kind, seed=0):
    """Integer instrument: (A8 [M, K], W8 [N, K], sa [M], sw [N]) on the CPU. Distinct, non-symmetric scale vectors."""
    A8, W8 = F.integer_codes((M, K), 1000 + seed, F.A_IMAX), F.integer_codes((N, K), 2000 + seed, F.W_IMAX)
    if kind == "pow2":
        return A8, W8, F.pow2_scales(M, 3000 + seed, *F.POW2_A), F.pow2_scales(N, 4000 + seed, *F.POW2_W)
    return A8, W8, F.real_scales(M, 3000 + seed, 30.0), F.real_scales(N, 4000 + seed, 10.0)


def tie_values():
    """bf16 values that are exact midpoints between adjacent e4m3 values (for amax = 448: inv = 1), 448 and -0.0 first."""
    pos = F.DECODE[:127]
    mids = (pos[:-1] + pos[1:]) / 2
    sign = torch.where(torch.arange(126) % 2 == 0, 1.0, -1.0).double()
    head = torch.tensor([448.0, -0.0, mids[0], -mids[1], mids[6], -mids[7], mids[8], -448.0], dtype=torch.float64)
    v = torch.cat([head, mids * sign, -mids * sign])
    assert torch.equal(v.to(torch.bfloat16).double(), v)
    return v


def qrows_input(cols, idx):
    """The six rows of a bl_quantize_rows_fp8 case, fp32 holding bf16 values."""
    g = torch.Generator().manual_seed(900 + cols)
    x = torch.zeros(QROWS_ROWS, cols, dtype=torch.float64)
    mant = torch.randn(cols, generator=g, dtype=torch.float64)
    x[0] = (mant * 10.0 ** torch.linspace(-30.0, 38.4, cols, dtype=torch.float64)).clamp(-BF16_MAX, BF16_MAX)
    x[0, 3] = BF16_MAX                                              # magnitudes from 1e-30 to bf16's largest finite value
    # row 1 stays zero
    x[2] = torch.randn(cols, generator=g, dtype=torch.float64).clamp(-3, 3)
    x[2, cols - 3] = 7.0                                            # the only maximum sits in the last 8-column chunk
    x[3] = torch.randn(cols, generator=g, dtype=torch.float64).clamp(-3, 3)
    x[3, 2] = -7.0                                                  # … in the first
    t = tie_values()
    x[4] = t.repeat((cols + t.numel() - 1) // t.numel())[:cols]     # amax = 448: rounding ties, subnormal ties, -0.0
    a = TINY_AMAX[idx % len(TINY_AMAX)]
    x[5, 0::3] = a * 0.5
    x[5, 6::9] = -a * 0.25
    x[5, 1] = -a                                                    # the tiny-amax row: zeros between tiny values
    out = x.to(torch.bfloat16).float()
    assert bool(torch.isfinite(out).all()) and float(out[5].abs().max()) == float(torch.tensor(a).to(torch.bfloat16))
    return out


def colamax_input(rows, cols):
    """Column c carries its maximum in row c mod rows (negative in odd columns), every other entry is strictly smaller;
    column 5 is all zero."""
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, cols, generator=g).clamp(-1, 1)
    c = torch.arange(cols)
    x[c % rows, c] = (2.0 + (c % 7) * 0.25) * torch.where(c % 2 == 1, -1.0, 1.0)
    x[:, 5] = 0.0
    return x.to(torch.bfloat16).float()


def tq_input(tokens, cols):
    x = G.gauss((tokens, cols), tokens * 1000 + cols) * torch.linspace(0.01, 30.0, cols)
    x[:, TQ_ZERO_CH] = 0.0
    x[:, TQ_TINY_CH] = 0.0
    x[tokens // 2, TQ_TINY_CH] = -1e-37
    return x.to(torch.bfloat16).float()


def tq_ldqs(tokens):
    ldq = (tokens + 63) // 64 * 64
    return (ldq, ldq + 256) if tokens == 65 else (ldq,)


# ---- exactness conditions ------------------------------------------------------------------------------------------------------
def test_integer_condition_holds_for_every_case():
    pmin, pmax = F.POW2_A[0] + F.POW2_W[0], F.POW2_A[1] + F.POW2_W[1]
    for M, N, K in INT_SHAPES:
        F.assert_integer_exact(K, pmin, pmax)
        assert K % 128 == 0 and N % 16 == 0
    with pytest.raises(AssertionError):
        F.assert_integer_exact(2 ** 24 // 48 + 128)
    with pytest.raises(AssertionError):
        F.assert_integer_exact(11008, pmin, pmax + 1)
    A8, W8, sa, sw = gemm_operands(5, 16, 128, "pow2")
    assert float(F.decode(A8).abs().max()) == 8 and float(F.decode(W8).abs().max()) == 6
    assert set(torch.log2(sa[:, None] * sw[None, :]).reshape(-1).tolist()) <= set(range(pmin, pmax + 1))
    for kind in SCALE_KINDS:                                         # distinct, non-symmetric scale vectors
        _, _, sa, sw = gemm_operands(256, 256, 256, kind)
        assert not torch.equal(sa, sw) and bool(torch.isfinite(sa).all()) and bool((sw > 0).all())
    _, _, sa, sw = gemm_operands(256, 256, 256, "real")
    assert len(sa.unique()) > 50 and bool(((sa.view(torch.int32) & 0xFFFF) != 0).any())      # arbitrary fp32 significands
    # any summation order of the integer products is exact in fp32
    K = 11008
    A8, W8, _, _ = gemm_operands(3, 16, K, "pow2")
    a, w = F.decode(A8).float(), F.decode(W8).float()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(8))
    acc = torch.zeros(3, 16, dtype=f32)
    for k0 in range(0, K, 688):
        acc = acc + a[:, perm[k0:k0 + 688]] @ w[:, perm[k0:k0 + 688]].t()
    assert torch.equal(acc.double(), F.acc64(A8, W8))


def test_selector_condition_holds_for_every_case():
    for M, N, K in SELECTOR_SHAPES:
        F.assert_selector_exact(M, N, K)
        assert M != N


# ---- encoder, decoder, layouts --------------------------------------------------------------------------------------------------
def test_decode_table_is_the_format():
    finite = F.FINITE
    assert finite.numel() == 254 and 0x00 in finite.tolist() and 0x80 in finite.tolist()
    assert torch.equal(F.decode(finite), finite.view(torch.float8_e4m3fn).double())
    assert bool(F.DECODE[[0x7F, 0xFF]].isnan().all()) and float(F.DECODE[0x7E]) == 448.0 and float(F.DECODE[0x01]) == 2.0 ** -9
    assert float(F.DECODE[0x08]) == 2.0 ** -6 and float(F.DECODE[0x07]) == 7 * 2.0 ** -9 and bool(torch.isfinite(F.DECODE[finite.long()]).all())


def test_encoder_equals_torch_cast_on_the_finite_range():
    vals = F.decode(F.FINITE).sort().values                          # 254 values, -0 and +0 adjacent
    mids = ((vals[:-1] + vals[1:]) / 2).float()
    assert mids.numel() == 253 and torch.equal(mids.double(), (vals[:-1] + vals[1:]) / 2)
    up, dn = torch.nextafter(mids, torch.tensor(float("inf"))), torch.nextafter(mids, torch.tensor(float("-inf")))
    every_bf16 = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    every_bf16 = every_bf16[torch.isfinite(every_bf16) & (every_bf16.abs() <= 448)]
    g = torch.Generator().manual_seed(1)
    rnd = torch.cat([(torch.rand(200000, generator=g) * 2 - 1) * 448, torch.randn(200000, generator=g) * 2.0 ** -7,
                     torch.randn(100000, generator=g)])
    x = torch.cat([mids, up, dn, vals.float(), every_bf16, rnd, torch.tensor([-0.0, 0.0, 448.0, -448.0])])
    x = x[x.abs() <= 448]
    assert torch.equal(F.encode_rne(x), x.to(torch.float8_e4m3fn).view(torch.uint8))
    assert torch.equal(F.encode_rne(F.decode(F.FINITE).float()), F.FINITE)                     # round trip, both zeros
    # outside torch's domain: saturation, where the cast gives NaN
    big = torch.tensor([448.0001, 464.0, 465.0, 1e30, -3e38], dtype=f32)
    assert F.encode_rne(big).tolist() == [0x7E, 0x7E, 0x7E, 0x7E, 0xFE]
    assert bool(big.to(torch.float8_e4m3fn).float().isnan().any())
    # ties go to the even code
    assert F.encode_rne(torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 1.0625, 1.1875, 7.5 * 2.0 ** -9], dtype=f32)).tolist() == \
        [0x00, 0x02, 0x38, 0x3A, 0x08]


def test_layout_definition_agrees_with_unpack_weight():
    from bridgelang_amd import ops
    g = torch.Generator().manual_seed(2)
    N, K = 48, 256
    codes = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)
    img = F.weight_image(codes)                                       # the independent definition, as bf16 pairs
    assert img.shape == (N // 16, K // 64, 64, 8)
    back = ops.unpack_weight(img).contiguous().view(torch.uint8).view(N, K)
    assert torch.equal(back, codes)
    idx = F.packed_index(N, K)
    assert sorted(idx.reshape(-1).tolist()) == list(range(N * K))     # a bijection
    assert int(idx[17, 64 + 35]) == (((1 * 4 + 1) * 64) + (1 + 16 * 2)) * 16 + 3


# ---- a torch emulation of the kernels, right and wrong ------------------------------------------------------------------------------
def _kperm():
    """The k order one MFMA sees inside a 128-wide step: lane group g supplies k in {16g … 16g+15} ∪ {64+16g …}."""
    return torch.cat([torch.cat([torch.arange(16 * g, 16 * g + 16), torch.arange(64 + 16 * g, 80 + 16 * g)]) for g in range(4)])


def emulate_gemm(epi, Abuf, M, K, W8, sa, sw, bias=None, scale=None, res=None, res_row_mod=0, wrong=None):
    """bl_gemm_fp8 in torch: Abuf is the [M + 3, K + 16] buffer the codes sit in (0x7F elsewhere). Returns the fp32 / bf16 output
    as fp32. `wrong` names one deliberate mistake."""
    A8 = Abuf[:M, :K]
    a, w = F.decode(A8), F.decode(W8)
    N = w.shape[0]
    if wrong == "k-permutation applied to one operand only":
        a = a.view(M, K // 128, 128)[:, :, _kperm()].reshape(M, K)
    if wrong == "last K-tile of an odd count dropped":
        assert (K // 128) % 2 == 1
        a, w = a[:, :K - 128], w[:, :K - 128]
    acc = a @ w.t()                                                   # exact (integer or single products)
    if wrong == "phantom tile read as real data":
        flat, lda = F.decode(Abuf.reshape(-1)), Abuf.shape[1]
        ph = torch.stack([flat[m * lda + K:m * lda + K + 128] for m in range(M)])
        acc = acc + ph @ w[:, :128].t()
    acc = acc.float()
    sa_, sw_ = sa, sw
    if wrong == "sa and sw exchanged":
        sa_, sw_ = sw[torch.arange(M) % N], sa[torch.arange(N) % M]
    if wrong == "scales applied after the bias":
        acc = acc + bias[None, :]
    if wrong == "one fp32 multiply by fl32(sa*sw)":
        x = acc * (sa_[:, None] * sw_[None, :])
    elif wrong == "multiplied by sa first":
        x = (acc * sa_[:, None]) * sw_[None, :]
    else:
        x = (acc * sw_[None, :]) * sa_[:, None]
    if epi == EPI_F32:
        return x
    if epi in (EPI_F32_BF16R, EPI_NONE):
        return rbf(x)
    if epi == EPI_SWIGLU:
        t = rbf(x)
        gt, u = t[:, 0::2], t[:, 1::2]
        return rbf(rbf(gt * torch.sigmoid(gt)) * u)
    v = x + bias if epi in G.HAS_BIAS and wrong != "scales applied after the bias" else x
    if epi == EPI_BIAS:
        return rbf(v)
    if epi == EPI_BIAS_GELU:
        return rbf(_erf_gelu(rbf(v)))
    v = rbf(v)
    if scale is not None:
        v = rbf(v * scale)
    rows = torch.arange(M) % res_row_mod if res_row_mod else torch.arange(M)
    return rbf(v + res[rows][:, :N])


def _gemm_case(kind, M=45, N=96, K=384):
    A8, W8, sa, sw = gemm_operands(M, N, K, kind, seed=7)
    Abuf = torch.full((M + 3, K + 16), 0x7F, dtype=torch.uint8)
    Abuf[:M, :K] = A8
    return dict(Abuf=Abuf, A8=A8, W8=W8, sa=sa, sw=sw, M=M, N=N, K=K, bias=G.dyadic_add((N,), 11), ls=G.layerscale(N, 12),
                res=G.dyadic_add((M, N), 13), table=G.dyadic_add((7, N), 14))


def _run_and_check(c, epi, wrong=None, scale=None, res=None, res_row_mod=0):
    kw = dict(bias=c["bias"] if epi in G.HAS_BIAS else None, scale=scale, res=res, res_row_mod=res_row_mod)
    got = emulate_gemm(epi, c["Abuf"], c["M"], c["K"], c["W8"], c["sa"], c["sw"], wrong=wrong,
                       **{**kw, "bias": c["bias"]})
    F.check_gemm(f"cpu emulation {G.EPI_NAMES[epi]} {wrong or 'right'}", epi, c["A8"], c["W8"], c["sa"], c["sw"], got, **kw)


@pytest.mark.parametrize("kind", SCALE_KINDS)
def test_emulation_passes_every_epilogue(kind):
    c = _gemm_case(kind)
    for epi in (EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_SWIGLU):
        _run_and_check(c, epi)
    _run_and_check(c, EPI_RES, res=c["res"])
    _run_and_check(c, EPI_BIAS_RES, res=c["res"])
    _run_and_check(c, EPI_BIAS_RES, res=c["res"], scale=c["ls"])
    _run_and_check(c, EPI_BIAS_RES, res=c["table"], scale=c["ls"], res_row_mod=7)
    for M, N, K in SELECTOR_SHAPES:
        A8, W8 = F.selector_case(M, N, K)
        Abuf = torch.full((M + 3, K + 16), 0x7F, dtype=torch.uint8)
        Abuf[:M, :K] = A8
        sa, sw = F.pow2_scales(M, 5, -2, 2), F.pow2_scales(N, 6, -3, 1)
        F.check_gemm("cpu emulation selector", EPI_F32, A8, W8, sa, sw, emulate_gemm(EPI_F32, Abuf, M, K, W8, sa, sw))


def test_pow2_scales_make_the_epilogue_adds_exact():
    """With power-of-two scales every linear epilogue equals the fp64 value: the fp32 roundings of the reference are the identity."""
    c = _gemm_case("pow2")
    x = F.acc64(c["A8"], c["W8"]) * c["sa"].double()[:, None] * c["sw"].double()[None, :]
    assert torch.equal(F.dequant(F.acc64(c["A8"], c["W8"]), c["sa"], c["sw"]), x)
    t = x + c["bias"].double()
    assert torch.equal(t.float().double(), t)
    assert torch.equal(G.linear_ref(EPI_BIAS, x, c["bias"]), F.rb64(t))
    c = _gemm_case("real")                                           # and with arbitrary scales they are not
    x = F.dequant(F.acc64(c["A8"], c["W8"]), c["sa"], c["sw"])
    t = x + c["bias"].double()
    assert not torch.equal(t.float().double(), t)


WRONG_GEMM = {
    "k-permutation applied to one operand only": EPI_F32,
    "last K-tile of an odd count dropped": EPI_F32,
    "phantom tile read as real data": EPI_F32,
    "sa and sw exchanged": EPI_F32,
    "multiplied by sa first": EPI_F32,
    "scales applied after the bias": EPI_BIAS,
    "one fp32 multiply by fl32(sa*sw)": EPI_F32,
}


@pytest.mark.parametrize("wrong", list(WRONG_GEMM))
def test_wrong_gemm_algorithms_are_rejected(wrong):
    c = _gemm_case("real")
    with pytest.raises(AssertionError):
        _run_and_check(c, WRONG_GEMM[wrong], wrong=wrong)
    if wrong in ("k-permutation applied to one operand only", "last K-tile of an odd count dropped", "phantom tile read as real data"):
        M, N, K = SELECTOR_SHAPES[1]                                   # the selector instrument rejects them too
        A8, W8 = F.selector_case(M, N, K)
        Abuf = torch.full((M + 3, K + 16), 0x7F, dtype=torch.uint8)
        Abuf[:M, :K] = A8
        sa, sw = F.pow2_scales(M, 5, -2, 2), F.pow2_scales(N, 6, -3, 1)
        with pytest.raises(AssertionError):
            F.check_gemm("cpu selector " + wrong, EPI_F32, A8, W8, sa, sw, emulate_gemm(EPI_F32, Abuf, M, K, W8, sa, sw, wrong=wrong))


def test_gauss_check_rejects_one_average_product():
    """Whatever the measured constant, the bound it may take (1 / (8 K)) rejects one dropped or duplicated average product,
    and accepts an fp32 evaluation in another order."""
    M, N, K = 40, 48, 1152
    g = G.gauss((M, K), 20), G.gauss((N, K), 21, K ** -0.5)
    (A8, sa, _), (W8, sw, _) = F.quantize_spec(g[0]), F.quantize_spec(g[1])
    bound = 1.0 / (8 * K)
    s = sa.double()[:, None] * sw.double()[None, :]
    x, mag = F.acc64(A8, W8) * s, F.acc_mag(A8, W8) * s
    F.check_gauss("cpu gauss fp32", EPI_F32, A8, W8, sa, sw, (F.decode(A8).float() @ F.decode(W8).float().t()) * sw[None, :] * sa[:, None],
                  bound=bound)
    for sign in (-1.0, 1.0):
        with pytest.raises(AssertionError):
            F.check_gauss("cpu gauss, one average product off", EPI_F32, A8, W8, sa, sw, x + sign * mag / K, bound=bound)
    if F.GAUSS_ERR_MAG_BOUND is not None:
        F.assert_gauss_bound_sharp(max(K for _, _, K in GAUSS_SHAPES))


# ---- quantisers ------------------------------------------------------------------------------------------------------------------
def emulate_quantize_rows(x, wrong=None, amax=None):
    """bl_quantize_rows_fp8 in torch (fp32 on the CPU), with torch's cast standing in for the hardware conversion."""
    if amax is None:
        seen = torch.cat([x[:, :-8], torch.zeros(x.shape[0], 1)], 1) if wrong == "amax misses the last 8-column chunk" else x
        amax = seen.abs().amax(dim=1)
    live = amax >= 2.0 ** -100
    safe = torch.where(live, amax, torch.ones_like(amax))
    inv = torch.where(live, torch.full_like(amax, 448.0) / safe, torch.ones_like(amax))
    scale = torch.where(live, safe / 448.0, torch.ones_like(amax))
    y = (x * inv[:, None]).clamp(-448, 448)
    if wrong is None or wrong.startswith("amax"):
        return y.to(torch.float8_e4m3fn).view(torch.uint8), scale
    pos = F.DECODE[:127]
    a = y.double().abs()
    i = (torch.searchsorted(pos, a.contiguous(), right=True) - 1).clamp(0, 126)
    if wrong == "ties away from zero":
        j = (i + 1).clamp(max=126)
        i = torch.where((pos[j] - a <= a - pos[i]) & (j > i), j, i)
    else:
        assert wrong == "truncation instead of RNE"
    return (i | (torch.signbit(y).long() << 7)).to(torch.uint8), scale


@pytest.mark.parametrize("cols", (8, 520, 4104))
def test_quantiser_emulation_passes_and_wrong_ones_are_rejected(cols):
    for idx in range(len(TINY_AMAX)):
        x = qrows_input(cols, idx)
        q, s = emulate_quantize_rows(x)
        F.check_quantize_rows("cpu quantise rows", x, q, s)
        assert s[1] == 1 and s[5] == (1 if idx < 3 else TINY_AMAX[3] / 448) and s[4] == 1 and not q[1].any()
        assert bool((F.decode(q[5]) == 0).all()) == (idx < 3)
    for wrong in ("truncation instead of RNE", "ties away from zero", "amax misses the last 8-column chunk"):
        with pytest.raises(AssertionError):
            F.check_quantize_rows("cpu wrong: " + wrong, x, *emulate_quantize_rows(x, wrong))
    # ties alone tell ties-away from RNE: without row 4 that mistake passes on this data or fails by luck, with it it must fail
    with pytest.raises(AssertionError):
        F.check_quantize_rows("cpu wrong: ties away, tie row", x[4:5], *emulate_quantize_rows(x[4:5], "ties away from zero"))


def test_parent_rule_writes_nan_codes_for_a_tiny_amax():
    """What the quantisers did before the tiny-amax rule, in fp32: 448 / amax = inf, 0·inf = NaN."""
    x = qrows_input(520, 0)[5:6]
    amax = x.abs().amax(dim=1)
    inv = torch.full_like(amax, 448.0) / amax
    assert bool(torch.isinf(inv).all()) and bool((x * inv[:, None]).isnan().any())
    q, s, live = F.quantize_spec(x)
    assert not bool(live.any()) and float(s) == 1.0 and bool((q & 0x7F == 0).all())


def test_quantize_weight_rule_on_cpu():
    """ops.quantize_weight_fp8 divides by the scale where the kernels multiply by its inverse; the zero-row rule is the same."""
    w = qrows_input(520, 0)
    amax = w.abs().amax(dim=1)
    scale, _, live = F.scales_spec(amax)
    q = (w / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    F.check_quantised("cpu quantise weight", w, q, scale)
    assert live.tolist() == [True, False, True, True, True, False]


def test_colamax_check_rejects_a_skipped_row():
    for rows in (3, 17, 257):
        x = colamax_input(rows, 520)
        F.check_colamax("cpu colamax", x, x.abs().amax(dim=0))
        assert float(x.abs().amax(dim=0)[5]) == 0.0
        for skip in (0, rows // 2, rows - 1):
            keep = torch.ones(rows, dtype=torch.bool)
            keep[skip] = False
            with pytest.raises(AssertionError):
                F.check_colamax("cpu wrong: one row skipped", x, x[keep].abs().amax(dim=0))


def emulate_transpose_quantize(x, amax, ldq, packed, wrong=None):
    T_, C_ = x.shape
    q, s = emulate_quantize_rows(x.t().contiguous(), amax=amax)
    rows = torch.full((C_, ldq), 0x55 if wrong == "token tail left unpadded" else 0, dtype=torch.uint8)
    rows[:, :T_] = q
    if not packed:
        return rows.reshape(-1), s
    ch, tok = torch.arange(C_)[:, None], torch.arange(ldq)[None, :]
    lane, byte = ch % 16 + 16 * ((tok % 64) // 16), tok % 16
    blk = (ch // 16) * (ldq // 64) + tok // 64
    idx = (blk * 16 + byte) * 64 + lane if wrong == "lane and byte exchanged" else (blk * 64 + lane) * 16 + byte
    out = torch.empty(C_ * ldq, dtype=torch.uint8)
    out[idx.reshape(-1)] = rows.reshape(-1)
    return out, s


@pytest.mark.parametrize("tokens,cols", [(65, 48), (300, 208), (1, 16)])
def test_transposing_quantiser_emulation_and_wrong_layouts(tokens, cols):
    x = tq_input(tokens, cols)
    amax = x.abs().amax(dim=0)
    for ldq in tq_ldqs(tokens):
        for packed in (False, True):
            q, s = emulate_transpose_quantize(x, amax, ldq, packed)
            F.check_transpose_quantize("cpu transposing quantiser", x, amax, q, s, ldq, packed)
            assert s[TQ_ZERO_CH] == 1 and s[TQ_TINY_CH] == 1
            if tokens < ldq:
                with pytest.raises(AssertionError):
                    F.check_transpose_quantize("cpu wrong: tail", x, amax, *emulate_transpose_quantize(x, amax, ldq, packed, "token tail left unpadded"),
                                               ldq, packed)
        with pytest.raises(AssertionError):
            F.check_transpose_quantize("cpu wrong: lane/byte", x, amax, *emulate_transpose_quantize(x, amax, ldq, True, "lane and byte exchanged"),
                                       ldq, True)
