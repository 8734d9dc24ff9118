"""The e4m3 family of csrc/gemm_fp8.hip, per element, against the exact reference of tests/fp8_ref64.py: bl_gemm_fp8 under
every epilogue its entry point accepts, bl_quantize_rows_fp8 in its seven instantiations, bl_colamax_bf16 and
bl_transpose_quantize_fp8 in both layouts. The case tables and input builders live in tests/test_fp8_ref_cpu.py, which
asserts every exactness condition and shows the checkers reject wrong algorithms without a GPU.

Composition. No exact end-to-end weight-gradient case is run: lossless quantisation and exact summation cannot hold
together. Exact codes, scales and layouts from the quantisers (test_quantize_rows, test_transpose_quantize) plus the exact
GEMM on arbitrary codes (test_gemm_integer, test_gemm_selector) compose to it.

Scaffolding as in tests/test_gemm_ref_gpu.py (Buf is imported from there). Outputs are the logical corner of a NaN-filled
buffer with ldc = n_out + 12 and three extra rows: everything outside must still be NaN, everything inside finite. A8 sits
in a [M + 3, K + 16] buffer filled with the NaN code 0x7F, scale_a is followed by NaN sentinels, the residual has its own
padded buffer. The quantisers write into buffers filled with 0x55 / NaN whose padding must be untouched. The GEMM operand
W8 is built from the codes by the layout definition of fp8_ref64.py, not by ops.pack_weight (test_layout_agrees_with_pack_weight
states once that the two agree). References and comparisons of the GEMM run on the device.

Gaussian instrument: the worst err / mag over the EPI_F32 cases was measured on an MI355X at GAUSS_ERR_MAG_MEASURED (see
fp8_ref64.py); 4× that is asserted and stays below 1 / (8·1152), the weight of one average product at the largest Gaussian K.
"""
import pytest
import torch

import fp8_ref64 as F
import gemm_ref64 as G
import train_ref64 as T64
from fp8_ref64 import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_RES, EPI_SWIGLU
from test_fp8_ref_cpu import (COLAMAX_COLS, COLAMAX_ROWS, GAUSS_SHAPES, INT_SHAPES, QROWS_COLS, QROWS_ROWS, SCALE_KINDS, SELECTOR_SHAPES,
                              TQ_COLS, TQ_TINY_CH, TQ_TOKENS, TQ_ZERO_CH, colamax_input, gemm_operands, qrows_input, tq_input, tq_ldqs)
from test_gemm_ref_gpu import OUT_MAP, RES_MOD, Buf

pytestmark = pytest.mark.gpu
NAN = float("nan")
bf16, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
CANARY = 0x55


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


# ---- operands ----------------------------------------------------------------------------------------------------------------
class Operands:
    """A8 in its 0x7F-filled [M + 3, K + 16] buffer, scale_a followed by NaN sentinels, W8 as the kernel reads it."""

    def __init__(self, dev, A8, W8, sa, sw):
        M, K = A8.shape
        self.M, self.N, self.K = M, W8.shape[0], K
        self.abuf = torch.full((M + 3, K + 16), 0x7F, dtype=u8, device=dev)
        self.A8 = self.abuf[:M, :K]
        self.A8.copy_(A8)
        self.sabuf = torch.full((M + 5,), NAN, dtype=f32, device=dev)
        self.sa = self.sabuf[:M]
        self.sa.copy_(sa)
        self.W8 = W8.to(dev)
        self.Wimg = F.weight_image(self.W8)
        self.sw = sw.to(dev).contiguous()
        with T64.on_device():
            self.x = F.dequant(F.acc64(self.A8, self.W8), self.sa, self.sw)          # fp64 on the device


def run_fp8(ops, dev, o, epi, n=None, *, bias=None, scale=None, res=None, res_row_mod=0, out_map=None, inplace=False):
    """One launch into a fresh NaN buffer. Returns (logical output as fp64 on the device, kept logical rows)."""
    n = o.N if n is None else n
    odt = f32 if epi in (EPI_F32, EPI_F32_BF16R) else bf16
    n_out = n // 2 if epi == EPI_SWIGLU else n
    kept, orows = G.out_rows(o.M, out_map, dev)
    nrows = o.M if out_map is None else ((o.M + out_map[0] - 1) // out_map[0]) * out_map[1]
    if inplace:
        C = Buf(nrows, n_out, dev, odt, data=res)
        res = C.v
    else:
        C = Buf(nrows, n_out, dev, odt)
    ops.gemm_fp8(o.A8, o.sa, o.Wimg[:n // 16], o.sw[:n], C.v, epi, bias=bias, scale=scale, res=res, res_row_mod=res_row_mod,
                 out_map=out_map)
    return C.take(G.EPI_NAMES[epi], None if out_map is None else orows), kept


# ---- bl_gemm_fp8: integer instrument ----------------------------------------------------------------------------------------------
INT_CASES = [(M, N, K, kind) for M, N, K in INT_SHAPES for kind in SCALE_KINDS]


@pytest.mark.parametrize("M,N,K,kind", INT_CASES, ids=[f"{M}x{N}x{K}-{kind}" for M, N, K, kind in INT_CASES])
def test_gemm_integer(dev, M, N, K, kind):
    from bridgelang_amd import ops
    F.assert_integer_exact(K)
    o = Operands(dev, *gemm_operands(M, N, K, kind))
    bias = G.dyadic_add((N,), 102).to(dev).to(bf16)
    ls = G.layerscale(N, 103).to(dev).to(bf16)
    res = Buf(M, N, dev, data=G.dyadic_add((M, N), 104))
    table = Buf(RES_MOD, N, dev, data=G.dyadic_add((RES_MOD, N), 105))

    def case(epi, **kw):
        what = f"fp8 {kind} {G.EPI_NAMES[epi]}" + "".join(f" {k}" for k in kw if k in ("scale", "out_map", "inplace"))
        b = bias if epi in G.HAS_BIAS else None
        C, kept = run_fp8(ops, dev, o, epi, bias=b, **kw)
        r = kw.get("res")
        if r is not None:                                              # gather the residual rows the kept output rows read
            r = r.double()[kept % kw["res_row_mod"] if kw.get("res_row_mod") else kept]
        F.check_gemm(what, epi, o.A8, o.W8, o.sa, o.sw, C, bias=b, scale=kw.get("scale"), res=r, x=o.x[kept])
        return C

    for epi in (EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_BIAS, EPI_BIAS_GELU):
        case(epi)
    plain = case(EPI_RES, res=res.v)
    assert torch.equal(case(EPI_RES, res=res.v.clone(), inplace=True), plain), "in-place residual differs"
    case(EPI_BIAS_RES, res=res.v)
    case(EPI_BIAS_RES, res=res.v, scale=ls)
    case(EPI_BIAS_RES, res=table.v, scale=ls, res_row_mod=RES_MOD, out_map=OUT_MAP)
    if N % 32 == 0:
        case(EPI_SWIGLU)
    assert bool(o.sabuf[M:].isnan().all()) and bool((o.abuf[M:] == 0x7F).all()) and bool((o.abuf[:, K:] == 0x7F).all())


@pytest.mark.parametrize("M,N,K", [(1, 16, 128), (300, 528, 384)], ids=["1x16x128", "300x528x384"])
def test_gemm_reports_its_form(dev, M, N, K):
    """bl_gemm_fp8 goes through the planner and the launcher of the bf16 entry points: bl_gemm_last_form names its one form,
    not the form of the bf16 call before it."""
    from bridgelang_amd import ops
    a = torch.zeros(64, 64, dtype=bf16, device=dev)
    ops.gemm(a, ops.pack_weight(a), torch.empty(64, 64, dtype=bf16, device=dev), ops.EPI_NONE)
    assert ops.gemm_last_form() == "gemm128"
    o = Operands(dev, *gemm_operands(M, N, K, "pow2"))
    C, _ = run_fp8(ops, dev, o, EPI_F32)
    assert ops.gemm_last_form() == "gemm256s_fp8"
    F.check_gemm("fp8 form f32", EPI_F32, o.A8, o.W8, o.sa, o.sw, C, x=o.x)


# ---- selector instrument ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", SELECTOR_SHAPES, ids=[f"{M}x{N}x{K}" for M, N, K in SELECTOR_SHAPES])
def test_gemm_selector(dev, M, N, K):
    from bridgelang_amd import ops
    A8, W8 = F.selector_case(M, N, K)
    o = Operands(dev, A8, W8, F.pow2_scales(M, 5, -2, 2), F.pow2_scales(N, 6, -3, 1))
    C, _ = run_fp8(ops, dev, o, EPI_F32)
    F.check_gemm("fp8 selector f32", EPI_F32, o.A8, o.W8, o.sa, o.sw, C, x=o.x)


# ---- Gaussian instrument ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", GAUSS_SHAPES, ids=[f"{M}x{N}x{K}" for M, N, K in GAUSS_SHAPES])
def test_gemm_gauss(dev, M, N, K):
    """Measured on an MI355X: worst err / mag over these cases' EPI_F32 outputs 1.556e-5 (at 2344x512x128; the others 3.6e-6 to
    7.8e-6) = F.GAUSS_ERR_MAG_MEASURED; asserted 4× that, 6.224e-5, which is below 1 / (8·1152) = 1.085e-4."""
    from bridgelang_amd import ops
    a, w = G.gauss((M, K), 200).to(dev).to(bf16), G.gauss((N, K), 201, K ** -0.5).to(dev).to(bf16)
    A8, sa, _ = ops.quantize_rows_fp8(a)
    W8, sw, _ = ops.quantize_rows_fp8(w)
    o = Operands(dev, A8, W8, sa, sw)
    bias = G.gauss((N,), 202).to(dev).to(bf16)
    res = Buf(M, N, dev, data=G.gauss((M, N), 203))
    C, _ = run_fp8(ops, dev, o, EPI_F32)
    with T64.on_device():
        print(f"fp8 gauss {M}x{N}x{K}: worst err/mag {F.gauss_err_mag(o.A8, o.W8, o.sa, o.sw, C):.4g}")
    F.assert_gauss_bound_sharp(K)
    F.check_gauss(f"fp8 gauss f32 {M}x{N}x{K}", EPI_F32, o.A8, o.W8, o.sa, o.sw, C)
    C, _ = run_fp8(ops, dev, o, EPI_BIAS_RES, bias=bias, res=res.v)
    F.check_gauss(f"fp8 gauss bias_res {M}x{N}x{K}", EPI_BIAS_RES, o.A8, o.W8, o.sa, o.sw, C, bias=bias, res=res.v)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def test_layout_agrees_with_pack_weight(dev):
    """The independent layout definition equals ops.pack_weight on the codes viewed as bf16 pairs, and ops.unpack_weight inverts it."""
    from bridgelang_amd import ops
    g = torch.Generator().manual_seed(2)
    N, K = 48, 384
    codes = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32).to(u8).to(dev)
    img = F.weight_image(codes)
    packed = ops.pack_weight(codes.view(bf16).contiguous())
    assert torch.equal(packed.view(torch.int16), img.view(torch.int16))
    assert torch.equal(ops.unpack_weight(img).contiguous().view(u8).view(N, K), codes)


# ---- bl_quantize_rows_fp8 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", QROWS_COLS)
def test_quantize_rows(dev, cols):
    """Codes and scales bit for bit against the specification, the tiny-amax rows included (before the rule the zeros of such
    a row became NaN codes: 448 / amax = inf, 0·inf = NaN; measured on an MI355X at amax = 1e-37 and 2^-130: every code of the row
    0x7F / 0xFF, nonzero elements included — ±inf converts to NaN, not to ±448 — and scale = amax / 448; 11 of these 14 cases and
    all 7 of test_transpose_quantize failed there)."""
    from bridgelang_amd import ops
    rows = QROWS_ROWS
    x = qrows_input(cols, QROWS_COLS.index(cols))
    X = Buf(rows, cols, dev, pad=8, data=x)
    qbuf = torch.full((rows + 3, cols + 8), CANARY, dtype=u8, device=dev)
    sbuf = torch.full((rows + 3,), NAN, dtype=f32, device=dev)
    ops.quantize_rows_fp8(X.v, q=qbuf[:rows, :cols], scales=sbuf[:rows])
    assert bool((qbuf[rows:] == CANARY).all()) and bool((qbuf[:, cols:] == CANARY).all()), "wrote outside the logical codes"
    assert bool(sbuf[rows:].isnan().all())
    F.check_quantize_rows(f"quantize_rows cols={cols}", x, qbuf[:rows, :cols], sbuf[:rows])
    assert float(sbuf[1]) == 1.0 and not bool(qbuf[1, :cols].any())                  # the zero row


def test_quantize_weight(dev):
    """ops.quantize_weight_fp8 (load-time torch ops) under the same zero-row rule: no NaN code, finite positive scales, scale 1
    and zero codes below the threshold. Its scale is torch's amax / 448 on the device — a multiplication by fl32(1 / 448), within
    an fp32 ulp of the kernels' division, measured one ulp apart on 3 of 16 rows — and its codes divide by that scale, so the
    codes are checked against the scale it returned."""
    from bridgelang_amd import ops
    w = torch.cat([qrows_input(512, i) for i in range(3)])[:16]
    Wp, sw = ops.quantize_weight_fp8(w.to(dev).to(bf16))
    codes = ops.unpack_weight(Wp).contiguous().view(u8).view(16, 512)
    sw = sw.cpu()
    scale, _, live = F.scales_spec(w.abs().amax(dim=1))
    assert bool((sw[~live] == 1).all()) and not bool(live.all())
    assert bool(((sw.view(torch.int32) - scale.view(torch.int32)).abs() <= 1).all()), "quantize_weight scales"
    F.assert_equal_bytes(codes, F.encode_rne(w / sw[:, None]), "quantize_weight codes")
    F.check_quantised("quantize_weight", w, codes, sw)


# ---- bl_colamax_bf16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", COLAMAX_ROWS)
def test_colamax(dev, rows):
    from bridgelang_amd import train_ops
    for cols in COLAMAX_COLS:
        x = colamax_input(rows, cols)
        X = Buf(rows, cols, dev, pad=8, data=x)
        abuf = torch.zeros(cols + 4, dtype=f32, device=dev)
        abuf[cols:] = NAN
        train_ops.colamax(X.v, abuf[:cols])
        assert bool(abuf[cols:].isnan().all())
        F.check_colamax(f"colamax {rows}x{cols}", x, abuf[:cols])


# ---- bl_transpose_quantize_fp8 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", TQ_TOKENS)
def test_transpose_quantize(dev, tokens):
    from bridgelang_amd import train_ops
    for cols in TQ_COLS:
        x = tq_input(tokens, cols)
        X = Buf(tokens, cols, dev, pad=8, data=x)
        amax = x.abs().amax(dim=0)
        amax_d = amax.to(dev)
        for ldq in tq_ldqs(tokens):
            for packed in (False, True):
                qbuf = torch.full((cols * ldq + 256,), CANARY, dtype=u8, device=dev)
                sbuf = torch.full((cols + 4,), NAN, dtype=f32, device=dev)
                train_ops.transpose_quantize_fp8(X.v, amax_d, qbuf[:cols * ldq], sbuf[:cols], ldq, packed)
                what = f"transpose_quantize {tokens}x{cols} ldq={ldq} {'packed' if packed else 'rows'}"
                assert bool((qbuf[cols * ldq:] == CANARY).all()) and bool(sbuf[cols:].isnan().all()), f"{what}: wrote past its output"
                F.check_transpose_quantize(what, x, amax, qbuf[:cols * ldq], sbuf[:cols], ldq, packed)
                assert float(sbuf[TQ_ZERO_CH]) == 1.0 and float(sbuf[TQ_TINY_CH]) == 1.0
