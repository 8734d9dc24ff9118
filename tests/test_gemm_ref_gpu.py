"""Every dispatch form of the bf16 GEMM family, per element, against the fp64 reference of tests/gemm_ref64.py.

Every case asserts the kernel form it means to reach through ops.gemm_last_form() (the host-side record each entry point
sets), and the closing test asserts that the forms this module reached are the full list ALL_FORMS: a new form without a
case fails there, and a heuristic change that moves a case fails in the case. The case tables live in
tests/test_gemm_ref_cpu.py, which checks the dyadic exactness condition for each of them without a GPU.

Scaffolding. Outputs are the [rows, n_out] corner of a NaN-filled buffer with ldc = n_out + 12 (ldc % 8 == 4; n_out + 8
for EPI_SWIGLU_BWD, whose ABI wants ldc % 8 == 0) and three rows beyond the last; after the launch every element outside
the logical output must still be NaN and every element inside finite. A sits in a NaN-filled [M + 3, K + 8] buffer, the
residual in [rows + 3, N + 12]; the workspace is NaN-filled before every form. References and comparisons run on the
device (test_reference_same_on_cpu_and_device checks them against the CPU once).

Form → case (the planners of csrc/gemm_plan.h; tests/test_gemm_plan_cpu.py checks the tables against them on the CPU)
  plan_gemm: TILE_CASES — gemm128 (700 x 272 x 448, 1 x 16 x 64, M = 32); mid<2|4|5, 1|4> unsliced and K-sliced S = 8 / 2 / 4;
      mid2<1>, <2,2>, <4>; ring 160 x 128; ring 128 x 128 K-sliced; gemm288s; gemm256s one partial round, persistent, and
      multi-round with an odd K-tile count; the 64 x 64 / 128 x 64 / 128 x 128 sub-tile tails; the split-K tail; each tail
      behind a persistent walk of the whole rounds
      test_tile_form_dyadic: twelve epilogues, LayerScale, res_row_mod + out_map, in-place residual; bit-exact or bounded
      test_tile_form_gauss: EPI_F32 and EPI_BIAS_RES on full-mantissa operands (K <= 1536)
      (unsliced mid<4|5, ·> exists only for N % 32 != 0, which the SwiGLU epilogues reject: SWIGLU_UNREACHABLE)
  plan_skinny: seven K x five epilogues x M 1, 5, 16 x N 4112 (257 tiles: two per workgroup, one in the last) and 16
      test_skinny_dyadic; fused a_norm through a 0/1 weight and a Gaussian weight      test_skinny_fused_norm
  plan_rows: rows_stream<8,8>, <6,8>, <8,4> + tree, mid<SK=8>, mid<SK=2> + tree x M 1, 17, 96, 128   test_rows_dyadic
  plan_gemm_tn: plain (odd / even K-tiles), persistent, all tiles split, split-K tail                  test_tn_dyadic
  norm_rows_kernel<NCH 1..10, RMS | LN>, rmsnorm_skinny_kernel<KS>                  test_norm_forward, test_rmsnorm_skinny
"""
import pytest
import torch

import gemm_ref64 as G
import train_ref64 as T64
from gemm_ref64 import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_KEEP, EPI_BIAS_RES, EPI_F32, EPI_F32_BF16R, EPI_GELU_BWD, EPI_NONE,
                        EPI_RES, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_SWIGLU_KEEP)
from test_gemm_ref_cpu import NORM_DIMS, NORM_ROWS, ROWS_CASES, SKINNY_K, SKINNY_KS, SKINNY_M, SKINNY_N, TILE_CASES, TN_CASES

pytestmark = pytest.mark.gpu
NAN = float("nan")
bf16, f32 = torch.bfloat16, torch.float32
EPS = 1e-6
OUT_MAP, RES_MOD = (50, 52, 4), 37          # rows 48, 49 of every 50-row group are dropped, rows 0-3 of every 52 stay unwritten
SWIGLU_UNREACHABLE = {"mid<4,1>", "mid<5,1>", "mid<4,4>", "mid<5,4>"}

ALL_FORMS = {
    # plan_gemm
    "gemm128", "mid<2,1>", "mid<2,4>", "mid<4,1>", "mid<5,1>", "mid<4,4>", "mid<5,4>", "mid<2,4>/S8", "mid<4,4>/S2", "mid<5,4>/S4",
    "mid2<1>", "mid2<2,2>", "mid2<4>", "ring160x128", "ring128x128/S8", "gemm288s", "gemm256s", "gemm256s_persistent",
    "gemm256s+tail64x64", "gemm256s+tail128x64", "gemm256s+tail128x128", "gemm256s+splitk2",
    "gemm256s_persistent+tail64x64", "gemm256s_persistent+tail128x64", "gemm256s_persistent+tail128x128", "gemm256s_persistent+splitk16",
    # plan_skinny
    *(f"skinny<KS={ks}>" for ks in SKINNY_KS.values()), *(f"skinny<KS={ks}>+norm" for ks in SKINNY_KS.values()),
    # plan_rows
    "rows_stream<8,8>", "rows_stream<6,8>", "rows_stream<8,4>+tree", "rows_mid<SK=8>", "rows_mid<SK=2>+tree",
    # plan_gemm_tn
    "tn", "tn_persistent", "tn_all_split+splitk4", "tn+splitk16",
}
REACHED = set()


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def reached(ops, want, what):
    got = ops.gemm_last_form()
    assert got == want, f"{what}: ran on {got}, the case means {want}"
    REACHED.add(got)


# ---- buffers ---------------------------------------------------------------------------------------------------------------
class Buf:
    """The [rows, cols] corner of a NaN-filled [rows + 3, cols + pad] buffer."""

    def __init__(self, rows, cols, dev, dtype=bf16, pad=12, data=None):
        self.buf = torch.full((rows + 3, cols + pad), NAN, dtype=dtype, device=dev)
        self.v = self.buf[:rows, :cols]
        if data is not None:
            self.v.copy_(data.to(dtype))

    def take(self, what, rows_idx=None, cols=None):
        """The logical output (all rows, or rows_idx) as fp64; everything else must still be NaN, everything inside finite."""
        cols = self.v.shape[1] if cols is None else cols
        written = torch.zeros(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        if rows_idx is None:
            written[:self.v.shape[0], :cols] = True
            out = self.buf[:self.v.shape[0], :cols]
        else:
            written[rows_idx, :cols] = True
            out = self.buf[rows_idx, :cols]
        assert bool(self.buf[~written].isnan().all()), f"{what}: wrote outside its logical output"
        assert bool(torch.isfinite(out).all()), f"{what}: non-finite or unwritten output"
        return out.double()


_ws = {}


def workspace(dev, fill=True):
    if "ws" not in _ws:
        _ws["ws"] = torch.empty(32 << 20, dtype=f32, device=dev)          # 128 MiB
    if fill:
        _ws["ws"].fill_(NAN)
    return _ws["ws"]


def n_out_of(epi, N):
    return N // 2 if epi == EPI_SWIGLU else 2 * N if epi == EPI_SWIGLU_BWD else N


def run_gemm(ops, dev, A, Wp, epi, M, N, *, bias=None, scale=None, res=None, res_row_mod=0, out_map=None, ws=None, inplace=False, **kw):
    """One launch into fresh NaN buffers. Returns (logical C, logical C2 or None, kept logical rows) as fp64 on the device."""
    odt = f32 if epi in (EPI_F32, EPI_F32_BF16R) else bf16
    n_out = n_out_of(epi, N)
    kept, orows = G.out_rows(M, out_map, dev)
    nrows = M if out_map is None else ((M + out_map[0] - 1) // out_map[0]) * out_map[1]
    if inplace:
        C = Buf(nrows, n_out, dev, odt, data=res)
        res = C.v
    else:
        C = Buf(nrows, n_out, dev, odt, pad=8 if epi == EPI_SWIGLU_BWD else 12)
    C2 = None
    if epi in (EPI_SWIGLU_KEEP, EPI_BIAS_GELU_KEEP):
        C2 = Buf(nrows, N // 2 if epi == EPI_SWIGLU_KEEP else N, dev)
    ops.gemm(A, Wp, C.v, epi, bias=bias, scale=scale, res=res, res_row_mod=res_row_mod, out_map=out_map, workspace=ws,
             out2=None if C2 is None else C2.v, **kw)
    what = G.EPI_NAMES[epi]
    sel = None if out_map is None else orows
    return C.take(what, sel), None if C2 is None else C2.take(what + " C2", sel), kept


# ---- the reference is the same on the CPU and on the device ------------------------------------------------------------------
def test_reference_same_on_cpu_and_device(dev):
    M, N, K = 33, 80, 512
    A, W = G.dyadic_a((M, K), 1), G.dyadic_w((N, K), 2)
    bias, ls, res = G.dyadic_add((N,), 3), G.layerscale(N, 4), G.dyadic_add((M, N), 5)
    x = G.product(A, W)
    xd = G.product(A.to(dev), W.to(dev))
    assert torch.equal(xd.cpu(), x)
    with T64.on_device():
        for epi, sc in ((EPI_NONE, None), (EPI_BIAS, None), (EPI_RES, None), (EPI_BIAS_RES, None), (EPI_BIAS_RES, ls)):
            ref_d = G.linear_ref(epi, xd, bias.to(dev), None if sc is None else sc.to(dev), res.to(dev))
            assert torch.equal(ref_d.cpu(), G.linear_ref(epi, x, bias, sc, res)), G.EPI_NAMES[epi]
        t, td = T64.rb64(x), T64.rb64(xd)
        assert torch.equal(td.cpu(), t)
        # transcendental functions differ in their last fp64 bits between the two libraries (and 1 + erf cancels in GELU's
        # negative tail): the two evaluations must agree to a millionth of the bound they are used with
        sd, sc = T64.swiglu_forward(td), T64.swiglu_forward(t)
        bound = T64._bound(sc["act"], sc["mag"], 2, sc["tie"], sc["extra"], T64.U)
        assert bool(((sd["act"].cpu() - sc["act"]).abs() <= 1e-6 * bound).all()) and torch.equal(sd["tie"].cpu(), sc["tie"])
        gd, gc = T64.gelu_forward(td), T64.gelu_forward(t)
        bound = T64._bound(gc["y"], gc["mag"], 4, None, gc["extra"], T64.U)
        assert bool(((gd["y"].cpu() - gc["y"]).abs() <= 1e-6 * bound).all())
        assert torch.allclose(gd["mag"].cpu(), gc["mag"], rtol=1e-9, atol=0) and torch.equal(gd["extra"].cpu(), gc["extra"])
    Ag, Wg = G.gauss((M, K), 6), G.gauss((N, K), 7)
    assert torch.allclose(G.product(Ag.to(dev), Wg.to(dev)).cpu(), G.product(Ag, Wg), rtol=1e-13, atol=1e-13)


# ---- tile forms ------------------------------------------------------------------------------------------------------------------
TILE_ALL = TILE_CASES + [("mid<5,4>", 270, 10192, 576, False)]
TILE_IDS = [f"{f}-{M}x{N}x{K}" for f, M, N, K, _ in TILE_ALL]


def _tile_operands(dev, M, N, K, gauss, seed):
    """A in its padded buffer, the packed weight (N rounded up to a multiple of 32 for the SwiGLU epilogues; the other
    epilogues take the leading N / 16 tiles of the same packing) and the row-major weight on the device."""
    from bridgelang_amd import ops
    Nw = N if N % 32 == 0 else N + 16
    if gauss:
        a, w = G.gauss((M, K), seed), G.gauss((Nw, K), seed + 1, K ** -0.5)
    else:
        a, w = G.dyadic_a((M, K), seed), G.dyadic_w((Nw, K), seed + 1)
    A = Buf(M, K, dev, pad=8, data=a)
    Wd = w.to(dev).to(bf16)
    return A, ops.pack_weight(Wd), Wd, Nw


@pytest.mark.parametrize("form,M,N,K,use_ws", TILE_ALL, ids=TILE_IDS)
def test_tile_form_dyadic(dev, form, M, N, K, use_ws):
    from bridgelang_amd import ops
    G.assert_dyadic_exact(K)
    A, Wp, Wd, Nw = _tile_operands(dev, M, N, K, False, 100)
    x_full = G.product(A.v, Wd)                                        # exact product [M, Nw], fp64 on the device
    ws = workspace(dev) if use_ws else None
    bias_w = G.dyadic_add((Nw,), 102).to(dev).to(bf16)
    ls = G.layerscale(N, 103).to(dev).to(bf16)
    res = Buf(M, N, dev, data=G.dyadic_add((M, N), 104))
    table = Buf(RES_MOD, N, dev, data=G.dyadic_add((RES_MOD, N), 105))
    gu = Buf(M, 2 * N, dev, pad=8, data=G.dyadic_add((M, 2 * N), 106))
    pre = Buf(M, N, dev, data=G.dyadic_add((M, N), 107))

    def case(epi, n=N, **kw):
        """Run one epilogue at n columns and check it; returns the logical output."""
        what = f"{form} {G.EPI_NAMES[epi]}" + "".join(f" {k}" for k in kw if k in ("scale", "out_map", "inplace"))
        wp = Wp[:n // 16]
        chk = dict(bias=bias_w[:n] if epi in G.HAS_BIAS else None, scale=kw.get("scale"))
        C, C2, kept = run_gemm(ops, dev, A.v, wp, epi, M, n, ws=ws, bias=chk["bias"], **kw)
        reached(ops, form, what)
        r = kw.get("res")
        if r is not None and epi in G.HAS_RES:                         # gather the residual rows the kept output rows read
            r = r.double()[kept % kw["res_row_mod"] if kw.get("res_row_mod") else kept]
        G.check_epilogue(what, epi, x_full[kept][:, :n], C, C2, bias=chk["bias"], scale=chk["scale"], res=r)
        return C

    for epi in (EPI_F32, EPI_F32_BF16R, EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_KEEP):
        case(epi)
    plain = case(EPI_RES, res=res.v)
    assert torch.equal(case(EPI_RES, res=res.v.clone(), inplace=True), plain), f"{form}: in-place residual differs"
    case(EPI_BIAS_RES, res=res.v)
    case(EPI_BIAS_RES, res=res.v, scale=ls)
    case(EPI_BIAS_RES, res=table.v, scale=ls, res_row_mod=RES_MOD, out_map=OUT_MAP)
    case(EPI_RES, res=table.v, res_row_mod=RES_MOD, out_map=OUT_MAP)
    case(EPI_GELU_BWD, res=pre.v)
    case(EPI_SWIGLU_BWD, res=gu.v)
    if form not in SWIGLU_UNREACHABLE:
        case(EPI_SWIGLU, n=Nw)
        case(EPI_SWIGLU_KEEP, n=Nw)


@pytest.mark.parametrize("form,M,N,K,use_ws", [c for c in TILE_ALL if c[3] <= G.GAUSS_KMAX],
                         ids=[i for i, c in zip(TILE_IDS, TILE_ALL) if c[3] <= G.GAUSS_KMAX])
def test_tile_form_gauss(dev, form, M, N, K, use_ws):
    from bridgelang_amd import ops
    A, Wp, Wd, _ = _tile_operands(dev, M, N, K, True, 200)
    wp, Wn = Wp[:N // 16], Wd[:N]
    ws = workspace(dev) if use_ws else None
    bias = G.gauss((N,), 202).to(dev).to(bf16)
    res = Buf(M, N, dev, data=G.gauss((M, N), 203))
    C, _, _ = run_gemm(ops, dev, A.v, wp, EPI_F32, M, N, ws=ws)
    reached(ops, form, "gauss f32")
    G.check_gauss(f"{form} gauss f32", EPI_F32, A.v, Wn, C)
    C, _, _ = run_gemm(ops, dev, A.v, wp, EPI_BIAS_RES, M, N, ws=ws, bias=bias, res=res.v)
    reached(ops, form, "gauss bias_res")
    G.check_gauss(f"{form} gauss bias_res", EPI_BIAS_RES, A.v, Wn, C, bias=bias, res=res.v)


# ---- the weight-streaming kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SKINNY_K)
def test_skinny_dyadic(dev, K):
    from bridgelang_amd import ops
    G.assert_dyadic_exact(K)
    form = f"skinny<KS={SKINNY_KS[K]}>"
    Nw = 4128                                                          # 258 tiles: the SwiGLU width (N % 32 == 0) next to 4112
    A = Buf(16, K, dev, pad=8, data=G.dyadic_a((16, K), 300))
    Wd = G.dyadic_w((Nw, K), 301).to(dev).to(bf16)
    Wp = ops.pack_weight(Wd)
    x_full = G.product(A.v, Wd)
    resd = G.dyadic_add((16, Nw), 302)
    for M in SKINNY_M:
        for N in SKINNY_N:
            res = Buf(M, N, dev, data=resd[:M, :N])
            for epi in G.SKINNY_EPIS:
                n = N if epi != EPI_SWIGLU else (Nw if N == 4112 else 32)
                what = f"{form} {G.EPI_NAMES[epi]} M={M} N={n}"
                C, _, _ = run_gemm(ops, dev, A.v[:M], Wp[:n // 16], epi, M, n, res=res.v if epi == EPI_RES else None, skinny=True)
                reached(ops, form, what)
                G.check_epilogue(f"{form} {G.EPI_NAMES[epi]}", epi, x_full[:M, :n], C, res=res.v if epi == EPI_RES else None)


@pytest.mark.parametrize("K", SKINNY_K)
def test_skinny_fused_norm(dev, K):
    """The fused a_norm's activations, read out exactly through a 0/1 weight (a product with 0 or 1 and a sum of zeros are
    exact, bf16 of a bf16 value is itself), against the fp64 HF RMSNorm; then a Gaussian weight at K <= 1536."""
    from bridgelang_amd import ops
    form = f"skinny<KS={SKINNY_KS[K]}>+norm"
    Np = min(K, 4112)
    cols = torch.randperm(K, generator=torch.Generator().manual_seed(400))[:Np].to(dev)
    sel = torch.zeros(Np, K, dtype=bf16, device=dev)
    sel[torch.arange(Np, device=dev), cols] = 1.0
    Wp = ops.pack_weight(sel)
    nw = (G.gauss((K,), 401, 0.25) + 1).to(bf16).to(dev)
    xs = G.gauss((16, K), 402, 3.0)
    xs[3] *= 2.0 ** -20                                                # a row of tiny values: rstd near 1/sqrt(eps)
    for M in SKINNY_M:
        A = Buf(M, K, dev, pad=8, data=xs[:M])
        C, _, _ = run_gemm(ops, dev, A.v, Wp, EPI_NONE, M, Np, skinny=True, a_norm=(nw, EPS))
        reached(ops, form, f"M={M}")
        G.check_rmsnorm(f"{form} activations", C, A.v, nw, EPS, cols=cols)
    if K <= G.GAUSS_KMAX:
        Wd = G.gauss((528, K), 403, K ** -0.5).to(dev).to(bf16)
        A = Buf(16, K, dev, pad=8, data=xs)
        C, _, _ = run_gemm(ops, dev, A.v, ops.pack_weight(Wd), EPI_F32, 16, 528, skinny=True, a_norm=(nw, EPS))
        reached(ops, form, "gauss")
        G.check_gauss_norm(f"{form} gauss f32", C, A.v, nw, EPS, Wd)


# ---- the rows forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N,K,use_ws,row_counts", ROWS_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in ROWS_CASES])
def test_rows_dyadic(dev, form, N, K, use_ws, row_counts):
    from bridgelang_amd import ops
    G.assert_dyadic_exact(K)
    Nw = N if N % 32 == 0 else N + 32 - N % 32
    Mx = max(row_counts)
    A = Buf(Mx, K, dev, pad=8, data=G.dyadic_a((Mx, K), 500))
    Wd = G.dyadic_w((Nw, K), 501).to(dev).to(bf16)
    Wp = ops.pack_weight(Wd)
    x_full = G.product(A.v, Wd)
    resd = G.dyadic_add((Mx, N), 502)
    for M in row_counts:
        res = Buf(M, N, dev, data=resd[:M])
        for epi in G.SKINNY_EPIS:
            n = Nw if epi == EPI_SWIGLU else N
            ws = workspace(dev) if use_ws else None
            C, _, _ = run_gemm(ops, dev, A.v[:M], Wp[:n // 16], epi, M, n, res=res.v if epi == EPI_RES else None, ws=ws, skinny_rows=True)
            reached(ops, form, f"{G.EPI_NAMES[epi]} M={M}")
            G.check_epilogue(f"{form} {G.EPI_NAMES[epi]}", epi, x_full[:M, :n], C, res=res.v if epi == EPI_RES else None)


# ---- the weight-gradient GEMM ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,T,M,N,use_ws", TN_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in TN_CASES])
def test_tn_dyadic(dev, form, T, M, N, use_ws):
    from bridgelang_amd import ops, train_ops
    G.assert_dyadic_exact(T, addmax=0.0)
    dy = Buf(T, M, dev, pad=8, data=G.dyadic_a((T, M), 600))           # rows past T and the pad columns hold NaN
    xx = Buf(T, N, dev, pad=16, data=G.dyadic_w((T, N), 601))
    C = Buf(M, N, dev, f32)
    train_ops.gemm_tn(dy.v, xx.v, C.v, workspace=workspace(dev) if use_ws else None)
    reached(ops, form, "tn")
    with T64.on_device():
        G.assert_exact(C.take(form), G.product_tn(dy.v, xx.v), f"{form} f32")


# ---- norm forward --------------------------------------------------------------------------------------------------------------------
def _norm_rows(rows, dim, seed):
    x = G.gauss((rows, dim), seed, 2.0)
    if rows >= 4:
        x[rows - 2] = (x[rows - 2] * 0.25 + 16.0).to(bf16).float()     # mean >> spread: offset / spread = 2^5
        x[rows - 1] = -1.5                                             # a constant row
    return x


@pytest.mark.parametrize("dim", NORM_DIMS)
def test_norm_forward(dev, dim):
    from bridgelang_amd import ops
    w = (G.gauss((dim,), 701, 0.25) + 1).to(bf16).to(dev)
    b = G.gauss((dim,), 702, 0.1).to(bf16).to(dev)
    for rows in NORM_ROWS:
        X = Buf(rows, dim, dev, pad=8, data=_norm_rows(rows, dim, 700))
        Y = Buf(rows, dim, dev, pad=24)                                # ldx != ldy != dim
        ops.rmsnorm(X.v, w, Y.v, EPS)
        G.check_rmsnorm(f"rmsnorm NCH={(dim // 8 + 63) // 64}", Y.take("rmsnorm"), X.v, w, EPS)
        Y = Buf(rows, dim, dev, pad=24)
        ops.layernorm(X.v, w, b, Y.v, EPS)
        G.check_layernorm(f"layernorm NCH={(dim // 8 + 63) // 64}", Y.take("layernorm"), X.v, w, b, EPS)


@pytest.mark.parametrize("K", SKINNY_K)
def test_rmsnorm_skinny(dev, K):
    from bridgelang_amd import ops
    w = (G.gauss((K,), 801, 0.25) + 1).to(bf16).to(dev)
    for rows in NORM_ROWS:
        x = _norm_rows(rows, K, 800)
        X = Buf(rows, K, dev, pad=8, data=x)
        Y = Buf(rows, K, dev, pad=24)
        ops.rmsnorm_skinny(X.v, w, Y.v, EPS)
        out = Y.take("rmsnorm_skinny")
        G.check_rmsnorm(f"rmsnorm_skinny KS={SKINNY_KS[K]}", out, X.v, w, EPS)
        Z = Buf(rows, K, dev, pad=8, data=x)                           # in place: y aliases x
        ops.rmsnorm_skinny(Z.v, w, Z.v, EPS)
        assert torch.equal(Z.take("rmsnorm_skinny in place"), out), "in place differs"


# ---- closing: the forms this module reached are the full list ----------------------------------------------------------------------
def test_every_form_was_reached():
    per_form = {}
    for what, ratio in T64.RATIOS.items():
        key = what if what.startswith(("rmsnorm", "layernorm")) else what.split(" ")[0]
        per_form[key] = max(per_form.get(key, 0.0), ratio)
    for key in sorted(per_form):
        print(f"largest err/bound {per_form[key]:.4f}  {key}")
    print(f"bit-exact elements compared: {sum(G.EXACT.values())} in {len(G.EXACT)} checks")
    assert REACHED == ALL_FORMS, f"not reached: {sorted(ALL_FORMS - REACHED)}; not listed: {sorted(REACHED - ALL_FORMS)}"
