"""Every dispatch branch of the training-step kernels (csrc/train.hip) at its smallest shape, against the fp64 reference
and the derived per-element bounds of tests/train_ref64.py.

Scaffolding: inputs come from rand_bf16; every 2-D input and output is a column window [:, 8 : 8 + cols] of a wider
buffer (leading dimension cols + 16, a multiple of 8) whose other elements hold a NaN sentinel; after the launch every
element outside an output window must still be the sentinel bit for bit and every element inside must be finite.
Dense outputs and workspaces are exactly as large as the case states and are followed by sentinel elements.

Branch → case
  norm_bwd_kernel<NCH, LN, DRL>  NCH 1: dim 8 (63 idle lanes); 2 (launch bounds 3): 520 ragged, 1024; 3: 1152, 1536;
      4 (RPW 2): 2048; 5: 2056 (ragged, the plain path even with dres), 2560; 6..10: 3072, 3584, 4096, 4608, 5120 — each
      for RMSNorm and LayerNorm, with and without dres, at 1 / 3 / 5 / 16 / 17 / 70 rows (partial RPW groups, one and
      several blocks, a ragged last block)                                        test_norm_backward
      DRL 5..10 (RMSNorm + dres, dim = NCH·512) and the same shapes under BL_NORM_BWD_DRL=0, both against fp64 and
      against each other                                                          test_norm_backward (dims >= 2560)
      more than 512 blocks → re-blocking to 20 rows                               test_rmsnorm_backward_8200_rows_reblocked
      workspace for two blocks → rpb doubling; the two rejections                 test_norm_backward_workspace_rules
  reduce_partials_kernel  nblocks 1, 4, 5, 28, 29, 32, 33, 61 (the `b + 28 < nblocks` loop and its tail)
                                                                                  test_reduce_partials_block_counts
  layerscale_bwd_kernel / scale_residual_kernel  cols 8, 1024 (128 threads), 2048, 2056 (second grid.y block), rows 1..5
      (the four-in-flight clamp) and 17                                           test_layerscale
  colsum_partial_kernel  rows 1, 15, 16, 17, 63, 64, 65, 300 x cols 8, 512, 520, 1032; rpb doubling     test_colsum
  element-wise kernels (grid_for caps the grid at 2048 x 256 threads): smallest shape, a shape just beyond 2048·256 work
      items with a ragged end (second trip of the grid-stride loop), a row of value edges
      test_swiglu, test_gelu, test_scale_residual_second_trip, test_rope_backward, test_scale, test_dropout
  ce_backward_kernel  n 8, 2048, 2056, 32064; confident / hopeless targets; ignored rows; one valid row
                                                                                  test_cross_entropy_backward
  gemm_tn_small_kernel<R, TRANS>  R 64 / 128 / 192 x both layouts x T 1, 31, 32, 33, 192 (6 steps), 193 (7: the ring
      wraps), 389 x N 64, 192 x alpha 1, 0.25 x ws none / present; 2 and 4 splits and the workspace one float short
                                                                                  test_gemm_tn_small, test_gemm_tn_small_splits
  embed_bwd_kernel                                                                test_embed_backward
  sumsq_partial_kernel (vector and scalar path), clip_coef_kernel, adamw_kernel   test_sumsq_and_clip, test_adamw
  map_rows / lora_block_mask / casts / axpy / zero_bytes / copy_bytes / batched_ops (first, interior, last entry of the
      binary search), bit for bit                                                 test_map_rows … test_batched_ops
"""
import pytest
import torch

import train_ref64 as T64
from conftest import rand_bf16
from test_train_ref_cpu import ADAM_HP, EDGES, adam_case, ce_case, edge_row

pytestmark = pytest.mark.gpu
EPS = 1e-6
PAD = 8
NAN = float("nan")
bf16, f32 = torch.bfloat16, torch.float32


# ---- windows and sentinels ----------------------------------------------------------------------------------------------
class Win:
    """A [rows, cols] window at column PAD of a NaN-filled [rows, cols + 2·PAD] buffer."""

    def __init__(self, rows, cols, dev, dtype=bf16, data=None):
        self.buf = torch.full((rows, cols + 2 * PAD), NAN, dtype=dtype, device=dev)
        self.v = self.buf[:, PAD:PAD + cols]
        if data is not None:
            self.v.copy_(data.to(dtype))
        self.before = self.buf.clone()

    def check(self, what):
        """Everything outside the window is untouched (bit for bit); everything inside is finite. Returns the window on the CPU."""
        itype = torch.int16 if self.buf.element_size() == 2 else torch.int32
        now, was = self.buf.view(itype).clone(), self.before.view(itype)
        cols = self.v.shape[1]
        now[:, PAD:PAD + cols] = was[:, PAD:PAD + cols]
        assert torch.equal(now, was), f"{what}: wrote outside its [rows, cols] window"
        out = self.v.float().cpu()
        assert torch.isfinite(out).all(), f"{what}: non-finite output"
        return out


def win(x, dev, dtype=bf16):
    return Win(x.shape[0], x.shape[1], dev, dtype, x)


class Flat:
    """n elements followed (and preceded) by sentinel elements: dense outputs and exactly sized workspaces."""

    def __init__(self, n, dev, dtype=f32, data=None, guard=16):
        self.n, self.g = n, guard
        self.buf = torch.full((n + 2 * guard,), NAN, dtype=dtype, device=dev)
        self.v = self.buf[guard:guard + n]
        if data is not None:
            self.v.copy_(data.reshape(-1).to(dtype))

    def check(self, what, finite=True):
        itype = {2: torch.int16, 4: torch.int32}[self.buf.element_size()]
        b = self.buf.view(itype)
        ref = torch.full((1,), NAN, dtype=self.buf.dtype).view(itype).item()
        assert bool((b[:self.g] == ref).all()) and bool((b[self.g + self.n:] == ref).all()), f"{what}: wrote past its {self.n} elements"
        out = self.v.cpu()
        if finite:
            assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
        return out


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- norm backward ---------------------------------------------------------------------------------------------------------
NORM_DIMS = [8, 520, 1024, 1152, 1536, 2048, 2056, 2560, 3072, 3584, 4096, 4608, 5120]
NORM_ROWS = [1, 3, 5, 16, 17, 70]
_norm_cache = {}


def _norm_inputs(rows, dim):
    """Seeded inputs, generated once per width (70 rows; the 8200-row case has its own) and sliced."""
    n = 70 if rows <= 70 else rows
    if (n, dim) not in _norm_cache:
        w = (rand_bf16((dim,), 2, 0.02) + 1).to(bf16).float()
        _norm_cache[(n, dim)] = (rand_bf16((n, dim), 1, 2.0), w, rand_bf16((n, dim), 3), rand_bf16((n, dim), 4))
    x, w, dy, dres = _norm_cache[(n, dim)]
    if n > 70:
        del _norm_cache[(n, dim)]
    return x[:rows], w, dy[:rows], dres[:rows]


def _run_norm(dev, ln, x, w, dy, dres, ws_floats, what):
    """One launch on windows; returns (dx, dw, db) on the CPU after the canary checks."""
    from bridgelang_amd import train_ops as T
    rows, dim = x.shape
    X, DY, DX = win(x, dev), win(dy, dev), Win(rows, dim, dev)
    DR = win(dres, dev) if dres is not None else None
    W = w.to(bf16).to(dev)
    dw, db, ws = Flat(dim, dev), Flat(dim, dev), Flat(ws_floats, dev)
    if ln:
        T.layernorm_backward(X.v, W, DY.v, DX.v, dw.v, db.v, ws.v, EPS, dres=DR.v if DR else None)
    else:
        T.rmsnorm_backward(X.v, W, DY.v, DX.v, dw.v, ws.v, EPS, dres=DR.v if DR else None)
    torch.cuda.synchronize()
    ws.check(f"{what} workspace", finite=False)
    return DX.check(f"{what} dx"), dw.check(f"{what} dw").double(), (db.check(f"{what} db").double() if ln else None)


@pytest.mark.parametrize("dim", NORM_DIMS)
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
def test_norm_backward(dev, ln, dim, monkeypatch):
    nm = "ln" if ln else "rms"
    drl_shape = (not ln) and dim >= 2560 and dim % 512 == 0
    for rows in NORM_ROWS:
        x, w, dy, dres = _norm_inputs(rows, dim)
        ws_floats = ((rows + 15) // 16) * dim * (2 if ln else 1)
        rpb, nblk = T64.norm_bwd_blocking(rows, dim, ws_floats, ln)
        assert rpb == 16
        for use_dres in (False, True):
            ref = T64.norm_backward(x, w, dy, EPS, dres if use_dres else None, ln)
            got = {}
            for drl in (("1", "0") if (drl_shape and use_dres) else ("1",)):
                monkeypatch.setenv("BL_NORM_BWD_DRL", drl)
                what = f"gpu {nm} bwd dim {dim} rows {rows}{' +dres' if use_dres else ''}{' DRL off' if drl == '0' else ''}"
                dx, dw, db = _run_norm(dev, ln, x, w, dy, dres if use_dres else None, ws_floats, what)
                T64.check_norm_backward(f"gpu {nm} bwd{' DRL off' if drl == '0' else ''}", ref, ln, rpb, nblk, dx, dw, db)
                got[drl] = (dx, dw)
            if len(got) == 2:        # same arithmetic with the dres row through LDS: bit-identical
                assert torch.equal(got["0"][0], got["1"][0]) and torch.equal(got["0"][1], got["1"][1])
    monkeypatch.delenv("BL_NORM_BWD_DRL", raising=False)


def test_rmsnorm_backward_8200_rows_reblocked(dev):
    """8200 x 2560 with dres and a workspace for ceil(rows/16) blocks: 513 > 512 blocks, so the launcher re-blocks to 20
    rows (410 blocks, DRL<5>). The only shape on this branch; the reference is computed in row slices."""
    rows, dim = 8200, 2560
    x, w, dy, dres = _norm_inputs(rows, dim)
    ws_floats = ((rows + 15) // 16) * dim
    rpb, nblk = T64.norm_bwd_blocking(rows, dim, ws_floats, False)
    assert (rpb, nblk) == (20, 410)
    dx, dw, _ = _run_norm(dev, False, x, w, dy, dres, ws_floats, "gpu rms bwd 8200 x 2560")
    ref = T64.norm_backward(x, w, dy, EPS, dres, False)
    T64.check_norm_backward("gpu rms bwd 8200 rows", ref, False, rpb, nblk, dx, dw)


def test_norm_backward_workspace_rules(dev):
    from bridgelang_amd import train_ops as T
    from bridgelang_amd._lib import BridgeLangHipError
    rows, dim = 70, 520
    x, w, dy, dres = _norm_inputs(rows, dim)
    for ln in (False, True):
        ws_floats = 2 * dim * (2 if ln else 1)                      # two blocks' partials: rpb doubles 16 → 64
        rpb, nblk = T64.norm_bwd_blocking(rows, dim, ws_floats, ln)
        assert (rpb, nblk) == (64, 2)
        dx, dw, db = _run_norm(dev, ln, x, w, dy, dres, ws_floats, "gpu norm bwd two-block workspace")
        T64.check_norm_backward(f"gpu {'ln' if ln else 'rms'} bwd rpb 64", T64.norm_backward(x, w, dy, EPS, dres, ln), ln, rpb, nblk, dx, dw, db)
    # rejections, as the wrapper's error: a workspace too small even for rpb = 4096, and dim = 5128
    big = torch.zeros(8200, 16, dtype=bf16, device=dev)
    w16 = torch.ones(16, dtype=bf16, device=dev)
    assert T64.norm_bwd_blocking(8200, 16, 2 * 16, False) is None
    with pytest.raises(BridgeLangHipError):
        T.rmsnorm_backward(big, w16, big, torch.empty_like(big), torch.empty(16, device=dev), torch.empty(2 * 16, device=dev), EPS)
    wide = torch.zeros(2, 5128, dtype=bf16, device=dev)
    with pytest.raises(BridgeLangHipError):
        T.rmsnorm_backward(wide, torch.ones(5128, dtype=bf16, device=dev), wide, torch.empty_like(wide), torch.empty(5128, device=dev),
                           torch.empty(5128, device=dev), EPS)
    with pytest.raises(BridgeLangHipError):
        T.layernorm_backward(wide, torch.ones(5128, dtype=bf16, device=dev), wide, torch.empty_like(wide), torch.empty(5128, device=dev),
                             torch.empty(5128, device=dev), torch.empty(2 * 5128, device=dev), EPS)
    torch.cuda.synchronize()


# ---- LayerScale, reduce_partials, colsum -------------------------------------------------------------------------------------
def _run_layerscale(dev, dy, u, ls, ws_floats, what):
    from bridgelang_amd import train_ops as T
    rows, cols = dy.shape
    DY, Uw, DU = win(dy, dev), win(u, dev), Win(rows, cols, dev)
    dsc, ws = Flat(cols, dev), Flat(ws_floats, dev)
    T.layerscale_backward(DY.v, Uw.v, ls.to(bf16).to(dev), DU.v, dsc.v, ws.v)
    torch.cuda.synchronize()
    ws.check(f"{what} workspace", finite=False)
    return DU.check(f"{what} du"), dsc.check(f"{what} dscale").double()


def _ls_inputs(rows, cols):
    return (rand_bf16((rows, cols), 3), rand_bf16((rows, cols), 6), (rand_bf16((cols,), 7, 0.02) + 0.1).to(bf16).float(),
            rand_bf16((rows, cols), 8))


@pytest.mark.parametrize("nblocks", [1, 4, 5, 28, 29, 32, 33, 61])
def test_reduce_partials_block_counts(dev, nblocks):
    rows, cols = 16 * nblocks - 3, 64
    dy, u, ls, _ = _ls_inputs(rows, cols)
    rpb, nblk = T64.rows_blocking(rows, cols, nblocks * cols, 16)
    assert (rpb, nblk) == (16, nblocks)
    du, dsc = _run_layerscale(dev, dy, u, ls, nblocks * cols, f"gpu layerscale {nblocks} blocks")
    ref = T64.layerscale_backward(dy, u, ls)
    T64.assert_bf16_close(du, ref["du"], ref["m_du"], 1, "gpu layerscale du")
    T64.assert_f32_close(dsc, ref["dscale"], ref["m_dscale"], T64.reduce_depth(rpb, nblk), "gpu reduce_partials dscale")


@pytest.mark.parametrize("cols", [8, 1024, 2048, 2056])
def test_layerscale(dev, cols):
    """Backward and the scale_residual forward. The forward check is exact: fp64 with the two documented roundings equals
    the kernel bit for bit (u·ls is exact in fp32 and the sum of two bf16 values never sits on a bf16 tie after one fp32
    rounding), which is asserted on top of the bound."""
    from bridgelang_amd import train_ops as T
    for rows in (1, 2, 3, 4, 5, 17):
        dy, u, ls, res = _ls_inputs(rows, cols)
        ws_floats = ((rows + 15) // 16) * cols
        du, dsc = _run_layerscale(dev, dy, u, ls, ws_floats, f"gpu layerscale {rows} x {cols}")
        ref = T64.layerscale_backward(dy, u, ls)
        T64.assert_bf16_close(du, ref["du"], ref["m_du"], 1, "gpu layerscale du")
        T64.assert_f32_close(dsc, ref["dscale"], ref["m_dscale"], T64.reduce_depth(16, (rows + 15) // 16), "gpu layerscale dscale")
        Uw, Rw, Y = win(u, dev), win(res, dev), Win(rows, cols, dev)
        T.scale_residual(Uw.v, ls.to(bf16).to(dev), Rw.v, Y.v)
        y = Y.check(f"gpu scale_residual {rows} x {cols}")
        yr, ym = T64.scale_residual(u, ls, res)
        T64.assert_bf16_close(y, yr, ym, 2, "gpu scale_residual y")
        assert torch.equal(y.double(), T64.rb64(yr))


@pytest.mark.parametrize("cols", [8, 512, 520, 1032])
def test_colsum(dev, cols):
    from bridgelang_amd import train_ops as T
    full = rand_bf16((300, cols), cols)
    cases = [(r, ((r + 63) // 64) * cols) for r in (1, 15, 16, 17, 63, 64, 65, 300)] + [(300, 2 * cols)]   # last: rpb doubles to 256
    for rows, ws_floats in cases:
        a = full[:rows]
        rpb, nblk = T64.rows_blocking(rows, cols, ws_floats, 64)
        A, out, ws = win(a, dev), Flat(cols, dev), Flat(ws_floats, dev)
        T.colsum(A.v, out.v, ws.v)
        torch.cuda.synchronize()
        ws.check("gpu colsum workspace", finite=False)
        ref, mag = T64.colsum(a)
        T64.assert_f32_close(out.check("gpu colsum").double(), ref, mag, T64.reduce_depth(rpb // 4, nblk), "gpu colsum")
    assert (rpb, nblk) == (256, 2)


# ---- element-wise kernels -------------------------------------------------------------------------------------------------------
def _gate_edges(gu, seed):
    n = len(EDGES)
    gu[0, 0:2 * n:2] = torch.tensor(EDGES, dtype=f32).to(bf16).float()
    gu[0, 1:2 * n:2] = rand_bf16((n,), seed)
    return gu


@pytest.mark.parametrize("rows,inter", [(1, 4), (3, 64), (257, 8196)], ids=["smallest", "edges", "second-trip"])
def test_swiglu(dev, rows, inter):
    from bridgelang_amd import train_ops as T
    gu, dact = rand_bf16((rows, 2 * inter), 1, 1.5), rand_bf16((rows, inter), 2)
    if inter == 64:
        gu = _gate_edges(gu, 9)
    GU, A = win(gu, dev), Win(rows, inter, dev)
    T.swiglu(GU.v, A.v)
    fr = T64.swiglu_forward(gu)
    T64.assert_bf16_close(A.check("gpu swiglu fwd"), fr["act"], fr["mag"], 2, "gpu swiglu fwd", tie=fr["tie"], extra=fr["extra"])
    DA, DG = win(dact, dev), Win(rows, 2 * inter, dev)
    T.swiglu_backward(GU.v, DA.v, DG.v)
    T64.check_swiglu_backward("gpu swiglu bwd", T64.swiglu_backward(gu, dact), DG.check("gpu swiglu bwd"))


@pytest.mark.parametrize("rows,cols", [(1, 8), (3, 64), (513, 8200)], ids=["smallest", "edges", "second-trip"])
def test_gelu(dev, rows, cols):
    from bridgelang_amd import train_ops as T
    x, dy = rand_bf16((rows, cols), 3, 2.0), rand_bf16((rows, cols), 4)
    if cols == 64:
        x[0] = edge_row(cols, 53)
        x[1] = torch.linspace(-9.0, -2.0, cols).to(bf16).float()      # the far negative tail, where erf_as's absolute error decides
    X, Y = win(x, dev), Win(rows, cols, dev)
    T.gelu(X.v, Y.v)
    fr = T64.gelu_forward(x)
    T64.assert_bf16_close(Y.check("gpu gelu fwd"), fr["y"], fr["mag"], 4, "gpu gelu fwd", extra=fr["extra"])
    DY, DX = win(dy, dev), Win(rows, cols, dev)
    T.gelu_backward(X.v, DY.v, DX.v)
    br = T64.gelu_backward(x, dy)
    T64.assert_bf16_close(DX.check("gpu gelu bwd"), br["dx"], br["mag"], 4, "gpu gelu bwd", extra=br["extra"])


def test_scale_residual_second_trip(dev):
    from bridgelang_amd import train_ops as T
    rows, cols = 513, 8200
    _, u, ls, res = _ls_inputs(rows, cols)
    Uw, Rw, Y = win(u, dev), win(res, dev), Win(rows, cols, dev)
    T.scale_residual(Uw.v, ls.to(bf16).to(dev), Rw.v, Y.v)
    yr, ym = T64.scale_residual(u, ls, res)
    y = Y.check("gpu scale_residual second trip")
    T64.assert_bf16_close(y, yr, ym, 2, "gpu scale_residual y")
    assert torch.equal(y.double(), T64.rb64(yr))


@pytest.mark.parametrize("B,S,H,hd,pos0", [(1, 1, 1, 16, 0), (2, 821, 32, 80, 3)], ids=["smallest", "second-trip-hd80"])
def test_rope_backward(dev, B, S, H, hd, pos0):
    from bridgelang_amd import train_ops as T
    from oracle.restate import rope_tables
    D = 3 * H * hd
    dqkv = rand_bf16((B * S, D), 6)
    cos, sin = rope_tables(hd, pos0 + S, 10000.0)
    G = win(dqkv, dev)                                                # ld = 3·H·hd + 16 > 3·H·hd
    T.rope_backward(G.v, cos.to(bf16).to(dev), sin.to(bf16).to(dev), B=B, S=S, H=H, head_dim=hd, pos0=pos0)
    got = G.check("gpu rope bwd")
    ref, mag = T64.rope_backward(dqkv, cos, sin, B, S, H, hd, pos0)
    T64.assert_bf16_close(got, ref, mag, 2, "gpu rope bwd")
    assert torch.equal(got[:, 2 * H * hd:], dqkv[:, 2 * H * hd:])     # the v third is untouched, bit for bit


@pytest.mark.parametrize("n", [8, 8 * (2048 * 256 + 13)], ids=["smallest", "second-trip"])
def test_scale(dev, n):
    from bridgelang_amd import train_ops as T
    x = rand_bf16((n,), 5)
    s = 0.3
    X, out = Flat(n, dev, bf16, x), Flat(n, dev, bf16)
    T.scale(X.v, s, out.v)
    s32 = torch.tensor(s, dtype=f32)
    got = out.check("gpu scale").float()
    T64.assert_bf16_close(got, x.double() * s32.double(), (x.double() * s32.double()).abs(), 2, "gpu scale")
    assert torch.equal(got, (x * s32).to(bf16).float())            # and the fp32 restatement bit for bit


@pytest.mark.parametrize("rows,cols,p", [(1, 8, 0.5), (513, 8200, 0.1)], ids=["smallest", "second-trip"])
def test_dropout(dev, rows, cols, p):
    """The exact host restatement of the mask (oracle.synth.dropout_keep), on windows and past the grid-stride loop's first trip."""
    from bridgelang_amd import train_ops as T
    from oracle.synth import dropout_keep
    x, u, dx0 = rand_bf16((rows, cols), 1), rand_bf16((rows, cols), 2), rand_bf16((rows, cols), 3)
    seed = torch.tensor([41], dtype=torch.int32, device=dev)
    X, O = win(x, dev), Win(rows, cols, dev)
    T.dropout(X.v, O.v, p, seed, 7)
    keep = torch.from_numpy(dropout_keep(41, 7, rows, cols, p))
    inv = torch.tensor(1.0 / (1.0 - p), dtype=f32)
    rb = lambda t: t.to(bf16).float()
    assert torch.equal(O.check("gpu dropout"), torch.where(keep, rb(x * inv), torch.zeros(())))
    Uw, DX = win(u, dev), win(dx0, dev)
    T.dropout_grad_fix(Uw.v, DX.v, p, seed, 7)
    assert torch.equal(DX.check("gpu dropout_grad_fix"), rb(dx0 + torch.where(keep, rb(u * (inv - 1.0)), -u)))


# ---- cross-entropy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 2048, 2056, 32064])
def test_cross_entropy_backward(dev, n):
    from bridgelang_amd import ops, train_ops as T
    rows = 12
    logits, tgt = ce_case(rows, n)
    one = torch.full((rows,), -100, dtype=torch.int64)
    one[7] = tgt[7]                                                 # a batch with exactly one valid row
    for targets in (tgt, one):
        L, D = win(logits, dev, f32), Win(rows, n, dev)
        Tg = targets.to(dev)
        row_loss, mc = torch.empty(rows, device=dev), Flat(2, dev)
        ops.cross_entropy(L.v, Tg, row_loss, mc.v)
        T.cross_entropy_backward(L.v, Tg, mc.v, D.v)
        ref = T64.cross_entropy(logits, targets)
        m = mc.check("gpu ce mean and count").double()
        assert m[1].item() == ref["count"]
        T64.assert_f32_close(m[0], ref["mean"], ref["m_mean"], T64.C_CE_MEAN, "gpu ce mean")
        dl = D.check("gpu ce bwd")
        T64.assert_bf16_close(dl, ref["dl"], ref["mag"], T64.C_CE, "gpu ce dlogits")
        assert bool((bits(dl.to(bf16))[targets == -100] == 0).all())       # ignored rows: exact (+0) zeros


# ---- small-output TN GEMM ------------------------------------------------------------------------------------------------------
def _run_tn(dev, Pw, Qw, R, N, trans, alpha, ws_floats, what):
    from bridgelang_amd import train_ops as T
    C = Flat(R * N, dev)
    ws = Flat(ws_floats, dev) if ws_floats else None
    T.gemm_tn_small(Pw.v, Qw.v, C.v.view((N, R) if trans else (R, N)), trans, ws.v if ws else None, alpha=alpha)
    torch.cuda.synchronize()
    if ws:
        ws.check(f"{what} workspace", finite=False)
    got = C.check(what).double().view((N, R) if trans else (R, N))
    return got.t() if trans else got


@pytest.mark.parametrize("R", [64, 128, 192])
def test_gemm_tn_small(dev, R):
    for N in (64, 192):
        for Tn in (1, 31, 32, 33, 192, 193, 389):
            Pm, Q = rand_bf16((Tn, R), Tn + R), rand_bf16((Tn, N), N + Tn)
            Pw, Qw = win(Pm, dev), win(Q, dev)
            for alpha in (1.0, 0.25):
                ref, mag = T64.gemm_tn(Pm, Q, alpha)
                for trans in (False, True):
                    for ws_floats in (0, 2 * R * N):
                        assert T64.tn_splits(Tn, R, N, ws_floats) == 1
                        got = _run_tn(dev, Pw, Qw, R, N, trans, alpha, ws_floats, f"gpu gemm_tn_small T {Tn} R {R} N {N}")
                        T64.assert_f32_close(got, ref, mag, Tn + T64.C_TN_EXTRA, f"gpu gemm_tn_small{' transposed' if trans else ''}")


@pytest.mark.parametrize("Tn,ws_mult,short,splits", [(512, 2, 0, 2), (512, 2, 1, 1), (1030, 4, 0, 4), (1030, 4, 1, 2)])
def test_gemm_tn_small_splits(dev, Tn, ws_mult, short, splits):
    """Split-T partials summed by reduce_partials_kernel: 2 and 4 splits by the launcher's rule, and one float short of
    the next doubling."""
    R, N = 64, 64
    ws_floats = ws_mult * R * N - short
    assert T64.tn_splits(Tn, R, N, ws_floats) == splits
    Pm, Q = rand_bf16((Tn, R), Tn + R), rand_bf16((Tn, N), N + Tn)
    Pw, Qw = win(Pm, dev), win(Q, dev)
    ref, mag = T64.gemm_tn(Pm, Q, 0.25)
    for trans in (False, True):
        got = _run_tn(dev, Pw, Qw, R, N, trans, 0.25, ws_floats, f"gpu gemm_tn_small T {Tn} {splits} splits")
        T64.assert_f32_close(got, ref, mag, Tn + T64.C_TN_EXTRA, "gpu gemm_tn_small split")


# ---- embedding scatter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 4096])
def test_embed_backward(dev, dim):
    from bridgelang_amd import train_ops as T
    B, L, V = 3, 7, 50
    g = torch.Generator().manual_seed(dim)
    mixed = torch.randint(1, V - 1, (B, L), generator=g)
    mixed[0, 0], mixed[1, 3], mixed[2, 6] = 0, V - 1, 0                 # rows 0 and V − 1
    for ids, NP in ((mixed, 4), (torch.full((B, L), 17), 4), (mixed, 0)):   # all ids equal: the heaviest collision; no patches
        dx, dw0 = rand_bf16((B, L + NP, dim), 1), rand_bf16((V, dim), 2)
        DW = Flat(V * dim, dev, f32, dw0)
        T.embed_backward(ids.to(dev), dx.to(bf16).to(dev), DW.v.view(V, dim), NP)
        got = DW.check("gpu embed bwd").view(V, dim)
        ref, mag, hits = T64.embed_backward(ids, dx, dw0, NP)
        T64.assert_f32_close(got.double(), ref, mag, (hits + 1).view(-1, 1), "gpu embed bwd")
        assert torch.equal(bits(got)[hits == 0], bits(dw0)[hits == 0])  # rows no id names stay exactly as they were


# ---- optimizer -------------------------------------------------------------------------------------------------------------------
def test_sumsq_and_clip(dev):
    from bridgelang_amd import train_ops as T
    nblocks = 4
    base = torch.randn(8195 + 8, generator=torch.Generator().manual_seed(3))
    G = base.to(dev)
    for n in (1, 3, 5, 1023, 8195):
        for off in (0, 1):                                          # off 1: a misaligned view, the scalar path
            g = G[off:off + n]
            part = Flat(nblocks, dev)
            T.sumsq_partial(g, part.v)
            got = part.check("gpu sumsq partials").double().sum()
            ref = T64.sumsq(base[off:off + n])
            chain = (n + 4 * 256 * nblocks - 1) // (4 * 256 * nblocks) + 3 if off == 0 else (n + 256 * nblocks - 1) // (256 * nblocks)
            T64.assert_f32_close(got, ref, ref, chain + 16, f"gpu sumsq{' unaligned' if off else ''}")
    part = Flat(nblocks, dev)
    T.sumsq_partial(G[:8195], part.v)
    pv = part.check("gpu sumsq partials").double()
    norm = float(torch.sqrt(pv.sum()))
    for max_norm in (1e3, 0.5):                                     # the norm (≈ 90) below and above max_norm
        nc = Flat(2, dev)
        T.clip_coef(part.v, max_norm, nc.v)
        out = nc.check("gpu clip coef").double()
        one = torch.ones((), dtype=torch.float64)
        T64.assert_f32_close(out[0], torch.tensor(norm, dtype=torch.float64), norm * one, 1, "gpu clip norm")
        T64.assert_f32_close(out[1], torch.tensor(T64.clip_coef(norm, max_norm), dtype=torch.float64), one, 4, "gpu clip coef")
        assert (out[1].item() == 1.0) == (max_norm > norm)


@pytest.mark.parametrize("step", [1, 1000])
def test_adamw(dev, step):
    from bridgelang_amd import train_ops as T
    n = 1003
    p0, m0, v0, g = adam_case(n)
    hp = ADAM_HP
    for wd in (0.0, hp["wd"]):
        for coef in (None, 0.37):
            for with_bf in (False, True):
                Pp, M, V, Gg = (Flat(n, dev, f32, t) for t in (p0, m0, v0, g))
                nc = torch.tensor([123.0, coef], device=dev) if coef is not None else None
                pb = Flat(n, dev, bf16) if with_bf else None
                T.adamw(Pp.v, M.v, V.v, Gg.v, step, hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=wd,
                        norm_coef=nc, p_bf16=pb.v if pb else None)
                c32 = float(torch.tensor(coef if coef is not None else 1.0, dtype=f32))
                ref = T64.adamw_step(p0, m0, v0, g, step, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, coef=c32)
                pn = Pp.check("gpu adamw p")
                T64.assert_f32_close(pn.double(), ref["p"], ref["m_p"], T64.C_ADAM_P, "gpu adamw p")
                T64.assert_f32_close(M.check("gpu adamw m").double(), ref["m"], ref["m_m"], T64.C_ADAM_M, "gpu adamw m")
                T64.assert_f32_close(V.check("gpu adamw v").double(), ref["v"], ref["m_v"], T64.C_ADAM_V, "gpu adamw v")
                assert torch.equal(bits(Gg.check("gpu adamw g")), bits(g))
                if pb:                                               # the bf16 copy is the RNE rounding of the kernel's own fp32 result
                    assert torch.equal(bits(pb.check("gpu adamw p_bf16")), bits(pn.to(bf16)))


# ---- exact movers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,stride,offset", [(1, 3, 2), (256, 300, 7)])
def test_map_rows(dev, group, stride, offset):
    from bridgelang_amd import train_ops as T
    rows, cols = 2 * group + (0 if group > 1 else 3), 72
    big_rows = ((rows - 1) // group) * stride + offset + group + 5
    m = (torch.arange(rows) // group) * stride + offset + torch.arange(rows) % group
    small, big = rand_bf16((rows, cols), 1), rand_bf16((big_rows, cols), 2)
    Sg, Bg = Win(rows, cols, dev), win(big, dev)                      # gather: small[r] ← big[m[r]]
    T.map_rows(Bg.v, Sg.v, rows=rows, group=group, stride=stride, offset=offset, scatter=False)
    assert torch.equal(Sg.check("gpu map_rows gather"), big[m])
    Ss, Bs = win(small, dev), Win(big_rows, cols, dev)                # scatter: big[m[r]] ← small[r]; other rows keep the sentinel
    T.map_rows(Ss.v, Bs.v, rows=rows, group=group, stride=stride, offset=offset, scatter=True)
    torch.cuda.synchronize()
    got = Bs.buf.cpu()
    want = Bs.before.cpu()
    want[m, PAD:PAD + cols] = small.to(bf16)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("members", [1, 2, 3])
@pytest.mark.parametrize("interleave", [False, True])
def test_lora_block_mask(dev, interleave, members):
    from bridgelang_amd import train_ops as T
    rp, n = 8, 6 * members
    R = rp * members
    g0 = torch.randn(n, R, generator=torch.Generator().manual_seed(members))
    G = Flat(n * R, dev, f32, g0)
    T.lora_block_mask(G.v.view(n, R), rp, members, interleave)
    row, col = torch.arange(n).view(-1, 1), torch.arange(R).view(1, -1)
    mem = (row % members) if interleave else (row // (n // members))
    want = torch.where(col // rp == mem, g0, torch.zeros(()))
    assert torch.equal(bits(G.check("gpu lora_block_mask").view(n, R)), bits(want))


def _cast_specials():
    one = 1.0
    v = [one + 2.0 ** -8, one + 3 * 2.0 ** -8, -(one + 2.0 ** -8), one + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0, float("inf"), -float("inf"),
         NAN, 1e-40, -1e-40, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 3.3895e38, 65504.0]
    return torch.tensor(v, dtype=f32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099])
def test_cast(dev, n):
    """fp32 → bf16 is round to nearest even (exact ties, ±0, ±inf, NaN, denormals included), bf16 → fp32 is exact."""
    from bridgelang_amd import train_ops as T
    sp = _cast_specials()
    src = torch.randn(n, generator=torch.Generator().manual_seed(n))
    if n >= 8:
        k = min(n, len(sp))
        src[:k] = sp[:k]
    else:
        src[:] = sp[n:2 * n]
    S, D = Flat(n, dev, f32, src), Flat(n, dev, bf16)
    T.cast(S.v, D.v)
    got, want = D.check("gpu cast f32 → bf16", finite=False), src.to(bf16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got.float()), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])
    B, F = Flat(n, dev, bf16, want), Flat(n, dev, f32)
    T.cast(B.v, F.v)
    back = F.check("gpu cast bf16 → fp32", finite=False)
    assert torch.equal(torch.isnan(back), nan) and torch.equal(bits(back)[~nan], bits(want.float())[~nan])


@pytest.mark.parametrize("n", [1, 3, 4099])
def test_axpy(dev, n):
    """y += a·x. One fp32 ulp: the product's rounding (absent when contracted to an FMA) and the sum's."""
    from bridgelang_amd import train_ops as T
    g = torch.Generator().manual_seed(n)
    y0, x = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a = 0.3
    Y, X = Flat(n, dev, f32, y0), Flat(n, dev, f32, x)
    T.axpy(Y.v, X.v, a)
    a32 = float(torch.tensor(a, dtype=f32))
    ref = y0.double() + a32 * x.double()
    T64.assert_f32_close(Y.check("gpu axpy").double(), ref, (a32 * x.double()).abs() + ref.abs(), 1, "gpu axpy")
    assert torch.equal(bits(X.check("gpu axpy x")), bits(x))


@pytest.mark.parametrize("n", [1, 15, 17, 4099])
def test_fill_zero_and_copy_bytes(dev, n):
    from bridgelang_amd import train_ops as T
    guard = 32
    data = torch.randint(1, 255, (n + 1,), dtype=torch.uint8, generator=torch.Generator().manual_seed(n))
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    T.fill_zero(buf[:n])
    assert bool((buf[:n] == 0).all()) and bool((buf[n:] == 0xA5).all())
    src = data.to(dev)
    for off in (0, 1):                                              # off 1: an unaligned source, the byte path
        dst = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
        T.copy_f32(src[off:off + n], dst[:n])
        want = data[off:off + n]
        assert torch.equal(dst[:n].cpu(), want) and bool((dst[n:] == 0xA5).all())


def test_batched_ops(dev):
    """Five mixed entries in one launch, each bit-identical to the stand-alone op it replaces; the kernel's binary search
    lands on the first (a 1-block copy), interior (a scaled pack and a scaled transposing pack into destination windows, a
    multi-block copy) and last (an unaligned byte copy) entry; what the table does not name is not touched."""
    from bridgelang_amd import train_ops as T
    s1, s2 = 0.5, 0.3
    small = torch.randn(100, generator=torch.Generator().manual_seed(1)).to(dev)
    large = torch.randn(300_000, generator=torch.Generator().manual_seed(2)).to(dev)
    raw = torch.randint(0, 255, (1001,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev)
    w = rand_bf16((64, 96), 4).to(bf16).to(dev)                        # [N, K] → k-blocks [2, 5) of kt_total = 6
    a = rand_bf16((70, 128), 5).to(bf16).to(dev)                       # [rows, cols] → k-blocks [1, 4) of kt_total = 5 (rows_pad 96)
    wwin, awin = win(w.float().cpu(), dev), win(a.float().cpu(), dev)  # strided sources
    outs = {}
    for mode in ("batched", "alone"):
        d_small = torch.full((100 + 8,), NAN, device=dev)
        d_large = torch.full((300_000 + 8,), NAN, device=dev)
        d_raw = torch.full((1001 + 32,), 0xA5, dtype=torch.uint8, device=dev)
        pk_w = torch.full((64 // 16, 6, 64, 8), NAN, dtype=bf16, device=dev)
        pk_a = torch.full((128 // 16, 5, 64, 8), NAN, dtype=bf16, device=dev)
        if mode == "batched":
            entries = [T.be_copy(small, d_small[:100]), T.be_pack(wwin.v, pk_w, kt_total=6, kb_offset=2, scale=s1),
                       T.be_transpose_pack(awin.v, pk_a, 96, kt_total=5, kb_offset=1, scale=s2), T.be_copy(large, d_large[:300_000]),
                       T.be_copy(raw[1:1001], d_raw[:1000])]
            assert entries[0][0].nblocks == 1 and entries[3][0].nblocks > 1
            T.batched(entries, dev)
        else:
            T.copy_f32(small, d_small[:100])
            tw, ta = torch.empty_like(w), torch.empty_like(a)
            T.scale(w, s1, tw)
            T.pack_into(tw, pk_w, 6, 2)
            T.scale(a, s2, ta)
            T.transpose_pack_into(ta, pk_a, 96, 5, 1)
            T.copy_f32(large, d_large[:300_000])
            T.copy_f32(raw[1:1001], d_raw[:1000])
        torch.cuda.synchronize()
        outs[mode] = [t.cpu() for t in (d_small, d_large, d_raw, pk_w, pk_a)]
    for got, want in zip(outs["batched"], outs["alone"]):
        assert torch.equal(bits(got), bits(want))
    d_small, d_large, d_raw, pk_w, pk_a = outs["batched"]
    assert torch.equal(d_small[:100], small.cpu()) and torch.isnan(d_small[100:]).all()
    assert torch.equal(d_large[:300_000], large.cpu()) and torch.isnan(d_large[300_000:]).all()
    assert torch.equal(d_raw[:1000], raw[1:1001].cpu()) and bool((d_raw[1000:] == 0xA5).all())
    assert torch.isnan(pk_w.float()[:, :2]).all() and torch.isnan(pk_w.float()[:, 5:]).all() and torch.isfinite(pk_w.float()[:, 2:5]).all()
    assert torch.isnan(pk_a.float()[:, :1]).all() and torch.isnan(pk_a.float()[:, 4:]).all() and torch.isfinite(pk_a.float()[:, 1:4]).all()
    wwin.check("gpu batched pack source")
    awin.check("gpu batched transpose-pack source")
