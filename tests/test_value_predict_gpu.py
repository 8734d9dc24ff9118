"""bl_value_predict_f32 (csrc/value.hip): the critic at inference, final RMSNorm and value head in one launch.

It is defined by composition, so the first check is bit identity with the two ops it restates: `ops.rmsnorm` → hn, then
`train_ops.value_head` over hn with every row a value row (token level, unclipped); column 0 of value_rows must be `out`,
fp32 bit for bit. The second check holds the result to the fp64 definition (`value_loss.value_loss`) on the device's own bf16
hn within the `v` bound tests/test_value_head_gpu.py derives (C_V = 8·ceil(dim/512) + 7 against Σ|hn||w| + |b|; the helper is
imported, no number is copied). Then: nothing but the rows and columns of the shape is read, nothing but out[r·out_stride] is
written, every rejection launches nothing, and a captured graph follows its inputs.

Shapes: dim 8 (the minimum), 520 (one full chunk of 512 and a partial one), 4096 (7B), 5120 (NCH = 10, the limit / 13B);
rows 1, 5, 16, 17 (a partial workgroup on either side of 4 and of 16); ldx = dim, dim + 8 and 10·dim (the un-padded plan's
S·D row stride); out_stride 1 and 3."""
import numpy as np
import pytest
import torch

from bridgelang_amd import _lib, ops, train_ops as T
from bridgelang_amd.training.value_loss import ValueLossConfig, value_loss
from test_value_head_gpu import value_tolerances

pytestmark = pytest.mark.gpu

EPS = 1e-6
DIMS, ROWS = (8, 520, 4096, 5120), (1, 5, 16, 17)
SENTINEL = 1234.5
CFG = ValueLossConfig(coef=1.0, clip=None, level="token")


def lds(dim):
    return (dim, dim + 8, 10 * dim)


def make_inputs(dim, rows, seed=0):
    """Host tensors: x [rows, dim] bf16 with rows at scales 1e-3, 1, 1e3 and one all-zero row (rstd = 1/sqrt(eps)), norm
    weights of both signs, a drawn head (std 0.05) with a non-zero bias."""
    g = torch.Generator().manual_seed(1000 * dim + rows + seed)
    scale = torch.tensor([1e-3, 1.0, 1e3])[torch.arange(rows) % 3][:, None]
    x = (torch.randn(rows, dim, generator=g) * scale).to(torch.bfloat16)
    if rows > 1:
        x[1] = 0
    elif seed == 1:              # rows == 1: the zero row is the seed-1 variant
        x[0] = 0
    nw = (torch.randn(dim, generator=g) * 0.5 + 0.25).to(torch.bfloat16)
    assert dim < 16 or (bool((nw > 0).any()) and bool((nw < 0).any()))
    w = (torch.randn(dim, generator=g) * 0.05).to(torch.bfloat16)
    b = torch.tensor([0.375 if seed % 2 == 0 else -1.625], dtype=torch.bfloat16)
    return x, nw, w, b


def padded(x, ld, dev, extra_rows=3):
    """x inside a NaN-filled [rows + extra_rows, ld] device buffer: columns [dim, ld) and the rows behind are poison."""
    rows, dim = x.shape
    buf = torch.full((rows + extra_rows, ld), float("nan"), dtype=torch.bfloat16)
    buf[:rows, :dim] = x
    return buf.to(dev)[:rows, :dim]


def composition(x_dev, nw, w, b, eps=EPS):
    """The two existing ops in sequence → (hn bf16 [rows, dim], v fp32 [rows])."""
    rows, dim = x_dev.shape
    dev = x_dev.device
    hn = torch.empty(rows, dim, dtype=torch.bfloat16, device=dev)
    ops.rmsnorm(x_dev, nw, hn, eps)
    idx, cnt = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    vrows, stats = torch.empty(rows, 4, dtype=torch.float32, device=dev), torch.empty(8, dtype=torch.float32, device=dev)
    T.value_head(hn, torch.full((rows,), 5, dtype=torch.int64, device=dev), w, b, torch.zeros(rows, device=dev), None, CFG,
                 idx, cnt, vrows, stats)
    return hn, vrows[:, 0].clone()


def predict(x_dev, nw, w, b, out_stride):
    """→ (out view [rows], the whole sentinel-filled buffer)."""
    rows = x_dev.shape[0]
    buf = torch.full((rows * out_stride + 5,), SENTINEL, dtype=torch.float32, device=x_dev.device)
    out = buf[:rows * out_stride:out_stride]
    T.value_predict(x_dev, nw, EPS, w, b, out)
    return out, buf


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_composition_definition_and_bounds(dev, dim, rows):
    for seed in ((0, 1) if rows == 1 else (0,)):
        x, nw, w, b = make_inputs(dim, rows, seed)
        nw_d, w_d, b_d = nw.to(dev), w.to(dev), b.to(dev)
        ref = None
        for ld in lds(dim):
            x_d = padded(x, ld, dev)
            hn, want = composition(x_d, nw_d, w_d, b_d)
            if ref is None:      # the fp64 definition on the device's own hn, once per shape
                h64 = hn.float().cpu().double().numpy()
                res = value_loss(h64, np.full(rows, 5, dtype=np.int64), w.double().numpy(), float(b), np.zeros(rows), None, CFG)
                tol, _, _ = value_tolerances(h64, w.double().numpy(), float(b), np.zeros(rows), None, res, CFG.coef)
                ref = (res.value, tol["v"], want.clone())
                assert np.isfinite(res.value).all()
            assert torch.equal(want.view(torch.int32), ref[2].view(torch.int32)), "the composition itself depends on ldx"
            for out_stride in (1, 3):
                out, buf = predict(x_d, nw_d, w_d, b_d, out_stride)
                torch.cuda.synchronize()
                # 1. bit identity with the composition
                assert torch.equal(out.view(torch.int32), want.view(torch.int32)), \
                    f"dim {dim} rows {rows} ldx {ld} out_stride {out_stride}: max |Δ| {float((out - want).abs().max())}"
                # 2. the fp64 definition within the derived bound
                err = np.abs(out.cpu().double().numpy() - ref[0])
                assert (err <= ref[1] + 2.0 ** -116).all(), (err.max(), ref[1].min())
                # 3. nothing else read (the NaNs around x would show) or written (the sentinels)
                assert bool(torch.isfinite(out).all())
                mask = torch.ones_like(buf, dtype=torch.bool)
                mask[:rows * out_stride:out_stride] = False
                assert bool((buf[mask] == SENTINEL).all())
    if rows > 1:
        assert float(want[1]) == float(b.float())        # the all-zero row: hn = 0, v = b exactly


def test_argument_checks(dev):
    lib = _lib.load()
    dim, rows = 520, 5
    x, nw, w, b = (t.to(dev) for t in make_inputs(dim, rows))
    big = torch.zeros(rows, 5128 + 8, dtype=torch.bfloat16, device=dev)
    out = torch.full((rows * 3,), SENTINEL, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(x=x, ldx=dim, rows=rows, dim=dim, nw=nw, w=w, b=b, out=out, stride=1, off=(0, 0, 0)):
        p = lambda t, o=0: None if t is None else t.data_ptr() + o
        return lib.bl_value_predict_f32(p(x, off[0]), ldx, rows, dim, p(nw, off[1]), EPS, p(w, off[2]), p(b), p(out), stride, s)

    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    for name in ("x", "nw", "w", "b", "out"):
        assert call(**{name: None}) == _lib.BL_E_ARG, name
    for kw in (dict(rows=0), dict(rows=-1), dict(dim=516), dict(dim=0), dict(x=big, ldx=5136, dim=5128), dict(stride=0), dict(stride=-3)):
        assert call(**kw) == _lib.BL_E_SHAPE, kw
    for kw in (dict(off=(2, 0, 0)), dict(off=(0, 8, 0)), dict(off=(0, 0, 6)), dict(ldx=dim + 4)):
        assert call(**kw) == _lib.BL_E_ALIGN, kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a rejected call launched"
    with pytest.raises((ValueError, TypeError)):
        T.value_predict(x, nw, EPS, w[:-8], b, out[:rows])
    with pytest.raises((ValueError, TypeError)):
        T.value_predict(x, nw, EPS, w, b, out[:rows].double())


def test_graph_capture_follows_its_inputs(dev):
    dim, rows, ld = 4096, 5, 10 * 4096
    x, nw, w, b = make_inputs(dim, rows)
    x_d, nw_d, w_d, b_d = padded(x, ld, dev), nw.to(dev), w.to(dev), b.to(dev)
    out = torch.full((rows,), SENTINEL, dtype=torch.float32, device=dev)
    op = T.value_predict(x_d, nw_d, EPS, w_d, b_d, out)          # warm-up launch outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        op.run()
    for seed in (0, 2, 3):
        x2, nw2, w2, b2 = make_inputs(dim, rows, seed)
        x_d.copy_(x2.to(dev)); nw_d.copy_(nw2.to(dev)); w_d.copy_(w2.to(dev)); b_d.copy_(b2.to(dev))
        out.fill_(SENTINEL)
        g.replay()
        got = out.clone()
        want, _ = predict(x_d, nw_d, w_d, b_d, 1)
        _, comp = composition(x_d, nw_d, w_d, b_d)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got.view(torch.int32), comp.view(torch.int32))
    assert not torch.equal(got, torch.full_like(got, SENTINEL))
