"""gemm288s_kernel's three-phase K loop (24 MFMAs per phase, three slots per K-tile, LDS-DMA pieces 2 / 3 / 4 with the
weight pieces of K-tile T+2 issued in the last slot of T): K-tile counts from the smallest reachable to the real
down_proj's 172, ragged edges, three rounds, every epilogue family the launcher instantiates the kernel for. Each case is
checked four ways: every output element written (NaN pre-fill), the oracle's arithmetic on sampled rows, bit identity with
the same rows computed one 288-row sequence at a time (the mid kernels: same K order), and bit identity of two
consecutive calls — a fragment read that overtakes its LDS-DMA piece, or a piece that overwrites rows still being read,
shows up as a run-to-run difference first.

All cases have M = 4608 or 4591: the planner picks the 288-row tiling only where it removes a leftover round of 256-row
tiles, and K >= 512."""
import pytest
import torch

from conftest import rand_bf16
from oracle import restate as R
from test_ops_gpu import close_bf16, dv, pk

pytestmark = pytest.mark.gpu

P = R.Prec(True)

CASES = [
    (4608, 4096, 512, "none"),       # nk = 8: the smallest K the planner sends here
    (4608, 4096, 640, "bias"),       # nk = 10: an odd number of (two-K-tile) loop iterations
    (4608, 4096, 1152, "res"),       # nk = 18
    (4608, 4096, 11008, "res"),      # the real down_proj: 172 K-tiles, 86 stage flips per stage
    (4591, 4000, 640, "none"),       # partial last row tile (zero-size descriptor rows), ragged N: per-store epilogue
    (4591, 4000, 640, "res"),        # the same edges through a residual read
    (4608, 12288, 512, "bias"),      # 768 tiles = three rounds
    (4608, 4096, 512, "swiglu"),
    (4608, 4096, 512, "f32"),        # fp32 output
]


@pytest.mark.parametrize("M,N,K,epi", CASES)
def test_gemm288_three_phase_loop(dev, M, N, K, epi):
    from bridgelang_amd import ops
    a, w = rand_bf16((M, K), 1), rand_bf16((N, K), 2, 0.05)
    A = dv(a, dev)
    sel = torch.cat([torch.arange(0, 200), torch.arange(2200, 2400), torch.arange(M - 200, M)])
    cols, dtype, kw = N, torch.bfloat16, {}
    if epi == "swiglu":
        cols = N // 2
        W = pk(torch.stack([w[:cols], w[cols:]], 1).reshape(N, K), dev)
        e = ops.EPI_SWIGLU
        g, u = R.linear(P, a[sel], w[:cols]), R.linear(P, a[sel], w[cols:])
        ref = P.rb(P.rb(torch.nn.functional.silu(g)) * u)
    elif epi == "f32":
        W, e, dtype = pk(w, dev), ops.EPI_F32, torch.float32
        ref = a[sel] @ w.t()
    elif epi == "res":
        r = rand_bf16((M, N), 4)
        W, e, kw = pk(w, dev), ops.EPI_RES, {"res": dv(r, dev)}
        ref = P.rb(r[sel] + R.linear(P, a[sel], w))
    elif epi == "bias":
        b = rand_bf16((N,), 3, 0.1)
        W, e, kw = pk(w, dev), ops.EPI_BIAS, {"bias": dv(b, dev)}
        ref = R.linear(P, a[sel], w, b)
    else:
        W, e = pk(w, dev), ops.EPI_NONE
        ref = R.linear(P, a[sel], w)
    what = f"gemm288 three-phase {M}x{N}x{K} {epi}"

    out = torch.full((M, cols), float("nan"), dtype=dtype, device=dev)
    ops.gemm(A, W, out, e, **kw)
    assert ops.gemm_last_form() == "gemm288s"
    assert not torch.isnan(out).any(), f"{what}: an output element was never written"

    again = torch.full((M, cols), float("nan"), dtype=dtype, device=dev)
    ops.gemm(A, W, again, e, **kw)
    assert ops.gemm_last_form() == "gemm288s"
    assert torch.equal(again, out), f"{what}: two consecutive calls differ"

    if epi == "f32":
        assert torch.allclose(out[sel].cpu(), ref, rtol=1e-4, atol=1e-4 * ref.abs().max().item()), what
    else:
        close_bf16(out[sel], ref, what)

    for s0 in (0, 288 * 7, M - 288 - (M % 288 and 5)):              # one 288-row sequence at a time: the mid kernels
        one = torch.full((288, cols), float("nan"), dtype=dtype, device=dev)
        kw1 = {k: (v[s0:s0 + 288] if k == "res" else v) for k, v in kw.items()}
        ops.gemm(A[s0:s0 + 288], W, one, e, **kw1)
        assert ops.gemm_last_form().startswith("mid2<")
        assert torch.equal(one, out[s0:s0 + 288]), f"{what}: rows {s0}..: result depends on the tiling"
