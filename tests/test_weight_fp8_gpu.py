"""bl_quantize_weight_fp8_packed / _batched (csrc/quantize_weight_fp8.hip): packed bf16 weight → packed e4m3 weight + scales,
bit for bit against the quantiser specification and the independent layout definition of fp8_ref64 (quantize_spec,
weight_image, check_quantised).

Data: Gaussian bf16 (std 0.02) whose row r is scaled by one of sixteen magnitudes 2^-20 … 2^20, a different one for each
row of every 16-row tile (a per-tile amax instead of a per-row one fails on every tile), with planted rows in the last tile:
0 all zero; 1 ±2^-120, below the live threshold (signed-zero codes, scale 1); 2 only the last column non-zero; 3 only the
first; 4 holds the largest finite bf16; 5 Gaussian with -0.0 entries; 6 all -0.0. Outputs are pre-filled with 0x7F bytes
and NaN scales and sit between guard regions."""
import pytest
import torch

import fp8_ref64 as F
from test_fp8_ref_cpu import gemm_operands

pytestmark = pytest.mark.gpu
bf16, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
NAN = float("nan")
GUARD = 256                      # bytes on either side of an output
BF16_MAX = 3.3895313892515355e38

SHAPES = [(16, 128),             # one tile, two e4m3 fragments
          (48, 384),             # odd tile count, k/64 = 6
          (32, 11008),           # k/128 = 86: beyond the register-resident part, not a power of two
          (4608, 512)]           # 288 tiles


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def make_weight(n: int, k: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * 0.02
    r = torch.arange(n) % 16
    w = w * torch.pow(2.0, ((r * 7) % 16).float() * (40.0 / 15.0) - 20.0)[:, None]      # sixteen distinct magnitudes per tile
    t = n - 16
    w[t + 0] = 0.0
    w[t + 1] = torch.where(torch.arange(k) % 2 == 0, 1.0, -1.0) * 2.0 ** -120
    w[t + 2] = 0.0
    w[t + 2, k - 1] = 0.37
    w[t + 3] = 0.0
    w[t + 3, 0] = -1.5
    w[t + 4, k // 2 + 5] = BF16_MAX
    w[t + 5, torch.arange(0, k, 3)] = -0.0
    w[t + 6] = -0.0
    w = w.to(bf16)
    assert bool(torch.isfinite(w.float()).all()) and float(w[t + 4].float().abs().max()) == BF16_MAX
    assert bool(torch.signbit(w[t + 6].float()).all()) and float(w[t + 1].float().abs().max()) == 2.0 ** -120
    return w


class Out:
    """w8 (n·k bytes) and scale ([n] fp32) inside 0x7F- / NaN-filled buffers with guard regions."""

    def __init__(self, n, k, dev):
        self.n, self.k = n, k
        self.qbuf = torch.full((GUARD + n * k + GUARD,), 0x7F, dtype=u8, device=dev)
        self.sbuf = torch.full((GUARD // 4 + n + GUARD // 4,), NAN, dtype=f32, device=dev)
        self.w8 = self.qbuf[GUARD:GUARD + n * k]
        self.scale = self.sbuf[GUARD // 4:GUARD // 4 + n]
        assert self.w8.data_ptr() % 16 == 0 and self.scale.data_ptr() % 16 == 0

    def guards_intact(self) -> bool:
        q, s, n = self.qbuf, self.sbuf, self.n
        return bool((q[:GUARD] == 0x7F).all()) and bool((q[GUARD + n * self.k:] == 0x7F).all()) and \
            bool(s[:GUARD // 4].isnan().all()) and bool(s[GUARD // 4 + n:].isnan().all())


def check_against_spec(what, w, out):
    n, k = w.shape
    codes, scale, live = F.quantize_spec(w)
    assert out.guards_intact(), f"{what}: wrote outside its outputs"
    F.assert_equal_bytes(out.scale.cpu().view(torch.int32), scale.view(torch.int32), f"{what} scales")
    F.assert_equal_bytes(out.w8.cpu(), F.pack_image(codes), f"{what} image")
    F.assert_equal_bytes(out.w8.cpu().view(bf16).view(n // 16, k // 64, 64, 8).view(torch.int16), F.weight_image(codes).view(torch.int16),
                         f"{what} weight_image")
    got = out.w8.cpu()[F.packed_index(n, k)]                     # code (row, column) wherever the layout puts it
    F.check_quantised(what, w, got, out.scale)
    t = n - 16
    assert not bool(live[t]) and not bool(live[t + 1]) and not bool(live[t + 6]) and int(live.sum()) == n - 3
    assert bool((out.scale.cpu()[~live] == 1.0).all())
    assert bool((got[t] == 0).all()) and bool((got[t + 6] == 0x80).all())
    assert bool((got[t + 1] == torch.where(torch.arange(k) % 2 == 0, 0, 0x80).to(u8)).all())       # signed zeros
    assert int(got[t + 2, k - 1]) == 0x7E and not bool(got[t + 2, :k - 1].any())
    assert int(got[t + 3, 0]) == 0xFE and not bool(got[t + 3, 1:].any())
    assert int(got[t + 4, k // 2 + 5]) == 0x7E
    return codes, scale


@pytest.mark.parametrize("n,k", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_single_call_equals_the_specification(dev, n, k):
    from bridgelang_amd import ops
    w = make_weight(n, k, 10 + n + k)
    wp = ops.pack_weight(w.to(dev))
    out = Out(n, k, dev)
    w8, s, op = ops.quantize_packed_weight_fp8(wp, w8=out.w8, scale=out.scale)
    assert w8 is out.w8 and s is out.scale and op.name == "bl_quantize_weight_fp8_packed"
    check_against_spec(f"quantize_packed {n}x{k}", w, out)
    first = (out.qbuf.clone(), out.sbuf.clone())
    op.run()                                                     # replay into the now dirty buffers: the same bytes
    assert torch.equal(out.qbuf, first[0]) and torch.equal(out.sbuf.view(torch.int32), first[1].view(torch.int32))
    # the allocating form returns the shapes ops.quantize_weight_fp8 returns
    w8b, sb, _ = ops.quantize_packed_weight_fp8(wp)
    assert w8b.dtype == bf16 and tuple(w8b.shape) == (n // 16, k // 64, 64, 8) and tuple(sb.shape) == (n,) and sb.dtype == f32
    assert torch.equal(w8b.view(-1).view(u8), out.w8) and torch.equal(sb.view(torch.int32), out.scale.view(torch.int32))


def test_batched_equals_single_calls(dev):
    from bridgelang_amd import ops, train_ops as T
    shapes = [(48, 384), (16, 4224), (80, 128)]                  # 3 + 1 + 5 items; 4224 = 33·128 spills past the resident part
    ws = [make_weight(n, k, 77 + i) for i, (n, k) in enumerate(shapes)]
    wps = [ops.pack_weight(w.to(dev)) for w in ws]
    single = [Out(n, k, dev) for n, k in shapes]
    for wp, o in zip(wps, single):
        ops.quantize_packed_weight_fp8(wp, w8=o.w8, scale=o.scale)
    batched = [Out(n, k, dev) for n, k in shapes]
    entries = [T.be_quantize_packed(wp, o.w8, o.scale) for wp, o in zip(wps, batched)]
    assert [e[0].n_items for e in entries] == [T.quantize_packed_items(n, k) for n, k in shapes] == [3, 1, 5]
    op = T.quantize_packed_batched(entries, dev, run=False)
    assert op.name == "bl_quantize_weight_fp8_packed_batched" and bool(batched[0].scale.isnan().all())   # run=False: nothing ran
    for rep in range(2):                                         # the second run finds dirty buffers
        op.run()
        for i, (w, a, b) in enumerate(zip(ws, single, batched)):
            assert b.guards_intact()
            assert torch.equal(a.w8, b.w8) and torch.equal(a.scale.view(torch.int32), b.scale.view(torch.int32)), f"entry {i}, run {rep}"
            if rep == 0:
                check_against_spec(f"batched entry {i}", w, b)


def test_gemm_reads_the_kernels_output(dev):
    """bl_gemm_fp8 on (w8, scale) from the kernel equals bl_gemm_fp8 on weight_image(specification codes), bit for bit: integer
    activations |a| <= 8 and integer weights |w| <= 6 of the integer instrument (as bf16 values), EPI_F32."""
    from bridgelang_amd import ops
    M, N, K = 300, 528, 384
    A8, W8, sa, _ = gemm_operands(M, N, K, "real")
    w = F.decode(W8).to(bf16)
    assert torch.equal(w.double(), F.decode(W8))
    codes, scale, _ = F.quantize_spec(w)
    out = Out(N, K, dev)
    ops.quantize_packed_weight_fp8(ops.pack_weight(w.to(dev)), w8=out.w8, scale=out.scale)
    A8, sa = A8.to(dev), sa.to(dev)
    got = torch.full((M, N), NAN, dtype=f32, device=dev)
    want = torch.full((M, N), NAN, dtype=f32, device=dev)
    ops.gemm_fp8(A8, sa, out.w8.view(bf16).view(N // 16, K // 64, 64, 8), out.scale, got, ops.EPI_F32)
    ops.gemm_fp8(A8, sa, F.weight_image(codes).to(dev), scale.to(dev), want, ops.EPI_F32)
    assert out.guards_intact() and bool(torch.isfinite(want).all()) and bool(want.abs().max() > 0)
    F.assert_equal_bytes(got.view(torch.int32), want.view(torch.int32), "gemm_fp8 on the kernel's output")


def test_rejected_arguments(dev):
    from bridgelang_amd import _lib, ops, train_ops as T
    lib = _lib.load()
    n, k = 32, 256
    wp = ops.pack_weight(torch.ones(n, k, dtype=bf16, device=dev))
    out = Out(n, k, dev)
    call = lambda w, n_, k_, q, s: lib.bl_quantize_weight_fp8_packed(w, n_, k_, q, s, None)
    W, Q, S = wp.data_ptr(), out.w8.data_ptr(), out.scale.data_ptr()
    assert call(None, n, k, Q, S) == _lib.BL_E_ARG and call(W, n, k, None, S) == _lib.BL_E_ARG and call(W, n, k, Q, None) == _lib.BL_E_ARG
    for bad_n, bad_k in ((24, k), (0, k), (n, 192), (n, 64), (n, 0), (-16, k), ((1 << 24) + 16, k)):
        assert call(W, bad_n, bad_k, Q, S) == _lib.BL_E_SHAPE, (bad_n, bad_k)
    assert call(W + 2, n, k, Q, S) == _lib.BL_E_ALIGN and call(W, n, k, Q + 8, S) == _lib.BL_E_ALIGN and call(W, n, k, Q, S + 4) == _lib.BL_E_ALIGN
    assert call(W, n, k, W, S) == _lib.BL_E_ARG and call(W, n, k, W + n * k, S) == _lib.BL_E_ARG       # the codes over the input
    assert call(W, n, k, Q, W + 2 * n * k - 16) == _lib.BL_E_ARG and call(W, n, k, Q, Q + 16) == _lib.BL_E_ARG
    assert lib.bl_quantize_weight_fp8_packed_batched(None, 1, None) == _lib.BL_E_ARG
    table = torch.zeros(48, dtype=u8, device=dev)
    assert lib.bl_quantize_weight_fp8_packed_batched(table.data_ptr(), 0, None) == _lib.BL_E_SHAPE
    assert lib.bl_quantize_weight_fp8_packed_batched(table.data_ptr() + 4, 1, None) == _lib.BL_E_ALIGN
    torch.cuda.synchronize()
    assert out.guards_intact() and bool((out.w8 == 0x7F).all()) and bool(out.scale.isnan().all())      # no rejected call launched
    with pytest.raises(ValueError):
        T.be_quantize_packed(ops.pack_weight(torch.ones(16, 192, dtype=bf16, device=dev)), out.w8[:16 * 192], out.scale[:16])
    with pytest.raises(ValueError):
        T.be_quantize_packed(wp, out.w8[:n * k - 16], out.scale)
    with pytest.raises(ValueError):
        T.be_quantize_packed(wp, wp.view(-1).view(u8)[:n * k], out.scale)
    with pytest.raises(ValueError):
        T.quantize_packed_batched([], dev)
    for bad_k in (64, 192):
        with pytest.raises(ValueError):
            ops.quantize_packed_weight_fp8(ops.pack_weight(torch.ones(16, bad_k, dtype=bf16, device=dev)))
    with pytest.raises(_lib.BridgeLangHipError):                 # what Python leaves to the library: the overlap check
        ops.quantize_packed_weight_fp8(wp, w8=wp.view(-1).view(u8)[:n * k], scale=out.scale)
