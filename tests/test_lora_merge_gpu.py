"""bl_lora_merge_bf16 / bl_lora_merge_batched_bf16 (csrc/lora_merge.hip) against the specification of
bridgelang_amd/training/lora.py::merged_reference, per element, on the packed layout.

Reference. `spec()` below restates the definition in fp64 torch on the device (torch's fp64 matmul, train_ref64.rb64 for
the single rounding): sB = bf16(fp32(s)·B), Δ = sB·A (exact products, fp64 sum), W' = bf16(W + Δ), W' = W where Δ == 0.
The small cases check once that it agrees bit for bit with the package's own CPU `merged_reference`.

Dyadic data — bit for bit. W = i/64 (|i| <= 127: eight significand bits), A = i/8 (|i| <= 8), B = j/16 (|j| <= 16),
s = 0.5, so sB = j/32 exactly and every product sB·A is a multiple of 2^-8 with |·| <= 0.5. A partial sum of at most R
products plus W is a multiple of 2^-8 below R/2 + 2; `assert_exact_sums` asserts (R·0.5 + 2)·2^8 <= 2^24, under which
every fp32 partial sum of the MFMA — in any order — and the fp32 add of W are exact. The kernel's single rounding then
acts on the same exact value as the reference's: every element must be equal.

Gaussian data — bounded, and exact away from ties. The products of bf16 values are exact in fp32; the MFMA adds the
R_row products a row sees (its member's rank block, or all R for an interleaved group; skipped blocks are exact zeros) in
some tree of fp32 adds, through which a product passes at most R_row − 1 adds: error <= (R_row − 1)·e·Σ|sB|·|A|. The add of
W is one more fp32 rounding (1·e·|W + Δ| <= e·mag) and the cross term with the final rounding one more: c = R + 1
>= R_row + 1 against mag = |W| + Σ|sB|·|A| (R, the full width, is used for every case: not sharper than needed, never
wider than the longest chain allows). The final rounding bf16(t) acts on an fp32 t within c·e·mag of the fp64 total: where
the total lies within δ = c·e·mag / ulp_bf16(total) ulps of a rounding boundary the two may round apart, and ulp_bf16 is
added to `tie` for exactly those elements (train_ref64.near_tie). Everywhere ELSE the two roundings must agree, so the
test also asserts got == spec on every element outside that mask — train_ref64.assert_bf16_close alone would allow an
ulp anywhere through its u·|ref| term.
"""
import ctypes as C

import pytest
import torch

import train_ref64 as T64
from gemm_ref64 import assert_exact, check_dyadic_values, dyadic, gauss

pytestmark = pytest.mark.gpu

S = 0.5
GUARD = 128                        # bf16 elements (256 bytes) before and after every output buffer
NAN_BITS = 0x7FC1                  # a NaN pattern no kernel produces

# (n, k, R, members, mode, rank, zero-from column of A)
CASES = [
    (16, 32, 64, 1, "single", 64, None),            # one fragment
    (48, 96, 64, 1, "single", 64, None),
    (80, 224, 64, 1, "single", 64, None),           # 35 fragments: a ragged last quad of k-strips
    (96, 64, 192, 3, "concat", 64, None),
    (64, 64, 128, 2, "interleave", 64, None),
    (32, 640, 64, 1, "single", 64, 588),            # K padding: A's columns 588.. are zero
    (12288, 4096, 192, 3, "concat", 32, None),      # 7B q|k|v at rank 32 of 64: a second trip of every grid-stride loop
    (48, 160, 96, 1, "single", 96, None),           # 96 ranks per row: the B block's chunks do not divide by the workgroup
    (32, 64, 32, 1, "single", 32, None),            # one 32-rank chunk
]
BIG = 6


def assert_exact_sums(R: int) -> None:
    assert (R * 0.5 + 2.0) * 2.0 ** 8 <= 2.0 ** 24, f"R = {R}: the dyadic partial sums are not exact in fp32"


def block_mask(n, R, members, mode, rank):
    """1 where B_all may be non-zero: row's own member block, first `rank` of its 64 padded columns."""
    rp = R // members
    rows = torch.arange(n)
    member = rows % members if mode == "interleave" else rows // (n // members)
    cols = torch.arange(R)
    return ((cols[None, :] // rp == member[:, None]) & ((cols % rp)[None, :] < rank)).float()


def make_case(i, dev, kind):
    n, k, R, members, mode, rank, zero_from = CASES[i]
    rp = R // members
    if kind == "dyadic":
        W, A, B = dyadic((n, k), 100 + i, 6, 127), dyadic((R, k), 200 + i, 3, 8), dyadic((n, R), 300 + i, 4, 16)
    else:
        W, A, B = gauss((n, k), 100 + i, 0.02), gauss((R, k), 200 + i, 1.0 / 32), gauss((n, R), 300 + i, 0.05)
    A = A * ((torch.arange(R) % rp) < rank).float()[:, None]
    if zero_from is not None:
        A[:, zero_from:] = 0
        W[:, zero_from:] = 0
    B = B * block_mask(n, R, members, mode, rank)
    if kind == "dyadic":
        check_dyadic_values(W, 6, 127 / 64), check_dyadic_values(A, 3, 1.0), check_dyadic_values(B, 4, 1.0)
        assert_exact_sums(R)
    return tuple(t.to(torch.bfloat16).to(dev) for t in (W, A, B))


def spec(W, A, B, s):
    """(W' as fp64 values, fp64 total, mag) on the arguments' device."""
    sB = (B.float() * s).to(torch.bfloat16)
    delta = sB.double() @ A.double()
    total = W.double() + delta
    out = torch.where(delta == 0, W.double(), T64.rb64(total))
    return out, total, W.double().abs() + sB.double().abs() @ A.double().abs()


def pack(W):
    from bridgelang_amd import ops
    return ops.pack_weight(W.contiguous())


def unpack(p, n, k):
    from bridgelang_amd.weights import _unpack
    return _unpack(p.view(n // 16, k // 32, 64, 8))


def guarded(n, k, dev):
    buf = torch.full((n * k + 2 * GUARD,), NAN_BITS, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return buf, buf[GUARD:GUARD + n * k]


def check_guards(buf, what):
    bits = buf.view(torch.int16)
    assert bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[-GUARD:] == NAN_BITS).all()), f"{what}: guard bytes written"
    assert not bool((bits[GUARD:-GUARD] == NAN_BITS).any()), f"{what}: output elements left unwritten"


def run_one(i, W, A, B, s, dev):
    from bridgelang_amd import train_ops as T
    n, k, R, members, mode = CASES[i][:5]
    buf, out = guarded(n, k, dev)
    T.lora_merge(pack(W), A, B, s, out, R // members, members, mode == "interleave")
    torch.cuda.synchronize()
    check_guards(buf, f"case {i}")
    return out


@pytest.fixture(scope="module")
def dyadic_runs(dev):
    """Every dyadic case once: inputs, the per-group kernel's packed output and the reference — shared, never modified."""
    runs = []
    for i in range(len(CASES)):
        W, A, B = make_case(i, dev, "dyadic")
        runs.append((W, A, B, run_one(i, W, A, B, S, dev), spec(W, A, B, S)[0]))
    return runs


@pytest.mark.parametrize("i", range(len(CASES)))
def test_dyadic_bit_for_bit(dyadic_runs, i):
    n, k = CASES[i][:2]
    W, A, B, out, ref = dyadic_runs[i]
    assert_exact(unpack(out, n, k), ref, f"lora_merge dyadic {CASES[i][:5]}")
    if CASES[i][6] is not None:
        assert bool((unpack(out, n, k)[:, CASES[i][6]:] == 0).all()), "K padding columns must stay 0"
    if i != BIG:                                                   # the package's CPU definition agrees with this file's
        from bridgelang_amd.training.lora import merged_reference
        assert torch.equal(merged_reference(W, A, B, S).view(torch.int16), ref.to(torch.bfloat16).cpu().view(torch.int16))


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 7, 8])
def test_gaussian_bounded(dev, i):
    n, k, R = CASES[i][:3]
    W, A, B = make_case(i, dev, "gauss")
    s = 0.37                                                       # bf16(s·B) rounds: the scaled operand is part of the definition
    got = unpack(run_one(i, W, A, B, s, dev), n, k).double()
    ref, total, mag = spec(W, A, B, s)
    c = R + 1
    near, ulp = T64.near_tie(total, c * T64.E * mag / T64.ulp_bf16(total))
    with T64.on_device():
        T64.assert_bf16_close(got, ref, mag, c, f"lora_merge gauss {CASES[i][:5]}", tie=near.double() * ulp)
    away = ~near
    print(f"lora_merge gauss {CASES[i][:5]}: {int(near.sum())} of {near.numel()} elements near a tie")
    assert bool((got[away] == ref[away]).all()), "an element away from every rounding boundary differs from the definition"


def test_identity_and_absorbed_update(dev):
    i = 3
    n, k, R, members, mode = CASES[i][:5]
    W, A, B = make_case(i, dev, "gauss")
    W.view(-1)[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -120, 3.0, -0.0, 0.0], dtype=torch.bfloat16)
    wbits = pack(W).view(torch.int16).view(-1)
    for what, bb, s in (("scale = 0", B, 0.0), ("B = 0", torch.zeros_like(B), S)):
        out = run_one(i, W, A, bb, s, dev)
        assert torch.equal(out.view(torch.int16), wbits), f"{what}: the merge must copy W bit for bit"
    # an update of 2^-4 ulp of W: W = 1 (ulp 2^-7), Δ = sB·A = 2^-6 · 2^-5 = 2^-11 on every element
    n, k, R = CASES[1][:3]
    W1 = torch.ones(n, k, dtype=torch.bfloat16, device=dev)
    A1 = torch.zeros(R, k, dtype=torch.bfloat16, device=dev)
    B1 = torch.zeros(n, R, dtype=torch.bfloat16, device=dev)
    A1[0], B1[:, 0] = 2.0 ** -5, 2.0 ** -5
    assert float(spec(W1, A1, B1, S)[1].min()) == 1.0 + 2.0 ** -11
    out = run_one(1, W1, A1, B1, S, dev)
    assert torch.equal(out.view(torch.int16), pack(W1).view(torch.int16).view(-1)), "an update below half an ulp is absorbed"


def test_batched_equals_per_group(dyadic_runs, dev):
    from bridgelang_amd import train_ops as T
    bufs, entries = [], []
    for i, (W, A, B, _, _) in enumerate(dyadic_runs):
        n, k, R, members, mode = CASES[i][:5]
        buf, out = guarded(n, k, dev)
        bufs.append((buf, out))
        entries.append(T.be_lora_merge(pack(W), A, B, S, out, R // members, members, mode == "interleave"))
    T.lora_merge_batched(entries, dev, run=True)
    torch.cuda.synchronize()
    for i, (buf, out) in enumerate(bufs):
        check_guards(buf, f"batched case {i}")
        assert torch.equal(out.view(torch.int16), dyadic_runs[i][3].view(torch.int16)), f"batched != per-group launch, case {i}"


def test_argument_errors_without_a_launch(dev):
    from bridgelang_amd import _lib
    lib = _lib.load()
    n, k, R = 32, 64, 64
    w = torch.zeros(n * k + 8, dtype=torch.bfloat16, device=dev)
    A = torch.zeros(R * k, dtype=torch.bfloat16, device=dev)
    B = torch.zeros(n * R, dtype=torch.bfloat16, device=dev)
    buf, out = guarded(n, k, dev)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda wp, op, nn=n, kk=k, rr=R, rp=64, m=1: lib.bl_lora_merge_bf16(wp, A.data_ptr(), B.data_ptr(), C.c_float(S), op, nn, kk,
                                                                                rr, rp, m, 0, st)
    assert call(w.data_ptr(), w.data_ptr()) == _lib.BL_E_ARG                     # in place
    assert call(w.data_ptr(), w.data_ptr() + 64) == _lib.BL_E_ARG                # overlapping
    assert call(None, out.data_ptr()) == _lib.BL_E_ARG
    assert call(w.data_ptr() + 2, out.data_ptr()) == _lib.BL_E_ALIGN
    assert call(w.data_ptr(), out.data_ptr() + 2) == _lib.BL_E_ALIGN
    assert call(w.data_ptr(), out.data_ptr(), nn=24) == _lib.BL_E_SHAPE          # n % 16
    assert call(w.data_ptr(), out.data_ptr(), kk=48) == _lib.BL_E_SHAPE          # k % 32
    assert call(w.data_ptr(), out.data_ptr(), rr=48, rp=48) == _lib.BL_E_SHAPE   # R % 32
    assert call(w.data_ptr(), out.data_ptr(), rr=64, rp=32, m=1) == _lib.BL_E_SHAPE   # R != members·rp
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == NAN_BITS).all()), "a rejected call must not launch"
    assert call(w.data_ptr(), out.data_ptr()) == _lib.BL_OK
    torch.cuda.synchronize()
    check_guards(buf, "accepted call")
