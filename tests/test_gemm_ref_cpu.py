"""The fp64 GEMM reference and its checks (tests/gemm_ref64.py) tell right from wrong, on the CPU.

* The dyadic exactness condition holds for every (K, value set) of tests/test_gemm_ref_gpu.py (the case tables live here
  and the GPU module imports them), and the generators produce what the condition assumes.
* An fp32 torch restatement with the kernels' roundings (fp32 accumulation, `.bfloat16()` where gemm_common.h rounds,
  silu / erf-GELU and their derivatives in fp32) passes every check: bit for bit where the reference claims exactness.
* Wrong algorithms, computed in fp64 so that only the algorithm is wrong, are all rejected. Which of them the older
  yardstick (close_bf16 of tests/test_ops_gpu.py: 2^-6·|ref| + 2^-8·max|ref| and 98 % of the elements equal) would accept
  is recorded in CLOSE_BF16_ACCEPTS / CLOSE_BF16_TOLERANCE_ACCEPTS and asserted, so the record cannot go stale.
"""
import math

import pytest
import torch

import gemm_ref64 as G
import train_ref64 as T64
from gemm_ref64 import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_KEEP, EPI_BIAS_RES, EPI_F32, EPI_F32_BF16R, EPI_GELU_BWD, EPI_NONE,
                        EPI_RES, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_SWIGLU_KEEP)

f32 = torch.float32

# ---- the GPU module's cases: form → (M, N, K, workspace) --------------------------------------------------------------------
# What the planner (csrc/gemm_plan.h) gives these shapes: tests/test_gemm_plan_cpu.py checks every entry against it without a
# GPU, and every case asserts the form it names through ops.gemm_last_form().
TILE_CASES = [
    ("gemm128", 700, 272, 448, False),
    ("gemm128", 1, 16, 64, False),
    ("gemm128", 32, 272, 448, False),
    ("mid<2,1>", 33, 80, 512, False),
    ("mid<2,4>", 120, 10192, 576, False),
    ("mid<4,1>", 130, 528, 576, False),
    ("mid<5,1>", 270, 528, 576, False),
    ("mid<4,4>", 130, 10192, 576, False),
    ("mid<2,4>/S8", 100, 1040, 4160, True),
    ("mid<4,4>/S2", 200, 1040, 1088, True),
    ("mid<5,4>/S4", 300, 144, 2112, True),
    ("mid2<1>", 330, 544, 576, False),
    ("mid2<2,2>", 630, 10208, 576, False),
    ("mid2<4>", 170, 25632, 512, False),
    ("ring160x128", 2081, 1936, 512, False),
    ("ring128x128/S8", 1000, 80, 4160, True),
    ("gemm288s", 2290, 7408, 512, False),
    ("gemm256s", 4100, 2064, 512, False),
    ("gemm256s_persistent", 2100, 9264, 512, False),
    ("gemm256s", 2100, 9264, 576, False),
    ("gemm256s+tail64x64", 4100, 4000, 576, False),
    ("gemm256s+tail128x64", 3900, 4368, 576, False),
    ("gemm256s+tail128x128", 4353, 4112, 576, False),
    ("gemm256s+splitk2", 2000, 4000, 8256, True),
    # whole rounds on the persistent walk (more than 512 tiles, an even K-tile count), then the leftover tiles
    ("gemm256s_persistent+tail64x64", 1159, 26256, 640, False),       # 5 x 103 tiles: 3 left over
    ("gemm256s_persistent+tail128x64", 1159, 26928, 640, False),      # 5 x 106: 18
    ("gemm256s_persistent+tail128x128", 1159, 27824, 640, False),     # 5 x 109: 33
    ("gemm256s_persistent+splitk16", 321, 65744, 8320, True),         # 2 x 257: 2; K >= 8192 and 513 tiles: no smaller shape gets here
]
SKINNY_K = (512, 1024, 1536, 4096, 5120, 11008, 13824)
SKINNY_KS = {512: 2, 1024: 4, 1536: 6, 4096: 16, 5120: 20, 11008: 43, 13824: 54}
SKINNY_M = (1, 5, 16)
SKINNY_N = (4112, 16)
# bl_gemm_skinny_rows_bf16: form → (N, K, workspace, row counts)
ROWS_CASES = [
    ("rows_stream<8,8>", 25504, 1024, False, (1, 17, 96)),
    ("rows_stream<6,8>", 4112, 1024, False, (1, 17, 96)),
    ("rows_stream<8,4>+tree", 4112, 1024, True, (1, 17, 96)),
    ("rows_mid<SK=8>", 528, 1536, False, (1, 17, 96, 128)),
    ("rows_mid<SK=8>", 4112, 1024, False, (128,)),
    ("rows_mid<SK=2>+tree", 528, 512, True, (1, 17, 96, 128)),
]
# bl_gemm_tn_bf16: form → (token rows T, M, N, workspace); M, N multiples of 8 but not of 256
TN_CASES = [
    ("tn", 33, 264, 520, False),                   # one K-tile (odd), T % 64 != 0
    ("tn", 1000, 264, 520, False),                 # 16 K-tiles (even)
    ("tn", 33, 4104, 3848, False),                 # 272 tiles, odd K-tile count: not persistent
    ("tn_persistent", 1000, 4104, 3848, False),    # 272 tiles, even K-tile count
    ("tn_all_split+splitk4", 1000, 264, 520, True),
    ("tn+splitk16", 8200, 4104, 3848, True),       # 16 leftover tiles in 16 slices, 129 K-tiles
]
NORM_DIMS = (8, 520, 1024, 1536, 2048, 2560, 3072, 3584, 4096, 4608, 5120)
NORM_ROWS = (1, 4, 5, 261)


def all_gpu_k():
    ks = {K for _, _, _, K, _ in TILE_CASES} | set(SKINNY_K) | {K for _, _, K, _, _ in ROWS_CASES}
    return sorted(ks | {T for _, T, _, _, _ in TN_CASES})


# ---- the instrument's premises -------------------------------------------------------------------------------------------------
def test_dyadic_condition_holds_for_every_gpu_case():
    for K in all_gpu_k():
        G.assert_dyadic_exact(K)
    G.assert_dyadic_exact(65536, addmax=0.0)                 # the product alone is exact up to K = 65 536
    with pytest.raises(AssertionError):
        G.assert_dyadic_exact(65536)                         # but not with the first epilogue add
    with pytest.raises(AssertionError):
        G.assert_dyadic_exact(4096, amax=4.0, wmax=8.0)
    with pytest.raises(AssertionError):
        G.assert_dyadic_exact(1024, fa=8, fw=8)


def test_generators_produce_the_value_sets():
    a, w, b = G.dyadic_a((64, 512), 1), G.dyadic_w((80, 512), 2), G.dyadic_add((64, 80), 3)
    G.check_dyadic_values(a, G.A_FRAC, 2.0)
    G.check_dyadic_values(w, G.W_FRAC, 1.0)
    G.check_dyadic_values(b, G.ADD_FRAC, G.ADD_MAX)
    assert a.abs().max() == 2.0 and w.abs().max() == 1.0 and b.abs().max() == 4.0 and len(a.unique()) == 33
    for t in (a, w, b, G.layerscale(80, 4), G.gauss((8, 8), 5)):
        assert torch.equal(t, t.to(torch.bfloat16).float())          # bf16 values
    assert torch.equal(a, G.dyadic_a((64, 512), 1))                  # seeded
    # every partial sum in any order is exact in fp32: a shuffled fp32 accumulation equals the fp64 product
    K = 13824
    a, w = G.dyadic_a((3, K), 6), G.dyadic_w((5, K), 7)
    x = G.product(a, w)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(8))
    acc = torch.zeros(3, 5, dtype=f32)
    for k0 in range(0, K, 864):
        idx = perm[k0:k0 + 864]
        acc = acc + (a[:, idx] @ w[:, idx].t())
    assert torch.equal(acc.double(), x)


# ---- an fp32 restatement with the kernels' roundings ---------------------------------------------------------------------------
def rbf(t):
    return t.to(torch.bfloat16).to(f32)


def _erf_gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t * (1.0 / math.sqrt(2.0))))


def restate_fp32(epi, A, W, bias=None, scale=None, res=None, res_row_mod=0):
    """gemm_common.h's epilogue_store4 statement by statement in fp32 torch. Returns (C, C2)."""
    acc = A.to(f32) @ W.to(f32).t()
    M, N = acc.shape
    if epi == EPI_F32:
        return acc, None
    if epi in (EPI_F32_BF16R, EPI_NONE):
        return rbf(acc), None
    if epi in (EPI_SWIGLU, EPI_SWIGLU_KEEP):
        t = rbf(acc)
        g, u = t[:, 0::2], t[:, 1::2]
        act = rbf(rbf(g * torch.sigmoid(g)) * u)
        return (act, None) if epi == EPI_SWIGLU else (t, act)
    if epi == EPI_SWIGLU_BWD:
        d, gu = rbf(acc), res[:M, :2 * N].to(f32)
        g, u = gu[:, 0::2], gu[:, 1::2]
        sg = torch.sigmoid(g)
        out = torch.empty(M, 2 * N)
        out[:, 0::2], out[:, 1::2] = d * u * (sg * (1.0 + g * (1.0 - sg))), d * rbf(g * sg)
        return rbf(out), None
    if epi == EPI_GELU_BWD:
        t = res[:M, :N].to(f32)
        grad = 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
        return rbf(rbf(acc) * grad), None
    v = acc + bias if epi in G.HAS_BIAS else acc
    if epi == EPI_BIAS:
        return rbf(v), None
    if epi == EPI_BIAS_GELU:
        return rbf(_erf_gelu(rbf(v))), None
    if epi == EPI_BIAS_GELU_KEEP:
        return rbf(v), rbf(_erf_gelu(rbf(v)))
    v = rbf(v)
    if scale is not None:
        v = rbf(v * scale)
    rows = torch.arange(M) % res_row_mod if res_row_mod else torch.arange(M)
    return rbf(v + res[rows][:, :N]), None


def _case(M=45, N=96, K=128, seed=10, mod=0):
    A, W = G.dyadic_a((M, K), seed), G.dyadic_w((N, K), seed + 1)
    return dict(A=A, W=W, x=G.product(A, W), bias=G.dyadic_add((N,), seed + 2), ls=G.layerscale(N, seed + 3),
                res=G.dyadic_add((mod or M, N), seed + 4), gu=G.dyadic_add((M, 2 * N), seed + 5), mod=mod)


@pytest.mark.parametrize("M,N,K,mod", [(45, 96, 128, 0), (33, 64, 4160, 7), (5, 32, 13824, 0)])
def test_reference_agrees_with_fp32_restatement(M, N, K, mod):
    c = _case(M, N, K, mod=mod)
    G.assert_dyadic_exact(K)
    for epi in range(12):
        for scale in ((None, c["ls"]) if epi == EPI_BIAS_RES else (None,)):
            res = c["gu"] if epi == EPI_SWIGLU_BWD else G.dyadic_add((M, N), 99) if epi == EPI_GELU_BWD else c["res"]
            rrm = mod if epi in G.HAS_RES else 0
            C, C2 = restate_fp32(epi, c["A"], c["W"], c["bias"], scale, res, rrm)
            G.check_epilogue(f"cpu fp32 restatement {G.EPI_NAMES[epi]}{' ls' if scale is not None else ''}", epi, c["x"], C, C2,
                             bias=c["bias"], scale=scale, res=res, res_row_mod=rrm)


def test_gauss_bound_accepts_fp32_and_rejects_lost_mantissa_bits():
    M, N, K = 40, 48, 576
    A, W = G.gauss((M, K), 20), G.gauss((N, K), 21)
    bias, res = G.gauss((N,), 22), G.gauss((M, N), 23)
    acc = A @ W.t()
    G.check_gauss("cpu gauss f32", EPI_F32, A, W, acc)
    G.check_gauss("cpu gauss bias_res", EPI_BIAS_RES, A, W, rbf(rbf(acc + bias) + res), bias=bias, res=res)
    # a fragment path that drops the operands' lowest mantissa bit
    trunc = lambda t: (t.view(torch.int32) & ~0x10000).view(f32)
    with pytest.raises(AssertionError):
        G.check_gauss("cpu gauss f32, low bit lost", EPI_F32, A, W, trunc(A.clone()) @ trunc(W.clone()).t())


def test_norm_references_accept_fp32_restatements():
    eps = 1e-6
    x, w, b = G.gauss((9, 520), 30, 2.0), (G.gauss((520,), 31, 0.02) + 1).to(torch.bfloat16).float(), G.gauss((520,), 32, 0.1)
    x[3] = (x[3] * 0.25 + 16.0).to(torch.bfloat16).float()           # mean >> spread (2^5)
    x[4] = 1.5                                                       # a constant row
    rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    G.check_rmsnorm("cpu rmsnorm fp32", rbf(w * rbf(x * rstd)), x, w, eps)
    mu = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    G.check_layernorm("cpu layernorm fp32", rbf((x - mu) * rs * w + b), x, w, b, eps)
    with pytest.raises(AssertionError):                              # HF's inner rounding skipped
        G.check_rmsnorm("cpu rmsnorm, one rounding", rbf(w * (x * rstd)), x, w, eps)
    with pytest.raises(AssertionError):                              # the mean rounded to bf16: fatal on the offset row
        mub = rbf(mu)
        G.check_layernorm("cpu layernorm, bf16 mean", rbf((x - mub) * rs * w + b), x, w, b, eps)


# ---- wrong algorithms ------------------------------------------------------------------------------------------------------------
def _wrong_algorithms():
    """name → (epilogue, kwargs of check_epilogue, the wrong output in fp64, the right output). M = 45: a ragged last 16-row tile."""
    c = _case(45, 96, 128, seed=40, mod=7)
    A, W, x, b, ls = c["A"].double(), c["W"].double(), c["x"], c["bias"].double(), c["ls"].double()
    res7, M = c["res"], 45
    resM = G.dyadic_add((M, 96), 48)
    rb = T64.rb64
    step = A[:, 32:64] @ W[:, 32:64].t()
    out = {}
    out["one 32-wide k-step dropped"] = (EPI_NONE, {}, rb(x - step))
    out["one k-step added twice"] = (EPI_NONE, {}, rb(x + step))
    sw = rb(x).clone()
    sw[:, 16:32], sw[:, 32:48] = rb(x)[:, 32:48], rb(x)[:, 16:32]
    out["two 16-column tiles swapped"] = (EPI_NONE, {}, sw)
    un = rb(x).clone()
    un[32:] = float("nan")
    out["last ragged row tile left unwritten"] = (EPI_NONE, {}, un)
    out["bias taken from column n + 4"] = (EPI_BIAS, dict(bias=c["bias"]), rb(x + torch.roll(b, -4)))
    tall = torch.cat([res7, G.dyadic_add((M - 7, 96), 49)])          # what lies behind the 7-row table
    out["residual row not wrapped under res_row_mod"] = (EPI_RES, dict(res=res7, res_row_mod=7), rb(rb(x) + tall.double()))
    t = rb(x[:, :96])
    g, u = t[:, 0::2], t[:, 1::2]
    out["gate/up swapped in SwiGLU"] = (EPI_SWIGLU, {}, rb(rb(u * torch.sigmoid(u)) * g))
    out["bf16(acc) skipped before the residual add"] = (EPI_RES, dict(res=resM), rb(x + resM.double()))
    out["LayerScale applied after the residual"] = (EPI_BIAS_RES, dict(bias=c["bias"], scale=c["ls"], res=resM),
                                                    rb((rb(x + b) + resM.double()) * ls))
    out["fp32 output rounded to bf16 under EPI_F32"] = (EPI_F32, {}, rb(x))
    return x, out


# close_bf16 (tests/test_ops_gpu.py) on this case, all 4320 elements compared: its tolerance clause alone accepts these —
# an error of one bf16 ulp, or a value moved by less than 2^-8·max|ref|, is invisible to it — and only its 98 %-equal
# clause rejects them; that clause in turn passes any defect confined to 2 % of the elements it samples.
CLOSE_BF16_TOLERANCE_ACCEPTS = {"bf16(acc) skipped before the residual add", "fp32 output rounded to bf16 under EPI_F32"}
CLOSE_BF16_ACCEPTS = set()


def test_wrong_algorithms_are_rejected():
    x, wrong = _wrong_algorithms()
    assert len(wrong) == 10
    accepted, tol_accepted = set(), set()
    for name, (epi, kw, got) in wrong.items():
        with pytest.raises(AssertionError):
            G.check_epilogue(f"cpu wrong: {name}", epi, x, got, **kw)
        if epi == EPI_SWIGLU:
            right = T64.rb64(T64.swiglu_forward(T64.rb64(x))["act"])
        else:
            right = G.linear_ref(epi, x, kw.get("bias"), kw.get("scale"), kw.get("res"), kw.get("res_row_mod", 0))
        finite = bool(torch.isfinite(got).all())
        tol_ok = finite and G.close_bf16_accepts(got, right, min_exact=0.0)
        ok = finite and G.close_bf16_accepts(got, right)
        print(f"close_bf16 {'ACCEPTS' if ok else 'rejects'} (tolerance clause alone {'accepts' if tol_ok else 'rejects'}; "
              f"{float((got == right).double().mean()):.3f} equal): {name}")
        accepted |= {name} if ok else set()
        tol_accepted |= {name} if tol_ok else set()
    assert accepted == CLOSE_BF16_ACCEPTS, accepted ^ CLOSE_BF16_ACCEPTS
    assert tol_accepted == CLOSE_BF16_TOLERANCE_ACCEPTS, tol_accepted ^ CLOSE_BF16_TOLERANCE_ACCEPTS


def test_right_algorithms_pass_on_the_wrong_algorithms_case():
    """The same case, computed right, passes every check the wrong ones fail (the rejections are not the checks' own noise)."""
    x, wrong = _wrong_algorithms()
    for name, (epi, kw, _) in wrong.items():
        if epi == EPI_SWIGLU:
            got = T64.rb64(T64.swiglu_forward(T64.rb64(x))["act"])
        else:
            got = G.linear_ref(epi, x, kw.get("bias"), kw.get("scale"), kw.get("res"), kw.get("res_row_mod", 0))
        G.check_epilogue(f"cpu right: {name}", epi, x, got, **kw)


def test_row_maps():
    kept, rows = G.out_rows(120, (50, 52, 4), "cpu")
    assert kept.numel() == 120 - 2 * 2 - 0 and int(rows.max()) == 2 * 52 + 19 + 4      # rows 48, 49 of each full group are dropped
    assert set(range(50)) - set(kept.tolist()) == {48, 49}
    assert G.res_rows(10, 4, "cpu").tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    kept, rows = G.out_rows(5, None, "cpu")
    assert torch.equal(kept, rows)
