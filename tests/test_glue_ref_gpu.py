"""Every branch of the glue kernels (csrc/glue.hip) and the greedy rows of csrc/sample.hip at its smallest shape, against
the references of tests/glue_ref.py. Every comparison is bit for bit except the cross-entropy values, which are held to
the per-row and mean bounds of tests/train_ref64.py (C_CE_MEAN; glue_ref.mean_c for the masked mean).

Scaffolding (glue_ref.Win / Flat): every buffer a kernel writes is a window of a larger allocation filled with a sentinel
(NaN; a fixed bit pattern for integers). The reference is applied to the CPU copy of the same allocation and the WHOLE
allocation is compared, so a write outside the logical output fails the same comparison as a wrong value. The cos / sin
tables sit between NaN guards too: a read past the table ends in the output. "Second trip": grid_for caps a grid at
2048 x 256 threads; the smallest shape with more work items than that, and a ragged end, runs the grid-stride loop twice.

Branch → case
  rope_kvcache_kernel  one thread per (token, head, 8 rotation pairs). hd 16 (one chunk per half head), 64, 80 (five chunks),
      128; H 1, 32; S 1 (decode form), 37; pos0 0; pos0 + S == cache_len; pos0 + S == the table length; B·S·H·hd/16 =
      524 640 work items (second trip); the first and last token's pairs differ by 2^20 (the fp32 sum is rounded)
      k_cache given: q in place, the k third unchanged, rotated k and v in cache rows [pos0, pos0 + S) only   test_rope_kvcache
      k_cache null (bl_rope_bf16): q and k in place, ld = 3·H·hd + 16, pad columns untouched                test_rope_in_place
  embed_splice_kernel  L 1 with no patches (decode), L 9 with 16 patches (the j == 0 row and the rows behind the patches,
      which keep their sentinel); dim 8, 4096; ids 0, V − 1, repeated; 524 799 work items                   test_embed_splice
  write_prefix_kernel  dim 8; T == n_prefix; T > n_prefix (the other rows untouched); 525 440 work items   test_write_prefix_tokens
  im2col_patch14_kernel  ld 592 (two zeroing stores per row), 640, 1088; chan0 0, 3 (the other tower's channels are NaN);
      B 1, 49 (526 848 work items); the `ci == 0` thread zeroes columns [588, ld)                           test_im2col_patch14
  pack_weight_kernel  (16, 32) one block of 64 lanes, (48, 96), (2064, 2080) second trip; source ld = K + 16;
      kb_off 0 / interior / last of kt_total = K/32 + 5 (the other k-blocks keep their sentinel); unpack_weight inverts it
      test_pack_weight; the launcher's rejections                                                           test_pack_weight_into_rejections
  argmax_kernel  n 4 (one active thread), 1024 (exactly one pass), 1028 (thread 0 alone in the second), 32064; ld = n + 8
      with +inf and NaN in the padding, and ld == n; in-thread loop, the shuffle levels, the four-wave LDS step: ties
      inside a thread, across lanes, across waves, across passes; all equal; all −inf; ±0; +inf; one, several, all NaN
      (argmax_key in bl_common.h)                                                                      test_argmax
  sample_kernel<false|true> step 1 + the greedy exit: the same rows at temperature 0 through ops.sample and ops.score
      (sixteen waves, the s_best / s_arg step)                                                              test_greedy_sample_and_score
  cross_entropy_rows_kernel  n 4, 1024, 1028, 32064; the targets and ±68 logits of ce_case; ignored rows (+0); one valid
      row; all ignored                                                                                      test_cross_entropy_rows
      the target guard: targets −1, n, n + 3 (NaN loss, NaN mean, counted; other rows unaffected)           test_cross_entropy_target_outside
  masked_mean_kernel  rows 1, 255, 256, 257, 1000 at n = 8 (the stride-256 loop and its tail)               test_masked_mean
  bl_argmax_f32 / bl_cross_entropy_f32 reject ld < n                                                         test_row_stride_below_row_rejected

Largest err / bound on MI355X (train_ref64.RATIOS): row loss 0.0080 (1000 rows, n 8), 0.0059 at n 1024, 0.0055 at n 32064;
the mean 0.0055 (256 rows), 0.0036 (one valid row, n 32064). Everything else is bit for bit.
"""
import pytest
import torch

import glue_ref as G
from conftest import rand_bf16
from glue_ref import Flat, Win
from oracle import restate as R
from test_glue_ref_cpu import MEAN_ROWS, ce_rows
from test_train_ref_cpu import ce_case

pytestmark = pytest.mark.gpu
bf16, f32, i32, i64 = torch.bfloat16, torch.float32, torch.int32, torch.int64


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def second_trip(items, whole_blocks=False):
    """More work items than one trip of the capped grid covers, and fewer than two: some threads make a second trip, most
    do not — and, unless the op's item count is a multiple of 256 by construction, the last block is partly idle."""
    assert G.GRID_CAP < items < 2 * G.GRID_CAP and (whole_blocks or items % 256), f"{items} work items are no ragged second trip"


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------
#             B   S     H   hd  pos0 cache_len table
ROPE_CASES = [(1, 1,    1,  16,  0,   1,    1),        # smallest; pos0 0; pos0 + S == cache_len == the table length
              (2, 37,   32, 16,  0,   40,   64),
              (2, 37,   1,  64,  3,   40,   64),       # pos0 + S == cache_len
              (2, 37,   32, 80,  5,   64,   42),       # five chunks per half head; pos0 + S == the table length
              (3, 1,    32, 128, 17,  32,   18),       # the decode form at the table's last position
              (2, 37,   4,  128, 0,   37,   37),
              (1, 3279, 32, 80,  2,   3281, 3281)]     # second trip: 524 640 work items
ROPE_IDS = [f"B{c[0]}-S{c[1]}-H{c[2]}-hd{c[3]}-pos{c[4]}" for c in ROPE_CASES]
_rope_inputs = {}


def _rope_setup(dev, case):
    """Shared, unchanged inputs of the two RoPE tests: qkv on the CPU, the tables on both sides."""
    if case not in _rope_inputs:
        _rope_inputs.clear()                                           # one case at a time: the largest holds 50 MB
        B, S, H, hd, pos0, cache_len, table = case
        cos, sin = R.rope_tables(hd, table, 10000.0)
        _rope_inputs[case] = (G.rope_inputs(B, S, H, hd, 8 + hd), cos, sin)
    qkv, cos, sin = _rope_inputs[case]
    half = case[3] // 2
    C, Sn = Flat((case[6], half), dev, data=cos), Flat((case[6], half), dev, data=sin)      # NaN beyond the last position
    if case[1] > 1000:
        second_trip(case[0] * case[1] * case[2] * (case[3] // 16))
    return qkv, cos, sin, C, Sn


@pytest.mark.parametrize("case", ROPE_CASES, ids=ROPE_IDS)
def test_rope_kvcache(dev, case):
    from bridgelang_amd import ops
    B, S, H, hd, pos0, cache_len, table = case
    qkv, cos, sin, C, Sn = _rope_setup(dev, case)
    Q = Flat((B * S, 3 * H * hd), dev, data=qkv)
    kc, vc = Flat((B, H, cache_len, hd), dev), Flat((B, H, cache_len, hd), dev)
    wq, wk, wv = Q.host(), kc.host(), vc.host()
    ops.rope_kvcache(Q.v, C.v, Sn.v, kc.v, vc.v, B=B, S=S, H=H, head_dim=hd, pos0=pos0)
    torch.cuda.synchronize()
    G.rope_(wq.v, cos, sin, B, S, H, hd, pos0, wk.v, wv.v)
    G.assert_bits(Q, wq, "rope_kvcache qkv (q rotated in place, k and v thirds unchanged)")
    G.assert_bits(kc, wk, "rope_kvcache k cache (rows [pos0, pos0 + S) only)")
    G.assert_bits(vc, wv, "rope_kvcache v cache")
    D = H * hd
    assert torch.equal(G.bits(wq.v[:, D:]), G.bits(qkv[:, D:].to(bf16)))          # the reference itself left k and v alone
    assert bool(wk.v[:, :, :pos0].isnan().all()) and bool(wk.v[:, :, pos0 + S:].isnan().all())


@pytest.mark.parametrize("case", ROPE_CASES, ids=ROPE_IDS)
def test_rope_in_place(dev, case):
    from bridgelang_amd import train_ops as T
    B, S, H, hd, pos0, cache_len, table = case
    qkv, cos, sin, C, Sn = _rope_setup(dev, case)
    Q = Win(B * S, 3 * H * hd, dev, data=qkv)                                      # ld = 3·H·hd + 16
    want = Q.host()
    T.rope(Q.v, C.v, Sn.v, B=B, S=S, H=H, head_dim=hd, pos0=pos0)
    torch.cuda.synchronize()
    G.rope_(want.v, cos, sin, B, S, H, hd, pos0)
    G.assert_bits(Q, want, "rope (q and k rotated in place, v and the pad columns untouched)")


# ---- copies -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,dim,V,npatch", [(1, 1, 8, 4, 0), (3, 1, 4096, 7, 0), (2, 9, 8, 5, 16), (3, 9, 4096, 100, 16),
                                              (3, 341, 4104, 50, 16)],
                         ids=["decode-dim8", "decode-dim4096", "patches-dim8", "patches-dim4096", "second-trip"])
def test_embed_splice(dev, B, L, dim, V, npatch):
    from bridgelang_amd import ops
    if L > 100:
        second_trip(B * L * dim // 8)
    g = torch.Generator().manual_seed(L + dim)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[0, 0], ids[-1, -1] = 0, V - 1
    if L > 2:
        ids[0, 1] = ids[0, 2] = V - 1                                               # a repeated id, next to each other
    assert bool((ids >= 0).all()) and bool((ids < V).all())
    table = rand_bf16((V, dim), 1).to(bf16)
    dst = Flat((B, L + npatch, dim), dev)
    want = dst.host()
    ops.embed_splice(ids.to(dev), table.to(dev), dst.v, npatch)
    torch.cuda.synchronize()
    G.embed_splice_(ids, table, want.v, npatch)
    G.assert_bits(dst, want, "embed_splice (the patch rows keep their sentinel)")
    assert npatch == 0 or bool(want.v[:, 1:1 + npatch].isnan().all())


@pytest.mark.parametrize("n_prefix,dim,B,T", [(1, 8, 1, 1), (5, 8, 3, 5), (5, 64, 3, 21), (5, 1024, 821, 6)],
                         ids=["smallest", "T==n_prefix", "T>n_prefix", "second-trip"])
def test_write_prefix_tokens(dev, n_prefix, dim, B, T):
    from bridgelang_amd import ops
    if B > 100:
        second_trip(B * n_prefix * dim // 8)
    pre = rand_bf16((n_prefix, dim), 4).to(bf16)
    x = Flat((B * T, dim), dev)
    want = x.host()
    ops.write_prefix_tokens(pre.to(dev), x.v, B, T)
    torch.cuda.synchronize()
    G.write_prefix_(pre, want.v, B, T)
    G.assert_bits(x, want, "write_prefix_tokens (rows [n_prefix, T) untouched)")


@pytest.mark.parametrize("B,ld,chan0", [(1, 592, 0), (1, 592, 3), (1, 640, 0), (1, 640, 3), (1, 1088, 0), (1, 1088, 3), (49, 592, 3)])
def test_im2col_patch14(dev, B, ld, chan0):
    from bridgelang_amd import ops
    if B > 1:
        second_trip(B * 256 * 42, whole_blocks=True)                               # 42 · 256 items per image
    pv = rand_bf16((B, 6, 224, 224), 3 + B)
    pv[:, 3 - chan0:6 - chan0] = G.NAN                                             # the other tower's channels: never read
    pv = pv.to(bf16)
    out = Flat((B * 256, ld), dev)
    want = out.host()
    ops.im2col_patch14(pv.to(dev), chan0, out.v)
    torch.cuda.synchronize()
    G.im2col_(pv, chan0, want.v)
    G.assert_bits(out, want, "im2col_patch14 (pad columns exactly zero)")
    assert bool((G.bits(want.v[:, 588:]) == 0).all()) and bool(torch.isfinite(want.v.float()).all())


# ---- weight packing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(16, 32), (48, 96), (2064, 2080)], ids=["one-block", "3x3-blocks", "second-trip"])
def test_pack_weight(dev, N, K):
    from bridgelang_amd import ops, train_ops as T
    if N > 1000:
        second_trip(N * K // 8)
    w = rand_bf16((N, K), N + K).to(bf16)
    W = Win(N, K, dev, data=w)                                                      # source ld = K + 16 > K
    dst = Flat((N // 16, K // 32, 64, 8), dev)
    want = dst.host()
    ops.pack_weight(W.v, out=dst.v)
    torch.cuda.synchronize()
    G.pack_into_(w, want.v)
    G.assert_bits(dst, want, "pack_weight")
    assert torch.equal(G.bits(ops.unpack_weight(dst.v).cpu()), G.bits(w))           # the round trip is the identity
    kt_total = K // 32 + 5
    for kb in (0, 2, 5):                                                            # first, interior, last
        assert kb + K // 32 <= kt_total
        dst = Flat((N // 16, kt_total, 64, 8), dev)
        want = dst.host()
        T.pack_into(W.v, dst.v, kt_total, kb)
        torch.cuda.synchronize()
        G.pack_into_(w, want.v, kb)
        G.assert_bits(dst, want, f"pack_weight_into k-block {kb} of {kt_total} (the other k-blocks keep their sentinel)")
        assert torch.equal(G.bits(ops.unpack_weight(dst.v)[:, 32 * kb:32 * kb + K].cpu()), G.bits(w))
    G.assert_bits(W, Win(N, K, "cpu", data=w), "pack_weight source")


def test_pack_weight_into_rejections(dev):
    from bridgelang_amd import _lib
    fn = _lib.load().bl_pack_weight_into_bf16
    N, K, kt_total = 32, 64, 4
    W = Win(N, K, dev, data=rand_bf16((N, K), 1))
    ld = W.v.stride(0)
    dst = Flat((N // 16, kt_total, 64, 8), dev)
    src, out, st = W.v.data_ptr(), dst.v.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert ld == K + 16 and src % 16 == 0 and out % 16 == 0
    shape = [(src, ld, 0, K, out, kt_total, 0), (src, ld, N, 0, out, kt_total, 0), (src, ld, 24, K, out, kt_total, 0),
             (src, ld, N, 48, out, kt_total, 0), (src, K - 8, N, K, out, kt_total, 0), (src, ld + 4, N, K, out, kt_total, 0),
             (src, ld, N, K, out, kt_total, -1), (src, ld, N, K, out, kt_total, kt_total - 1), (src, ld, N, K, out, 1, 0)]
    for a in shape:
        assert fn(*a, st) == _lib.BL_E_SHAPE, f"bl_pack_weight_into_bf16{a[1:4] + a[5:]} must be rejected as a shape error"
    assert fn(src + 2, ld, N, K, out, kt_total, 0, st) == _lib.BL_E_ALIGN
    assert fn(src, ld, N, K, out + 2, kt_total, 0, st) == _lib.BL_E_ALIGN
    assert fn(None, ld, N, K, out, kt_total, 0, st) == _lib.BL_E_ARG and fn(src, ld, N, K, None, kt_total, 0, st) == _lib.BL_E_ARG
    torch.cuda.synchronize()
    assert bool(dst.buf.isnan().all()), "a rejected call wrote something"
    assert fn(src, ld, N, K, out, kt_total, kt_total - K // 32, st) == _lib.BL_OK     # and the last legal offset is accepted
    torch.cuda.synchronize()
    want = Flat((N // 16, kt_total, 64, 8), "cpu")
    G.pack_into_(W.v.cpu(), want.v, kt_total - K // 32)
    G.assert_bits(dst, want, "pack_weight_into at the last legal offset")


# ---- argmax and the greedy rows ---------------------------------------------------------------------------------------------------
ARGMAX_N = [4, 1024, 1028, 32064]
_argmax_rows = {}


def _argmax_case(n):
    """Shared, unchanged: the rows at width n in a row stride of n + 8 (+inf and NaN in the padding)."""
    if n not in _argmax_rows:
        _argmax_rows[n] = G.argmax_rows(n, n + 8)
    return _argmax_rows[n]


@pytest.mark.parametrize("n", ARGMAX_N)
def test_argmax(dev, n):
    from bridgelang_amd import ops
    lg, names = _argmax_case(n)
    rows = len(names)
    want = Flat((rows,), "cpu", i64, data=torch.argmax(lg[:, :n], -1))
    L = lg.to(dev)
    for what, view in (("ld = n + 8", L[:, :n]), ("ld == n", L[:, :n].contiguous())):
        out = Flat((rows,), dev, i64)
        ops.argmax(view, out.v)
        torch.cuda.synchronize()
        G.check_argmax(out.v, lg, n, f"argmax n {n} {what}", names)
        G.assert_bits(out, want, f"argmax n {n} {what}")


@pytest.mark.parametrize("n", ARGMAX_N)
def test_greedy_sample_and_score(dev, n):
    """Temperature 0 through the sampler and the scorer: the id, the (1, 1) pair, the score of the argmax (1, 1) and of its
    neighbour (0, 1), and the one-hot over the whole row equal torch.argmax of the same rows. Nothing here is fed on."""
    from bridgelang_amd import ops
    lg, names = _argmax_case(n)
    rows = len(names)
    am = torch.argmax(lg[:, :n], -1)
    L = lg.to(dev)[:, :n]
    temp, top_k, top_p = torch.zeros(rows, device=dev), torch.zeros(rows, dtype=i32, device=dev), torch.ones(rows, device=dev)
    seed = torch.arange(rows, dtype=i64, device=dev)
    ids, wt = Flat((rows,), dev, i64), Flat((rows, 2), dev, i64)
    ops.sample(L, temp, top_k, top_p, seed, 3, ids.v, wt.v)
    torch.cuda.synchronize()
    G.check_argmax(ids.v, lg, n, f"greedy sample n {n}", names)
    G.assert_bits(ids, Flat((rows,), "cpu", i64, data=am), f"greedy sample ids n {n}")
    G.assert_bits(wt, Flat((rows, 2), "cpu", i64, data=torch.ones(rows, 2, dtype=i64)), f"greedy sample weights n {n}")
    for tokens, hit in ((am, 1), ((am + 1) % n, 0)):
        wt, rw = Flat((rows, 2), dev, i64), Flat((rows, n), dev, i32)
        ops.score(L, temp, top_k, top_p, tokens.to(dev), wt.v, 0, rw.v)
        torch.cuda.synchronize()
        pair = torch.tensor([hit, 1], dtype=i64).expand(rows, 2)
        G.assert_bits(wt, Flat((rows, 2), "cpu", i64, data=pair), f"greedy score n {n} of the argmax{'' if hit else ' + 1'}")
        onehot = torch.nn.functional.one_hot(am, n).to(i32)
        G.assert_bits(rw, Flat((rows, n), "cpu", i32, data=onehot), f"greedy score one-hot n {n}")


# ---- cross-entropy ----------------------------------------------------------------------------------------------------------------
def _run_ce(dev, logits, targets, pad_fill=None):
    """One launch on a logits window (8 pad columns on each side and a guard row above and below, all inside one allocation);
    returns (row_loss, mean_and_count) on the CPU after the sentinel checks."""
    from bridgelang_amd import ops
    rows, n = logits.shape
    L = Win(rows, n, dev, f32, data=logits, fill=pad_fill)
    before = L.host()
    rl, mc = Flat((rows,), dev, f32), Flat((2,), dev, f32)
    ops.cross_entropy(L.v, targets.to(dev), rl.v, mc.v)
    torch.cuda.synchronize()
    G.outside_untouched(rl, "cross_entropy row_loss")
    G.outside_untouched(mc, "cross_entropy mean_and_count")
    G.assert_bits(L, before, "cross_entropy logits")
    return rl.v.cpu(), mc.v.cpu()


@pytest.mark.parametrize("n", [4, 1024, 1028, 32064])
def test_cross_entropy_rows(dev, n):
    rows = 12
    logits, tgt = ce_case(rows, n)
    one = torch.full((rows,), -100, dtype=i64)
    one[7] = tgt[7]
    none = torch.full((rows,), -100, dtype=i64)
    for what, targets in (("ce_case", tgt), ("one valid row", one), ("all ignored", none)):
        rl, mc = _run_ce(dev, logits, targets)
        G.check_cross_entropy(f"gpu ce n {n} {what}", rl, mc, logits, targets)


@pytest.mark.parametrize("rows", MEAN_ROWS)
def test_masked_mean(dev, rows):
    logits, tgt = ce_rows(rows, 8)
    rl, mc = _run_ce(dev, logits, tgt)
    G.check_cross_entropy(f"gpu masked mean {rows} rows", rl, mc, logits, tgt)


@pytest.mark.parametrize("n", [4, 1028])
def test_cross_entropy_target_outside(dev, n):
    """Targets −1, n and n + 3, one per launch and all three together: with 8 pad columns on each side of the window even a
    kernel without the guard reads inside the allocation. The pad holds 1.5 here, not NaN, so that such a kernel returns a
    finite, wrong loss, which fails here (from a NaN pad it would return the NaN the rule asks for)."""
    rows = 12
    logits, tgt = ce_case(rows, n)
    cases = [{4: -1}, {4: n}, {4: n + 3}, {1: -1, 7: n, 11: n + 3}]
    for c in cases:
        out = tgt.clone()
        for r, t in c.items():
            assert out[r] != -100
            out[r] = t
        rl, mc = _run_ce(dev, logits, out, pad_fill=1.5)
        G.check_cross_entropy_outside(f"gpu ce n {n} targets {sorted(c.values())}", rl, mc, logits, out)


def test_row_stride_below_row_rejected(dev):
    """ld < n: rows would overlap. The strided view stays inside one allocation."""
    from bridgelang_amd import ops
    from bridgelang_amd._lib import BridgeLangHipError
    n = 16
    base = torch.zeros(3 * n, device=dev)
    lg = base.as_strided((2, n), (n - 4, 1))
    out = Flat((2,), dev, i64)
    with pytest.raises(BridgeLangHipError):
        ops.argmax(lg, out.v)
    rl, mc = Flat((2,), dev, f32), Flat((2,), dev, f32)
    with pytest.raises(BridgeLangHipError):
        ops.cross_entropy(lg, torch.zeros(2, dtype=i64, device=dev), rl.v, mc.v)
    torch.cuda.synchronize()
    for x in (out, rl, mc):
        assert bool((G.bits(x.buf.cpu()) == G.bits(type(x)(x.shape, "cpu", x.buf.dtype).buf)).all()), "a rejected call wrote something"
    ok = base.as_strided((2, n), (n, 1))                                            # ld == n is the smallest legal stride
    ops.argmax(ok, out.v)
    torch.cuda.synchronize()
    assert out.v.tolist() == [0, 0]

