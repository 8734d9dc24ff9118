"""The glue-kernel references and comparators (tests/glue_ref.py) tell right from wrong, on the CPU.

Each reference is checked against an independent formulation of the same operation — transformers' apply_rotary_pos_emb on
bf16 tensors, F.unfold, F.cross_entropy(reduction="none"), a plain loop for the packing formula and for the argmax
order — and each comparison is shown to reject a planted near-miss: the rotation halves swapped, the position off by one,
the k third rotated in place although a cache is given, a row written one slot late, ties resolved to the last index, NaN
never winning (the argmax order before bl_common.h::argmax_key), the pad columns of im2col left unzeroed, a k-block one
slot off, a cross-entropy target read one column off or outside the row.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import glue_ref as G
import train_ref64 as T64
from conftest import rand_bf16
from oracle import restate as R
from test_train_ref_cpu import ce_case

bf16, f32 = torch.bfloat16, torch.float32
CPU = "cpu"


def rejected(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------
def _hf_rope(x, cos, sin, pos0):
    """transformers' Llama apply_rotary_pos_emb on bf16 tensors ([B, H, S, hd], cos / sin = cat(freqs, freqs)); its literal
    formula where the installed transformers does not have the function under this name."""
    S = x.shape[2]
    c = torch.cat([cos, cos], -1)[pos0:pos0 + S].to(bf16)[None]                  # [1, S, hd]
    s = torch.cat([sin, sin], -1)[pos0:pos0 + S].to(bf16)[None]
    xb = x.to(bf16)
    try:
        from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
        return apply_rotary_pos_emb(xb, xb, c, s)[0].float()
    except ImportError:
        half = x.shape[-1] // 2
        rot = torch.cat((-xb[..., half:], xb[..., :half]), dim=-1)
        return ((xb * c[:, None]) + (rot * s[:, None])).float()


def _rope_case(hd, B=2, S=5, H=3, pos0=2, cache_len=9, table=16):
    cos, sin = R.rope_tables(hd, table, 10000.0)
    qkv = G.rope_inputs(B, S, H, hd, 11)
    Q = G.Win(B * S, 3 * H * hd, CPU, data=qkv)
    kc, vc = G.Flat((B, H, cache_len, hd), CPU), G.Flat((B, H, cache_len, hd), CPU)
    return B, S, H, hd, pos0, cos, sin, qkv, Q, kc, vc


@pytest.mark.parametrize("hd", [16, 64, 80, 128])
def test_rope_reference_is_hf_in_bf16(hd):
    B, S, H, hd, pos0, cos, sin, qkv, Q, kc, vc = _rope_case(hd)
    D = H * hd
    t = qkv.view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)                            # [3, B, H, S, hd]
    back = lambda x: x.permute(0, 2, 1, 3).reshape(B * S, D)
    q_hf, k_hf = _hf_rope(t[0], cos, sin, pos0), _hf_rope(t[1], cos, sin, pos0)
    # the 2^20 rows really make the fp32 sum inexact: the exact sum of the two rounded products needs more than 24 bits somewhere
    half = hd // 2
    a = (t[0][..., :half] * cos[pos0:pos0 + S]).to(bf16).double() + (-t[0][..., half:] * sin[pos0:pos0 + S]).to(bf16).double()
    assert bool((a != a.float().double()).any()), "no pair whose fp32 sum is rounded: the 2^20 rows do not exercise it"
    # without a cache: q and k rotated in place, v and the pad columns untouched
    W = Q.host()
    G.rope_(W.v, cos, sin, B, S, H, hd, pos0)
    assert torch.equal(W.v[:, :D].float(), back(q_hf)) and torch.equal(W.v[:, D:2 * D].float(), back(k_hf))
    want = Q.host()
    want.v[:, :2 * D] = torch.cat([back(q_hf), back(k_hf)], 1).to(bf16)
    G.assert_bits(W, want, "rope without a cache")
    # with caches: k third unchanged, rotated k and v in cache rows [pos0, pos0 + S) only
    W, K, V = Q.host(), kc.host(), vc.host()
    G.rope_(W.v, cos, sin, B, S, H, hd, pos0, K.v, V.v)
    wq, wk, wv = Q.host(), kc.host(), vc.host()
    wq.v[:, :D] = back(q_hf).to(bf16)
    wk.v[:, :, pos0:pos0 + S] = k_hf.to(bf16)
    wv.v[:, :, pos0:pos0 + S] = t[2].to(bf16)
    for got, exp, name in ((W, wq, "qkv"), (K, wk, "k cache"), (V, wv, "v cache")):
        G.assert_bits(got, exp, f"rope with caches: {name}")


def test_rope_near_misses_rejected():
    B, S, H, hd, pos0, cos, sin, qkv, Q, kc, vc = _rope_case(80)
    half = hd // 2

    def run(**kw):
        W, K, V = Q.host(), kc.host(), vc.host()
        G.rope_(W.v, kw.pop("cos", cos), kw.pop("sin", sin), B, S, H, hd, pos0, K.v, V.v, **kw)
        return W, K, V
    good = run()
    same = run()
    for g, s in zip(good, same):
        G.assert_bits(g, s, "the reference twice")

    def swapped(x, p0):                                       # rotate_half = cat(x2, −x1): the halves' roles swapped
        c, s = cos[p0:p0 + S].view(1, 1, S, half), sin[p0:p0 + S].view(1, 1, S, half)
        x1, x2 = x[..., :half], x[..., half:]
        rb = G.P.rb
        return torch.cat([rb(rb(x1 * c) + rb(x2 * s)), rb(rb(x2 * c) + rb(-x1 * s))], -1)
    bad = run(rotate=swapped)
    rejected(G.assert_bits, bad[0], good[0], "halves swapped: q")
    rejected(G.assert_bits, bad[1], good[1], "halves swapped: k cache")
    G.assert_bits(bad[2], good[2], "halves swapped: v cache is a copy all the same")
    bad = run(cos=cos[1:], sin=sin[1:])                         # the angle of position pos0 + s + 1
    rejected(G.assert_bits, bad[0], good[0], "position off by one: q")
    rejected(G.assert_bits, bad[1], good[1], "position off by one: k cache")
    bad = run(cache_pos0=pos0 + 1)                              # right values, one cache slot late
    G.assert_bits(bad[0], good[0], "one slot late: q is right")
    rejected(G.assert_bits, bad[1], good[1], "one slot late: k cache")
    rejected(G.assert_bits, bad[2], good[2], "one slot late: v cache")
    inplace = Q.host()                                          # k rotated in place although the caches are given
    G.rope_(inplace.v, cos, sin, B, S, H, hd, pos0)
    rejected(G.assert_bits, inplace, good[0], "k third rotated in place")
    assert torch.equal(inplace.v[:, :H * hd], good[0].v[:, :H * hd])     # and only the k third tells them apart


# ---- copies -------------------------------------------------------------------------------------------------------------------
def test_copies_against_loops_and_one_slot_late():
    B, L, dim, V, npatch = 3, 4, 8, 5, 2
    ids = torch.tensor([[0, 4, 4, 1], [4, 0, 2, 2], [3, 3, 3, V - 1]])
    table = rand_bf16((V, dim), 1).to(bf16)
    dst = G.Flat((B, L + npatch, dim), CPU)
    got = dst.host()
    G.embed_splice_(ids, table, got.v, npatch)
    want = dst.host()
    for b in range(B):
        for j in range(L):
            want.v[b, 0 if j == 0 else j + npatch] = table[ids[b, j]]
    G.assert_bits(got, want, "embed_splice")
    assert bool(got.v[:, 1:1 + npatch].isnan().all())
    late = dst.host()
    for b in range(B):
        for j in range(L):
            r = b * (L + npatch) + (0 if j == 0 else j + npatch) + (j == L - 1)          # the last one lands in the guard
            late.buf[late.guard + r * dim:late.guard + (r + 1) * dim] = table[ids[b, j]]
    rejected(G.assert_bits, late, got, "embed_splice: last row one slot late")
    # prefix broadcast
    n_prefix, T = 3, 5
    pre = rand_bf16((n_prefix, dim), 2).to(bf16)
    x = G.Flat((B * T, dim), CPU)
    got, want = x.host(), x.host()
    G.write_prefix_(pre, got.v, B, T)
    for b in range(B):
        for j in range(n_prefix):
            want.v[b * T + j] = pre[j]
    G.assert_bits(got, want, "write_prefix_tokens")
    late = x.host()
    G.write_prefix_(pre, late.buf[late.guard + dim:late.guard + dim + B * T * dim].view(B * T, dim), B, T)    # every row one slot late
    rejected(G.assert_bits, late, got, "write_prefix_tokens one slot late")


def test_im2col_is_unfold_and_pad_columns_matter():
    pv = rand_bf16((2, 6, 224, 224), 3)
    for chan0 in (0, 3):
        pix = pv.clone()
        pix[:, 3 - chan0:6 - chan0] = G.NAN                                       # the other tower's channels are never read
        ref = F.unfold(pv[:, chan0:chan0 + 3], kernel_size=14, stride=14).transpose(1, 2).reshape(2 * 256, 588)
        for ld in (592, 640):
            out = G.Win(2 * 256, ld, CPU)
            got, want = out.host(), out.host()
            G.im2col_(pix.to(bf16), chan0, got.v)
            want.v[:, :588] = ref.to(bf16)
            want.v[:, 588:] = 0
            G.assert_bits(got, want, f"im2col chan0 {chan0} ld {ld}")
            unzeroed = out.host()
            unzeroed.v[:, :588] = ref.to(bf16)
            rejected(G.assert_bits, unzeroed, got, "im2col: pad columns left as they were")
            unzeroed.v[:, 588:] = 0
            unzeroed.v[17, ld - 1] = G.NAN                                        # one pad element missed
            rejected(G.assert_bits, unzeroed, got, "im2col: one pad element left")


def test_pack_formula_round_trip_and_block_offsets():
    from bridgelang_amd.ops import unpack_weight
    N, K, kt_total = 48, 96, 7
    w = rand_bf16((N, K), 5).to(bf16)
    for kb in (0, 2, kt_total - K // 32):
        dst = G.Flat((N // 16, kt_total, 64, 8), CPU)
        got, want = dst.host(), dst.host()
        G.pack_into_(w, got.v, kb)
        for nt in range(N // 16):
            for ks in range(K // 32):
                for lane in range(64):
                    r, c = 16 * nt + (lane & 15), 32 * ks + 8 * (lane >> 4)
                    want.v[nt, kb + ks, lane] = w[r, c:c + 8]
        G.assert_bits(got, want, f"pack_into kb {kb}")
        assert torch.equal(unpack_weight(got.v)[:, 32 * kb:32 * kb + K], w)            # the inverse
        other = torch.ones(kt_total, dtype=torch.bool)
        other[kb:kb + K // 32] = False
        assert bool(got.v[:, other].isnan().all())                                      # the other k-blocks keep their sentinel
        if kb:
            off = dst.host()
            G.pack_into_(w, off.v, kb - 1)
            rejected(G.assert_bits, off, got, "pack_into one k-block early")
    dense = G.Flat((N // 16, K // 32, 64, 8), CPU).host()
    G.pack_into_(w, dense.v)
    assert torch.equal(unpack_weight(dense.v), w)
    tr = G.Flat((N // 16, K // 32, 64, 8), CPU).host()                                  # lane → (row, chunk) transposed
    tr.v.copy_(dense.v.view(N // 16, K // 32, 4, 16, 8).transpose(2, 3).reshape(dense.v.shape))
    rejected(G.assert_bits, tr, dense, "pack: lanes in chunk-major order")


# ---- argmax ---------------------------------------------------------------------------------------------------------------------
def _argmax_nan_never_wins(lg):
    """The comparison `q > best || (q == best && i < bi)` from (−inf, 0x7fffffff): a NaN never wins."""
    x = torch.where(lg.isnan(), torch.full_like(lg, -math.inf), lg)
    out = torch.argmax(x, -1)
    return torch.where(lg.isnan().all(-1), torch.full_like(out, 0x7FFFFFFF), out)


@pytest.mark.parametrize("n", [4, 1024, 1028, 32064])
def test_argmax_rows_specification_and_near_misses(n):
    lg, names = G.argmax_rows(n, n + 8)
    assert bool(lg[:, n:].isinf().logical_or(lg[:, n:].isnan()).all())
    row = lg[:, :n]
    want = torch.tensor([G.first_nan_else_first_max(r) for r in row])
    G.check_argmax(want, lg, n, "the plain loop", names)                                 # torch.argmax is that specification
    assert want[names.index("all NaN")] == 0 and want[names.index("all -inf")] == 0 and want[names.index("all equal")] == 0
    assert want[names.index("-0 then +0")] == 0 and want[names.index("+0 then -0")] == 0
    assert bool(row[names.index("one NaN")].isnan().sum() == 1)
    last = n - 1 - torch.argmax(row.flip(-1), -1)                                        # ties (and NaNs) to the LAST index
    rejected(G.check_argmax, last, lg, n, "ties to the last index")
    tie_rows = [i for i, s in enumerate(names) if s.startswith("tie") or s == "all equal"]
    assert bool((last[tie_rows] != want[tie_rows]).any())
    old = _argmax_nan_never_wins(row)
    rejected(G.check_argmax, old, lg, n, "NaN never wins")
    assert old[names.index("all NaN")] == 0x7FFFFFFF                                      # the id that indexed the embedding table
    nan_rows = [i for i, s in enumerate(names) if "NaN" in s]
    assert bool((old[nan_rows] != want[nan_rows]).any()) and bool((old[[i for i in range(len(names)) if i not in nan_rows]]
                                                                 == want[[i for i in range(len(names)) if i not in nan_rows]]).all())
    rejected(G.check_argmax, torch.argmax(lg, -1), lg, n, "a kernel that reads the padding")


# ---- cross-entropy ----------------------------------------------------------------------------------------------------------------
def _ce_fp32(logits, targets, ignore_index=-100, guard=True):
    """glue.hip's two-pass row loss and masked mean in fp32 torch. guard=False: the row is indexed by whatever the target
    is (here: the flattened logits, as an unguarded kernel would read its neighbour row or column)."""
    rows, n = logits.shape
    mx = logits.amax(-1)
    s = torch.exp(logits - mx[:, None]).sum(-1)
    valid = targets != ignore_index
    inside = (targets >= 0) & (targets < n)
    flat = logits.reshape(-1)
    at = (torch.arange(rows) * n + torch.where(valid, targets, torch.zeros_like(targets))).clamp(0, rows * n - 1)
    lt = flat[at]
    if guard:
        lt = torch.where(inside | ~valid, lt, torch.full_like(lt, G.NAN))
    loss = torch.where(valid, torch.log(s) + mx - lt, torch.zeros(()))
    cnt = int(valid.sum())
    return loss, torch.tensor([loss.sum().item() / cnt if cnt else 0.0, float(cnt)], dtype=f32)


@pytest.mark.parametrize("n", [4, 1028])
def test_cross_entropy_rows_reference_and_near_misses(n):
    rows = 12
    logits, tgt = ce_case(rows, n)
    ref = T64.cross_entropy(logits, tgt)
    assert set(ref) >= {"dl", "mag", "mean", "m_mean", "count", "loss", "lmag"}
    per_row = F.cross_entropy(logits.double(), tgt, ignore_index=-100, reduction="none")
    assert torch.allclose(ref["loss"], per_row, rtol=1e-12, atol=1e-12)
    assert abs(ref["loss"].sum().item() / ref["count"] - ref["mean"].item()) <= 1e-12 and bool((ref["loss"][::3] == 0).all())
    assert abs(ref["lmag"].sum().item() / ref["count"] - ref["m_mean"].item()) <= 1e-9
    loss, mc = _ce_fp32(logits, tgt)
    G.check_cross_entropy("cpu legit fp32 ce", loss, mc, logits, tgt)
    shifted = torch.where(tgt >= 0, (tgt + 1) % n, tgt)                                   # the target read one column off
    rejected(G.check_cross_entropy, "one column off", *_ce_fp32(logits, shifted), logits, tgt)
    neg = loss.clone()
    neg[0] = -0.0
    rejected(G.check_cross_entropy, "ignored row -0", neg, mc, logits, tgt)
    # all rows ignored, exactly one valid row
    none = torch.full_like(tgt, -100)
    G.check_cross_entropy("cpu all ignored", *_ce_fp32(logits, none), logits, none)
    one = none.clone()
    one[7] = tgt[7]
    G.check_cross_entropy("cpu one valid row", *_ce_fp32(logits, one), logits, one)
    # targets outside the vocabulary: NaN with the guard, a silent wrong loss without
    for bad in (-1, n, n + 3):
        out = tgt.clone()
        out[4] = bad
        G.check_cross_entropy_outside(f"cpu guarded target {bad}", *_ce_fp32(logits, out), logits, out)
        rejected(G.check_cross_entropy_outside, f"unguarded target {bad}", *_ce_fp32(logits, out, guard=False), logits, out)


def ce_rows(rows, n):
    """`rows` rows of ce_case from its row 1 on (a valid row with target 0), so that one row is a case too."""
    logits, tgt = ce_case(rows + 11, n)
    return logits[1:1 + rows].contiguous(), tgt[1:1 + rows].contiguous()


MEAN_ROWS = [1, 255, 256, 257, 1000]


@pytest.mark.parametrize("rows", MEAN_ROWS)
def test_masked_mean_bound_holds_for_fp32_sums(rows):
    """A sequential fp32 sum per thread, then the 256 partials: the order of masked_mean_kernel up to the shuffle tree."""
    logits, tgt = ce_rows(rows, 8)
    loss, mc = _ce_fp32(logits, tgt)
    valid = tgt != -100
    part = torch.zeros(256, dtype=f32)
    for r0 in range(0, rows, 256):
        chunk = torch.where(valid[r0:r0 + 256], loss[r0:r0 + 256], torch.zeros(()))
        part[:len(chunk)] += chunk
    s = part.view(4, 64).sum(-1).sum()
    mc[0] = s / mc[1] if mc[1] > 0 else 0.0
    G.check_cross_entropy(f"cpu fp32 masked mean {rows} rows", loss, mc, logits, tgt)
    assert G.mean_c(rows) == T64.C_CE_MEAN + math.ceil(rows / 256) + 10
