"""The fp64 attention comparator (tests/attn_ref64.py) tells right from wrong, on the CPU.

Legitimate implementations (the oracle's bf16-rounding attention and autograd over it; an fp32 online-softmax forward
that rounds P to bf16 per 64-key chunk) must pass the per-element bound. Wrong algorithms, computed in fp64 so that only
the algorithm is wrong, must fail it. Which of the wrong algorithms the older whole-tensor checks (`grad_close` at
2.5e-2, `close_bf16`) would accept is printed as evidence; it asserts nothing.
"""
import math

import pytest
import torch

from attn_ref64 import (C_DK, C_DQ, C_DV, C_O, LOG2E, assert_attn_close, assert_lse_close, backward, forward, peaked_q,
                        visible)
from conftest import rand_bf16
from oracle import restate as R

P = R.Prec(True)

# (B, H, Sq, Skv, hd, causal, masked lengths or None)
SMALL = (2, 2, 45, 45, 64, True, [45, 30])
LONG = (1, 2, 333, 333, 128, True, None)
NONCAUSAL = (2, 2, 150, 150, 72, False, [150, 97])


def _inputs(B, H, Sq, Skv, hd, causal, lens, seed, peaked=False):
    q, k, v = (rand_bf16((B, H, n, hd), seed + i) for i, n in enumerate((Sq, Skv, Skv)))
    mask = None
    if lens is not None:
        mask = torch.zeros(B, Skv, dtype=torch.uint8)
        for b, n in enumerate(lens):
            mask[b, :n] = 1
    if peaked:
        q = peaked_q(q, k, causal, mask)
    do = rand_bf16((B, H, Sq, hd), seed + 7)
    return q, k, v, do, mask


def _rows(B, Sq, lens):
    rows = torch.ones(B, Sq, dtype=torch.bool)
    if lens is not None:
        for b, n in enumerate(lens):
            rows[b, n:] = False
    return rows


def _online_fp32(q, k, v, scale, causal, mask, chunk=64):
    """fp32 chunked online softmax in the base-2 domain, P rounded to bf16 per chunk (the chunked forward kernel's
    arithmetic, attention.hip attn_fwd_kernel): returns bf16-valued o and fp32 lse2."""
    B, H, Sq, hd = q.shape
    Skv = k.shape[2]
    sl2e = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    o = torch.zeros(B, H, Sq, v.shape[-1])
    lse = torch.zeros(B, H, Sq)
    for b in range(B):
        vis = visible(Sq, Skv, causal, None if mask is None else mask[b])
        m_run = torch.full((H, Sq, 1), float("-inf"))
        l = torch.zeros(H, Sq, 1)
        acc = torch.zeros(H, Sq, v.shape[-1])
        for c0 in range(0, Skv, chunk):
            s = (q[b] @ k[b, :, c0:c0 + chunk].transpose(-1, -2)) * sl2e
            s = s.masked_fill(~vis[:, c0:c0 + chunk], float("-inf"))
            m_new = torch.maximum(m_run, s.amax(-1, keepdim=True))
            m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp2(m_run - m_use)
            e = torch.exp2(s - m_use)
            l = l * alpha + e.sum(-1, keepdim=True)
            acc = acc * alpha + P.rb(e) @ v[b, :, c0:c0 + chunk]
            m_run = m_new
        o[b] = P.rb(acc / torch.where(l > 0, l, torch.ones_like(l)))
        lse[b] = torch.where(l > 0, m_run + torch.log2(l), torch.full_like(l, float("inf"))).squeeze(-1)
    return o, lse


@pytest.mark.parametrize("shape", [SMALL, LONG, NONCAUSAL], ids=["small-causal-masked", "long-causal-S333", "hd72-masked"])
@pytest.mark.parametrize("peaked", [False, True], ids=["randn", "peaked"])
def test_legitimate_implementations_pass(shape, peaked):
    B, H, Sq, Skv, hd, causal, lens = shape
    q, k, v, do, mask = _inputs(*shape, seed=3, peaked=peaked)
    scale = hd ** -0.5
    rows = _rows(B, Sq, lens)
    ref = forward(q, k, v, scale, causal, mask)
    # 1. the oracle's bf16-rounding attention (two-pass softmax, P rounded to bf16, O rounded to bf16)
    o_r = R.attention(P, q, k, v, scale, causal, key_mask=mask)
    assert_attn_close(o_r, ref["o"], ref["m_o"], C_O, "cpu legit restate O", rows)
    # 2. fp32 online softmax, P rounded per 64-key chunk
    o_on, lse_on = _online_fp32(q, k, v, scale, causal, mask)
    assert_attn_close(o_on, ref["o"], ref["m_o"], C_O, "cpu legit online O", rows)
    assert_lse_close(lse_on, ref["lse2"], ref["mag_s"], "cpu legit online lse", rows)
    # 3. autograd over the oracle's attention. Its delta comes from the fp32 O before the final bf16 rounding, so the
    #    reference is given that O (the kernels get, and are checked with, their own bf16 O).
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_a = R.attention(P, qr, kr, vr, scale, causal, key_mask=mask)
    g = do * rows.view(B, 1, Sq, 1)
    (o_a * g).sum().backward()
    with torch.no_grad():
        s = (q @ k.transpose(-1, -2)) * scale
        vis = torch.stack([visible(Sq, Skv, causal, None if mask is None else mask[b]) for b in range(B)])
        s = s.masked_fill(~vis[:, None], float("-inf"))
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        o_pre = (P.rb(e) @ v) / torch.where(l > 0, l, torch.ones_like(l))
    rb = backward(q, k, v, o_pre, g, scale, causal, mask)
    assert_attn_close(qr.grad, rb["dq"], rb["m_dq"], C_DQ, "cpu legit autograd dQ", rows)
    assert_attn_close(kr.grad, rb["dk"], rb["m_dk"], C_DK, "cpu legit autograd dK")
    assert_attn_close(vr.grad, rb["dv"], rb["m_dv"], C_DV, "cpu legit autograd dV")


# ---- wrong algorithms, each computed in fp64 ------------------------------------------------------------------------
def _softmax64(s):
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return e / torch.where(l > 0, l, torch.ones_like(l))


def _scores(q, k, scale):
    return scale * (q.double() @ k.double().transpose(-1, -2))


def _fwd_with_vis(q, k, v, scale, vis):
    s = _scores(q, k, scale).masked_fill(~vis, float("-inf"))
    return _softmax64(s) @ v.double()


def _vis_all(B, Sq, Skv, causal, mask, shift=0):
    out = []
    for b in range(B):
        vis = visible(Sq, Skv, False, None if mask is None else mask[b])
        if causal:
            i = torch.arange(Sq).view(-1, 1) + (Skv - Sq) + shift
            vis = vis & (torch.arange(Skv).view(1, -1) <= i)
        out.append(vis)
    return torch.stack(out)[:, None]


def _bwd_from_p(p, q, k, v, o, do, scale, dk_scale=None):
    q, k, v, o, do = (t.double() for t in (q, k, v, o, do))
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    return dict(dq=scale * ds @ k, dk=(scale if dk_scale is None else dk_scale) * ds.transpose(-1, -2) @ q,
                dv=p.transpose(-1, -2) @ do)


def _wrong_cases():
    """name → function(q, k, v, do, mask, scale, o_bf16) → {tensor name ("o", "dq", "dk", "dv"): fp64 result}."""
    def causal_shift(shift):
        def f(q, k, v, do, mask, scale, o):
            B, H, Sq, _ = q.shape
            return {"o": _fwd_with_vis(q, k, v, scale, _vis_all(B, Sq, k.shape[2], True, mask, shift))}
        return f

    def drop_tile(width):
        def f(q, k, v, do, mask, scale, o):
            B, H, Sq, _ = q.shape
            vis = _vis_all(B, Sq, k.shape[2], True, mask).clone()
            vis[..., 64:64 + width] = False             # one tile of keys skipped by every row
            return {"o": _fwd_with_vis(q, k, v, scale, vis)}
        return f

    def leak(q, k, v, do, mask, scale, o):
        B, H, Sq, _ = q.shape
        vis = _vis_all(B, Sq, k.shape[2], True, mask).clone()
        vis[1, :, HOLE:, HOLE] = True                   # the masked key inside batch element 1's valid rows
        return {"o": _fwd_with_vis(q, k, v, scale, vis)}

    def neighbour_lse(q, k, v, do, mask, scale, o):
        B, H, Sq, _ = q.shape
        s = _scores(q, k, scale).masked_fill(~_vis_all(B, Sq, k.shape[2], True, mask), float("-inf"))
        lse = torch.logsumexp(s, -1, keepdim=True)
        lse_n = torch.cat([lse[..., 1:, :], lse[..., -1:, :]], dim=-2)      # row i uses row i + 1's
        p = torch.exp(s - lse_n)
        return _bwd_from_p(p, q, k, v, o, do, scale)

    def no_rescale(q, k, v, do, mask, scale, o):
        # online softmax in fp64 where the accumulators are NOT rescaled when the last chunk raises the max
        B, H, Sq, _ = q.shape
        Skv = k.shape[2]
        s = _scores(q, k, scale).masked_fill(~_vis_all(B, Sq, Skv, True, mask), float("-inf"))
        m_run = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
        l = torch.zeros_like(m_run)
        acc = torch.zeros(s.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
        n_chunks = (Skv + 63) // 64
        for c in range(n_chunks):
            sc = s[..., 64 * c:64 * c + 64]
            m_new = torch.maximum(m_run, sc.amax(-1, keepdim=True))
            m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp(m_run - m_use)
            if c == n_chunks - 1:
                alpha = torch.ones_like(alpha)            # the defect: last chunk added without its rescale
            e = torch.exp(sc - m_use)
            l = l * alpha + e.sum(-1, keepdim=True)
            acc = acc * alpha + e @ v.double()[..., 64 * c:64 * c + 64, :]
            m_run = m_new
        return {"o": acc / torch.where(l > 0, l, torch.ones_like(l))}

    def dk_no_scale(q, k, v, do, mask, scale, o):
        B, H, Sq, _ = q.shape
        p = _softmax64(_scores(q, k, scale).masked_fill(~_vis_all(B, Sq, k.shape[2], True, mask), float("-inf")))
        return _bwd_from_p(p, q, k, v, o, do, scale, dk_scale=1.0)

    def delta_other_head(q, k, v, do, mask, scale, o):
        B, H, Sq, _ = q.shape
        p = _softmax64(_scores(q, k, scale).masked_fill(~_vis_all(B, Sq, k.shape[2], True, mask), float("-inf")))
        o_wrong = o.roll(1, dims=1)                                         # head h takes head h - 1's O
        q, k, v, do = (t.double() for t in (q, k, v, do))
        dp = do @ v.transpose(-1, -2)
        ds = p * (dp - (do * o_wrong.double()).sum(-1, keepdim=True))
        return dict(dq=scale * ds @ k, dk=scale * ds.transpose(-1, -2) @ q, dv=p.transpose(-1, -2) @ do)

    return {
        "causal-off-by-one-plus": causal_shift(+1),
        "causal-off-by-one-minus": causal_shift(-1),
        "dropped-16-key-tile": drop_tile(16),
        "dropped-64-key-tile": drop_tile(64),
        "leaked-masked-key": leak,
        "neighbour-row-lse": neighbour_lse,
        "chunk-without-rescale": no_rescale,
        "dk-without-scale": dk_no_scale,
        "delta-from-other-head": delta_other_head,
    }


WRONG = _wrong_cases()
WRONG_SHAPE = (2, 2, 200, 200, 128, True, [200, 150])
HOLE = 40                                              # batch element 1 also masks this key inside its valid rows


@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_algorithms_fail(name):
    from test_ops_gpu import close_bf16
    from test_train_ops_gpu import grad_close
    B, H, Sq, Skv, hd, causal, lens = WRONG_SHAPE
    q, k, v, do, mask = _inputs(*WRONG_SHAPE, seed=11, peaked=(name == "chunk-without-rescale"))
    mask[1, HOLE] = 0
    scale = hd ** -0.5
    rows = _rows(B, Sq, lens)
    ref = forward(q, k, v, scale, causal, mask)
    o_bf = ref["o"].float().to(torch.bfloat16).float()         # the bf16 O a kernel would hand to its backward
    do = do * rows.view(B, 1, Sq, 1)
    got = WRONG[name](q, k, v, do, mask, scale, o_bf)
    refs = {"o": (ref["o"], ref["m_o"], C_O)}
    if set(got) - {"o"}:
        rb = backward(q, k, v, o_bf, do, scale, causal, mask)
        refs.update(dq=(rb["dq"], rb["m_dq"], C_DQ), dk=(rb["dk"], rb["m_dk"], C_DK), dv=(rb["dv"], rb["m_dv"], C_DV))
    caught, old = [], []
    for t, val in got.items():
        r, mag, c = refs[t]
        rws = rows if t in ("o", "dq") else None
        try:
            assert_attn_close(val, r, mag, c, f"cpu wrong {name} {t}", rws)
        except AssertionError as ex:
            caught.append(f"{t}: {str(ex)[:160]}")
        # the older checks, on the valid rows, as the existing GPU tests call them (information only)
        ref_old = r if t != "o" else R.attention(P, q, k, v, scale, causal, key_mask=mask).double()
        for b in range(B):
            sl = (slice(None), slice(0, lens[b])) if t in ("o", "dq") else (slice(None),)
            g_b, r_b = val[b][sl].float(), ref_old[b][sl].float()
            try:
                if t == "o":
                    close_bf16(g_b.to(torch.bfloat16), r_b, "old", rtol=2 ** -5, atol_scale=2 ** -7, min_exact=0.55)
                else:
                    grad_close(g_b, r_b, "old", tol=2.5e-2)
                verdict = "accepts"
            except AssertionError:
                verdict = "rejects"
            old.append(f"{t} b={b}: {'close_bf16' if t == 'o' else 'grad_close(2.5e-2)'} {verdict}")
    print(f"{name}: new bound rejects {len(caught)} of {len(got)} tensors; old checks: " + "; ".join(old))
    assert caught, f"{name}: the fp64 bound accepted a wrong algorithm"


def test_empty_row_reference():
    """A row with no visible key: o = 0, lse = +inf, zero gradients (attention.hip:28)."""
    B, H, S, hd = 2, 1, 20, 64
    q, k, v, do, _ = _inputs(B, H, S, S, hd, False, None, seed=5)
    mask = torch.ones(B, S, dtype=torch.uint8)
    mask[1] = 0
    f = forward(q, k, v, hd ** -0.5, False, mask)
    assert torch.all(f["o"][1] == 0) and torch.all(torch.isinf(f["lse2"][1])) and torch.isfinite(f["lse2"][0]).all()
    bw = backward(q, k, v, f["o"], do, hd ** -0.5, False, mask)
    for t in ("dq", "dk", "dv"):
        assert torch.all(bw[t][1] == 0)
    # the comparator accepts exact zeros and infinities and rejects a wrong finite lse for an empty row
    assert_attn_close(f["o"].float(), f["o"], f["m_o"], C_O, "cpu empty-row O")
    assert_lse_close(f["lse2"].float(), f["lse2"], f["mag_s"], "cpu empty-row lse")
    bad = f["lse2"].clone()
    bad[1] = 0.0
    with pytest.raises(AssertionError):
        assert_lse_close(bad, f["lse2"], f["mag_s"], "cpu empty-row lse (wrong)")
    assert math.isinf(float(f["lse2"][1, 0, 0]))
