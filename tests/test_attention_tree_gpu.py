"""The shared-prompt attention pair (attention_tree.hip: bl_attention_tree_lse_bf16 / bl_attention_tree_backward_bf16) and the
per-row rotary embedding (bl_rope_pos_bf16 / bl_rope_pos_backward_bf16).

Attention: every output element against an fp64 reference built from the pieces of tests/attn_ref64.py (its `_probs`, its
magnitude companions, its comparators and its constants C_O, C_DV, C_DQ, C_DK, LSE_REL, unchanged) with the tree visibility
of bridgelang_amd/training/shared_prompt.py::tree_visible passed in. q / k / v are the three thirds of fused qkv rows and dq /
dk / dv those of fused dqkv rows, as the training step lays them out; every buffer has guard rows in front and behind that
must still hold their sentinel afterwards.

Shapes: B = 2, H = 2, hd = 128 over prefix ∈ {1, 31, 33, 288} × branch ∈ {1, 7, 8} × G ∈ {1, 2, 8, 16} (totals from 2 to 416
rows: 64-row query tiles and 128-row blocks that end inside a branch, 16-row tiles that hold two or sixteen branches), each
with a key mask that hides the tail of the prefix of batch element 1, flat and peaked scores; one case with the last rows of
every branch masked (short branches). With G = 1 the mask is plain causal and the results are held to the same bound.

What this grid does not reach (tests/tree_paths.py is the host model of the kernels' tile schedule that counts it, and
tests/test_tree_paths_cpu.py pins the counts): no 256-key chunk is ever skipped by a dq workgroup, the forward skips one chunk
in one tile of one case, no dkv workgroup walks more than two 256-row chunks or starts past row 256, no branch is longer than
8 rows, and no chunk or step is fully masked. tests/test_attention_tree_long_gpu.py runs those paths — past 512 rows, branches
up to 300 rows, masks that hide whole chunks — with the helpers of this file and the same bounds.
"""
import numpy as np
import pytest
import torch

import attn_ref64 as A
from attn_ref64 import C_DK, C_DQ, C_DV, C_O, FLOOR, assert_attn_close, assert_lse_close
from conftest import rand_bf16

pytestmark = pytest.mark.gpu
SENT = -7.0          # guard-row sentinel (bf16-exact)
GR = 3               # guard rows in front of and behind every row buffer
B, H, HD = 2, 2, 128

PREFIXES, BRANCHES, GROUPS = (1, 31, 33, 288), (1, 7, 8), (1, 2, 8, 16)
CASES = [(p, nb, g) for p in PREFIXES for nb in BRANCHES for g in GROUPS]


def _vis(prefix, branch, S, mask):
    from bridgelang_amd.training.shared_prompt import tree_visible
    return [torch.from_numpy(tree_visible(prefix, branch, S, None if mask is None else mask[b].numpy())) for b in range(B)]


def _mask(prefix, branch, G, hide_prefix=(0, 3), short=0):
    """[B, S] uint8: batch element b hides the last min(hide_prefix[b], prefix − 1) prefix rows and the last `short` rows of
    every branch."""
    S = prefix + G * branch
    m = torch.ones(B, S, dtype=torch.uint8)
    for b in range(B):
        h = min(hide_prefix[b], prefix - 1)
        if h:
            m[b, prefix - h:prefix] = 0
        if short:
            for g in range(G):
                m[b, prefix + (g + 1) * branch - short:prefix + (g + 1) * branch] = 0
    return m


def _peaked(q, k, vis, gain=1.5):
    """attn_ref64.peaked_q under a given visibility: q ×4 and each row's largest score moved to its last visible key."""
    out = 4.0 * q.float()
    S = q.shape[2]
    for b in range(B):
        v = vis[b]
        last = torch.where(v.any(1), S - 1 - v.flip(1).int().argmax(1), torch.full((S,), -1))
        rows = last >= 0
        out[b][:, rows] += gain * k[b].float()[:, last[rows]]
    return out.to(torch.bfloat16).float()


def ref_forward(q, k, v, scale, vis):
    q, k, v = (t.double() for t in (q, k, v))
    o, m_o = torch.zeros_like(q), torch.zeros_like(q)
    lse2, mag_s = torch.zeros(q.shape[:3], dtype=torch.float64), torch.zeros(q.shape[:3], dtype=torch.float64)
    for b in range(q.shape[0]):
        p, lse2[b] = A._probs(q[b], k[b], scale, vis[b])
        o[b], m_o[b] = p @ v[b], p @ v[b].abs()
        mag_s[b] = (scale * A.LOG2E) * (p * (q[b].abs() @ k[b].abs().transpose(-1, -2))).sum(-1)
    return dict(o=o, lse2=lse2, m_o=m_o, mag_s=mag_s)


def ref_backward(q, k, v, o, do, scale, vis):
    q, k, v, o, do = (t.double() for t in (q, k, v, o, do))
    out = {n: torch.zeros_like(q) for n in ("dq", "dk", "dv", "m_dq", "m_dk", "m_dv")}
    out["delta"] = torch.zeros(q.shape[:3], dtype=torch.float64)
    for b in range(q.shape[0]):
        p, _ = A._probs(q[b], k[b], scale, vis[b])
        dp = do[b] @ v[b].transpose(-1, -2)
        dl = (do[b] * o[b]).sum(-1, keepdim=True)
        ds, dsm = p * (dp - dl), p * (dp.abs() + dl.abs())
        out["delta"][b] = dl.squeeze(-1)
        out["dq"][b], out["m_dq"][b] = scale * (ds @ k[b]), scale * (dsm @ k[b].abs())
        out["dk"][b], out["m_dk"][b] = scale * (ds.transpose(-1, -2) @ q[b]), scale * (dsm.transpose(-1, -2) @ q[b].abs())
        out["dv"][b], out["m_dv"][b] = p.transpose(-1, -2) @ do[b], p.transpose(-1, -2) @ do[b].abs()
    return out


def _rows(t):
    """[B, H, S, hd] → [B·S, H·hd] rows."""
    b, h, s, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b * s, h * d)


def _heads(rows, S):
    return rows.view(B, S, H, HD).permute(0, 2, 1, 3).float()


def _guarded(body, dev):
    buf = torch.full((body.shape[0] + 2 * GR, body.shape[1]), SENT, dtype=torch.bfloat16)
    buf[GR:GR + body.shape[0]] = body.to(torch.bfloat16)
    return buf.to(dev)


def _guards_intact(buf, what):
    c = buf.cpu().float()
    assert bool((c[:GR] == SENT).all()) and bool((c[-GR:] == SENT).all()), f"{what}: guard rows were written"


def run_tree(dev, q, k, v, mask, prefix, branch, do=None, stat_fill=None):
    """The kernels over fused qkv rows with guard rows; CPU float [B, H, S, hd] results and lse / delta [B, H, S]. `stat_fill`
    (default: the sentinel) is what lse / delta hold before the call, their pad rows [S, pad32(S)) included; those come back
    as lse_pad / delta_pad."""
    from bridgelang_amd import train_ops as T
    S, D = q.shape[2], H * HD
    qkv = _guarded(torch.cat([_rows(q), _rows(k), _rows(v)], dim=1), dev)
    o = _guarded(torch.zeros(B * S, D), dev)
    body, ob = qkv[GR:GR + B * S], o[GR:GR + B * S]
    pad = (S + 31) // 32 * 32
    PADG = 16        # guard floats round lse / delta (multiples of 4 keep the 16-byte alignment)
    lse = torch.full((B * H * pad + 2 * PADG,), float(SENT), device=dev)
    if stat_fill is not None:
        lse[PADG:PADG + B * H * pad] = stat_fill
    st, so = (S * 3 * D, HD, 3 * D), (S * D, HD, D)
    kw = dict(B=B, H=H, S=S, prefix=prefix, branch=branch, head_dim=HD, q_strides=st, k_strides=st, v_strides=st, o_strides=so,
              key_mask=None if mask is None else mask.to(dev))
    lv = lse[PADG:PADG + B * H * pad]
    T.attention_tree_lse(body[:, :D], body[:, D:2 * D], body[:, 2 * D:], ob, lv, **kw)
    torch.cuda.synchronize()
    _guards_intact(qkv, "forward qkv")
    _guards_intact(o, "forward o")
    assert bool((lse[:PADG] == SENT).all()) and bool((lse[-PADG:] == SENT).all()), "forward: lse guards were written"
    out = dict(o=_heads(ob.cpu(), S), lse=lv.cpu().view(B, H, pad)[:, :, :S].clone(), o_bits=ob.cpu().view(torch.int16).clone(),
               lse_bits=lv.cpu().view(torch.int32).view(B, H, pad)[:, :, :S].clone(), lse_pad=lv.cpu().view(B, H, pad)[:, :, S:].clone())
    if do is not None:
        g = _guarded(_rows(do), dev)
        dqkv = _guarded(torch.zeros(B * S, 3 * D), dev)
        db = dqkv[GR:GR + B * S]
        delta = torch.full((B * H * pad + 2 * PADG,), float(SENT), device=dev)
        dl = delta[PADG:PADG + B * H * pad]
        if stat_fill is not None:
            dl.fill_(stat_fill)
        T.attention_tree_backward(body[:, :D], body[:, D:2 * D], body[:, 2 * D:], ob, g[GR:GR + B * S], lv, dl,
                                  db[:, :D], db[:, D:2 * D], db[:, 2 * D:], **kw)
        torch.cuda.synchronize()
        _guards_intact(dqkv, "backward dqkv")
        _guards_intact(qkv, "backward qkv")
        assert bool((delta[:PADG] == SENT).all()) and bool((delta[-PADG:] == SENT).all()), "backward: delta guards were written"
        c = db.cpu()
        out.update(dq=_heads(c[:, :D].contiguous(), S), dk=_heads(c[:, D:2 * D].contiguous(), S), dv=_heads(c[:, 2 * D:].contiguous(), S),
                   delta=dl.cpu().view(B, H, pad)[:, :, :S].clone(), d_bits=c.view(torch.int16).clone(),
                   delta_pad=dl.cpu().view(B, H, pad)[:, :, S:].clone())
    return out


def case_inputs(prefix, branch, G, mask, seed, peaked):
    """q, k, v (bf16-representable fp32 [B, H, S, hd]) and the per-batch visibility of one case, from its seed alone."""
    S = prefix + G * branch
    q, k, v = (rand_bf16((B, H, S, HD), seed + i) for i in range(3))
    vis = _vis(prefix, branch, S, mask)
    if peaked:
        q = _peaked(q, k, vis)
    return q, k, v, vis


def check_case(dev, prefix, branch, G, mask, seed, peaked, what, stat_fill=None):
    S, scale = prefix + G * branch, HD ** -0.5
    q, k, v, vis = case_inputs(prefix, branch, G, mask, seed, peaked)
    rows = torch.ones(B, S, dtype=torch.bool) if mask is None else mask.bool()      # masked (padding) query rows are not specified
    do = rand_bf16((B, H, S, HD), seed + 4) * rows.view(B, 1, S, 1)
    got = run_tree(dev, q, k, v, mask, prefix, branch, do, stat_fill=stat_fill)
    ref = ref_forward(q, k, v, scale, vis)
    assert_attn_close(got["o"], ref["o"], ref["m_o"], C_O, f"tree fwd O {what}", rows)
    assert_lse_close(got["lse"], ref["lse2"], ref["mag_s"], f"tree fwd lse {what}", rows)
    rb = ref_backward(q, k, v, got["o"], do, scale, vis)
    assert_attn_close(got["dq"], rb["dq"], rb["m_dq"], C_DQ, f"tree bwd dQ {what}", rows)
    assert_attn_close(got["dk"], rb["dk"], rb["m_dk"], C_DK, f"tree bwd dK {what}")
    assert_attn_close(got["dv"], rb["dv"], rb["m_dv"], C_DV, f"tree bwd dV {what}")
    sel = rows.view(B, 1, S).expand(B, H, S)
    dmag = (do.double() * got["o"].double()).abs().sum(-1)
    derr = (got["delta"].double() - rb["delta"]).abs()
    assert bool((derr[sel] <= (2.0 ** -16 * dmag + FLOOR)[sel]).all()), f"{what}: delta differs from rowsum(dO * O)"
    if mask is not None:
        dead = (mask == 0).view(B, 1, S, 1).expand_as(got["dk"])
        assert bool((got["dk"][dead] == 0).all()) and bool((got["dv"][dead] == 0).all()), f"{what}: masked keys got gradient"
    return q, k, v, do, got


@pytest.mark.parametrize("prefix,branch,G", CASES, ids=[f"p{p}-nb{nb}-G{g}" for p, nb, g in CASES])
def test_tree_against_fp64(dev, prefix, branch, G):
    seed = 7000 + 10 * CASES.index((prefix, branch, G))
    mask = _mask(prefix, branch, G)
    for peaked in (False, True):
        check_case(dev, prefix, branch, G, mask, seed + (5 if peaked else 0), peaked,
                   f"p{prefix}-nb{branch}-G{G}-{'peaked' if peaked else 'flat'}")


def test_short_branches_and_repeatability(dev):
    """The last two rows of every branch masked (branches shorter than nb) beside a hidden prefix tail; and a second call
    over the same inputs gives identical bits (fixed summation order, no atomics)."""
    prefix, branch, G = 33, 8, 8
    mask = _mask(prefix, branch, G, hide_prefix=(2, 5), short=2)
    q, k, v, do, got = check_case(dev, prefix, branch, G, mask, 7900, True, "short-branches")
    again = run_tree(dev, q, k, v, mask, prefix, branch, do)
    for t in ("o_bits", "lse_bits", "d_bits"):
        assert torch.equal(got[t], again[t]), f"{t}: two calls differ"


def test_no_mask_and_masked_rows_are_never_read(dev):
    """key_mask = NULL runs; and K / V rows no compared query may see — masked keys and the OTHER branches — may hold ±3e4
    without changing a bit of a branch's outputs."""
    prefix, branch, G = 31, 7, 8
    S = prefix + G * branch
    check_case(dev, prefix, branch, G, None, 7950, False, "no-mask")
    mask = _mask(prefix, branch, G, hide_prefix=(0, 4))
    q, k, v = (rand_bf16((B, H, S, HD), 7960 + i) for i in range(3))
    keep = torch.zeros(B, S, dtype=torch.bool)
    keep[:, :prefix] = True
    keep[:, prefix + 2 * branch:prefix + 3 * branch] = True           # branch 2 and the prefix are compared
    keep &= mask.bool()
    do = rand_bf16((B, H, S, HD), 7964) * keep.view(B, 1, S, 1)
    hide = ~keep                                                       # every other branch, and the masked prefix tail
    hide[:, :prefix] = mask[:, :prefix] == 0
    big = 3.0e4 * (torch.randint(0, 2, k.shape, generator=torch.Generator().manual_seed(1)) * 2 - 1).float()
    sel = hide.view(B, 1, S, 1)
    base = run_tree(dev, q, k, v, mask, prefix, branch, do)
    pert = run_tree(dev, q, torch.where(sel, big, k), torch.where(sel, -big, v), mask, prefix, branch, do)
    rows = keep.view(B, 1, S, 1).expand(B, H, S, HD)
    for t in ("o", "dq", "dk", "dv"):
        assert torch.equal(base[t][rows], pert[t][rows]), f"{t}: changed when rows that must not be read were overwritten"


def test_argument_errors_launch_nothing(dev):
    from bridgelang_amd import _lib
    from bridgelang_amd import train_ops as T
    from bridgelang_amd.ops import run_all
    S, prefix, branch = 33 + 2 * 8, 33, 8
    D = H * HD
    qkv = torch.zeros(B * S, 3 * D, dtype=torch.bfloat16, device=dev)
    o = torch.full((B * S, D), SENT, dtype=torch.bfloat16, device=dev)
    dqkv = torch.full((B * S, 3 * D), SENT, dtype=torch.bfloat16, device=dev)
    pad = (S + 31) // 32 * 32
    lse, delta = torch.full((B * H * pad,), SENT, device=dev), torch.full((B * H * pad,), SENT, device=dev)
    st, so = (S * 3 * D, HD, 3 * D), (S * D, HD, D)
    good = dict(B=B, H=H, S=S, prefix=prefix, branch=branch, head_dim=HD, q_strides=st, k_strides=st, v_strides=st, o_strides=so)
    bad = [dict(prefix=0), dict(branch=0), dict(prefix=-1), dict(branch=7), dict(head_dim=64),
           dict(q_strides=(S * 3 * D, HD, 3 * D + 4)), dict(o_strides=(S * D + 2, HD, D)), dict(prefix=S + 8)]
    for change in bad:
        kw = dict(good, **change)
        for build in (lambda: T.attention_tree_lse(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, lse, run=False, **kw),
                      lambda: T.attention_tree_backward(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, o, lse, delta, dqkv[:, :D],
                                                        dqkv[:, D:2 * D], dqkv[:, 2 * D:], run=False, **kw)):
            with pytest.raises(_lib.BridgeLangHipError, match="BL_E_ARG|BL_E_SHAPE"):
                run_all([build()])
    cos = torch.zeros(64, HD // 2, dtype=torch.bfloat16, device=dev)
    pos = torch.zeros(B * S, dtype=torch.int32, device=dev)
    # head_dim not a multiple of 16, no heads, rows narrower than 3·H·head_dim
    for kw in (dict(H=H, head_dim=HD + 8), dict(H=0, head_dim=HD), dict(H=H + 1, head_dim=HD)):
        for fn in (T.rope_pos, T.rope_pos_backward):
            with pytest.raises(_lib.BridgeLangHipError, match="BL_E_SHAPE"):
                run_all([fn(dqkv, cos, cos, pos, rows=B * S, run=False, **kw)])
    torch.cuda.synchronize()
    for t in (o, dqkv, lse, delta):
        assert bool((t.float() == SENT).all()), "a rejected call wrote to an output"


# ---- per-row rotary embedding -------------------------------------------------------------------------------------------
def _rope_setup(dev, Bq, S, Hq, seed, extra_cols=16):
    from bridgelang_amd.engine import rope_tables
    from glue_ref import rope_inputs
    cos, sin = rope_tables(HD, 512, 10000.0, dev)
    D = Hq * HD
    body = torch.full((Bq * S, 3 * D + extra_cols), SENT)
    body[:, :3 * D] = rope_inputs(Bq, S, Hq, HD, seed)
    return cos, sin, body


def _rope_pair(dev, body, fn_ref, fn_pos):
    a, b = _guarded(body, dev), _guarded(body, dev)
    rows = body.shape[0]
    fn_ref(a[GR:GR + rows])
    fn_pos(b[GR:GR + rows])
    torch.cuda.synchronize()
    return a.cpu(), b.cpu()


@pytest.mark.parametrize("Bq,S,Hq,pos0", [(2, 19, 2, 0), (3, 40, 3, 7), (1, 1, 1, 300)])
def test_rope_pos_equals_rope_at_regular_positions(dev, Bq, S, Hq, pos0):
    from bridgelang_amd import train_ops as T
    cos, sin, body = _rope_setup(dev, Bq, S, Hq, 8100 + S)
    pos = (pos0 + torch.arange(Bq * S) % S).to(torch.int32).to(dev)
    kw = dict(H=Hq, head_dim=HD)
    for ref_fn, pos_fn, what in ((T.rope, T.rope_pos, "forward"), (T.rope_backward, T.rope_pos_backward, "backward")):
        a, b = _rope_pair(dev, body, lambda x: ref_fn(x, cos, sin, B=Bq, S=S, pos0=pos0, **kw),
                          lambda x: pos_fn(x, cos, sin, pos, rows=Bq * S, **kw))
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"rope_pos {what} differs from rope (guards and pad columns included)"
        assert not torch.equal(a[GR:-GR, :3 * Hq * HD].float(), body[:, :3 * Hq * HD]), "nothing was rotated"


def test_rope_pos_at_scattered_positions(dev):
    """Positions as the shared-prompt layout has them (runs that restart, repeats) against a host restatement of the rotation
    (tests/glue_ref.py::rope_, row by row), bit for bit; the backward against bl_rope_backward_bf16 called row by row."""
    from bridgelang_amd import train_ops as T
    from glue_ref import rope_
    rows, Hq = 23, 2
    cos, sin, body = _rope_setup(dev, 1, rows, Hq, 8200)
    g = torch.Generator().manual_seed(5)
    pos = torch.cat([torch.arange(9), 9 + torch.arange(4), 9 + torch.arange(4), torch.randint(0, 512, (6,), generator=g)]).to(torch.int32)
    assert pos.numel() == rows
    D = Hq * HD
    got = _guarded(body, dev)
    T.rope_pos(got[GR:GR + rows], cos, sin, pos.to(dev), rows=rows, H=Hq, head_dim=HD)
    want = body.to(torch.bfloat16).clone()
    cc, sc = cos.cpu(), sin.cpu()
    for r in range(rows):
        rope_(want[r:r + 1], cc, sc, 1, 1, Hq, HD, int(pos[r]))
    torch.cuda.synchronize()
    gc = got.cpu()
    _guards_intact(got, "rope_pos")
    assert torch.equal(gc[GR:GR + rows].view(torch.int16), want.view(torch.int16)), "rope_pos differs from the host restatement"
    gb, wb = _guarded(body, dev), _guarded(body, dev)
    T.rope_pos_backward(gb[GR:GR + rows], cos, sin, pos.to(dev), rows=rows, H=Hq, head_dim=HD)
    for r in range(rows):
        T.rope_backward(wb[GR + r:GR + r + 1], cos, sin, B=1, S=1, H=Hq, head_dim=HD, pos0=int(pos[r]))
    torch.cuda.synchronize()
    assert torch.equal(gb.cpu().view(torch.int16), wb.cpu().view(torch.int16)), "rope_pos_backward differs from rope_backward row by row"
    assert bool((gc[GR:GR + rows, 2 * D:3 * D].float() == body[:, 2 * D:3 * D]).all()), "the v third changed"
