"""bl_attention_probs_f32 (csrc/attention_probs.hip) against its fp64 definition, bridgelang_amd/attention_taps.py.

Reference: q is rotated on the host with oracle.restate.apply_rope (the three bf16 roundings the kernel's rope_pair makes),
then attention_taps.probs_reference runs the fp64 softmax over the cached (rotated) K.

Bound, per element of P:   |got − ref| <= C_P·u·ref + FLOOR,   C_P = 0.25, u = 2^-8, FLOOR = 2^-110.
It is the forward model of tests/attn_ref64.py with the dominant term taken out, because this kernel does NOT round P to bf16:
  * fp32 scores: a 128-term fp32 accumulation of exact bf16 products and the multiply by fp32(scale·log2e) move s' by at most
    ~130·2^-24·|s'| <= 2^-10.9 for |s'| <= 64, i.e. <= 0.09u relative in exp2(s' − m); it enters P through the numerator and
    through the denominator: 0.18u.
  * v_exp_f32 (1 ulp), the fp32 row sum of <= 2048 terms (n·2^-24 <= 2^-13 = 0.03u) and the fp32 reciprocal and multiply
    (2 roundings): together < 0.07u.
Sum 0.25. FLOOR is attn_ref64's: an exp2 result below 2^-126 may be flushed to zero. The model's precondition |s'| <= 64 is
asserted on the fp64 scores of every case. Further: every row with a visible key sums to 1 within 2^-9 (2048 elements each
off by <= 0.25u·P sum to <= 2^-10), and seg equals the fp64 sum of the RETURNED P over the segment within n·2^-24·sum + FLOOR
(n = segment length: at most n − 1 fp32 additions of non-negative terms, each rounding <= 2^-24 of the running sum).
These constants are final: a GPU run that exceeds one is a finding about the kernel, not a reason to widen it.
"""
import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from attn_ref64 import LOG2E, peaked_q  # noqa: E402
from conftest import rand_bf16  # noqa: E402

from bridgelang_amd import attention_taps as T  # noqa: E402
from oracle import restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

U, FLOOR, C_P = 2.0 ** -8, 2.0 ** -110, 0.25
HD = 128
SCALE = HD ** -0.5
MAX_POS = 512
SENT = 777.0
_COS, _SIN = R.rope_tables(HD, MAX_POS, 10000.0)       # fp32 tensors of bf16 values [MAX_POS, 64]


def _rotate(q, pos):
    """q [B, H, Sq, 128] (bf16 values) rotated at positions pos[b] + row."""
    return torch.cat([R.apply_rope(R.Prec(), q[b:b + 1], _COS, _SIN, int(pos[b])) for b in range(q.shape[0])], dim=0)


def _masks(kind, B, Sq, Skv):
    if kind is None:
        return None
    m = torch.ones(B, Skv, dtype=torch.uint8)
    if kind == "pad_hole":            # sequence 0 right-padded, the last sequence with a hole
        m[0, Skv - 15:] = 0
        m[B - 1, 100:120] = 0
        if B > 1:
            m[B - 1, Skv - 7:] = 0
    elif kind == "empty_row":         # sequence 0 right-padded; the last hides every key its first query row could see
        m[0, Skv - 25:] = 0
        m[B - 1, :Skv - Sq + 1] = 0
    return m


class Case:
    """One launch's inputs on the host, its fp64 reference, and the device buffers (with sentinels around the outputs)."""

    def __init__(self, dev, B, H, Sq, Skv, causal, seed, mask=None, form="rotated", pos=None, layout="compact", extra_cols=0,
                 peaked=False, nan_fill=True, bounds=None):
        self.dev, self.B, self.H, self.Sq, self.Skv, self.causal, self.form = dev, B, H, Sq, Skv, causal, form
        D = H * HD
        q = rand_bf16((B, H, Sq, HD), seed)
        k = rand_bf16((B, H, Skv, HD), seed + 1)
        self.mask = _masks(mask, B, Sq, Skv)
        self.pos = [0] * B if pos is None else ([pos] * B if isinstance(pos, int) else list(pos))
        if form == "rotated":
            if peaked:
                q = peaked_q(q, k, causal, self.mask)
            q_mem, q_rot = q, q
        else:
            q_mem, q_rot = q, _rotate(q, self.pos)
        self.k_host, self.q_rot = k, q_rot
        s2 = (SCALE * LOG2E) * (q_rot.double() @ k.double().transpose(-1, -2))
        self.smax = float(s2.abs().max())
        self.ref = T.probs_reference(q_rot, k, SCALE, causal, self.mask)

        # q in memory: compact [B, H, Sq, 128] or the q third of fused qkv rows [B*Sq, 3D]
        if layout == "fused":
            buf = rand_bf16((B * Sq, 3 * D), seed + 2)
            buf[:, :D] = q_mem.permute(0, 2, 1, 3).reshape(B * Sq, D)
            self.q_dev, self.q_strides = buf.to(torch.bfloat16).to(dev), (Sq * 3 * D, HD, 3 * D)
        else:
            self.q_dev, self.q_strides = q_mem.to(torch.bfloat16).contiguous().to(dev), (H * Sq * HD, Sq * HD, HD)
        # K as a cache view: rows >= Skv, and the rows of masked keys, hold NaN
        self.cache_len = (Skv + 1 + 63) // 64 * 64
        cache = torch.full((B, H, self.cache_len, HD), float("nan") if nan_fill else 0.0)
        cache[:, :, :Skv] = k
        if self.mask is not None and nan_fill:
            for b in range(B):
                cache[b][:, (self.mask[b] == 0).nonzero().flatten()] = float("nan")
        self.k_dev = cache.to(torch.bfloat16).to(dev)
        self.k_strides = (H * self.cache_len * HD, self.cache_len * HD, HD)
        self.mask_dev = None if self.mask is None else self.mask.to(dev)
        self.cos, self.sin = _COS.to(torch.bfloat16).to(dev), _SIN.to(torch.bfloat16).to(dev)
        self.rope_pos = None
        if form == "rope_pos":
            self.rope_pos = torch.tensor(self.pos, dtype=torch.int32, device=dev)
        # outputs between sentinels
        self.p_cols = Skv + extra_cols
        self.p_buf = torch.full((B, H, Sq, self.p_cols + 8), SENT, dtype=torch.float32, device=dev)
        self.probs = self.p_buf[..., 4:4 + self.p_cols]
        if bounds is None:
            cuts = sorted({0, 1, Skv // 3, Skv // 3, (2 * Skv) // 3, Skv - 1, Skv + 5})
            bounds = [cuts[:] for _ in range(B)]
            bounds[-1] = [min(c + 1, Skv + 9) for c in cuts]
        self.bounds = torch.tensor(bounds, dtype=torch.int32)
        self.n_seg = self.bounds.shape[1] - 1
        self.bounds_dev = self.bounds.to(dev)
        n = B * H * Sq * self.n_seg
        self.s_buf = torch.full((n + 16,), SENT, dtype=torch.float32, device=dev)
        self.seg = self.s_buf[8:8 + n].view(B, H, Sq, self.n_seg)

    def op(self, probs=True, seg=True, **over):
        from bridgelang_amd import ops
        kw = dict(B=self.B, H=self.H, Sq=self.Sq, Skv=self.Skv, head_dim=HD, q_strides=self.q_strides, k_strides=self.k_strides,
                  causal=self.causal, scale=SCALE, key_mask=self.mask_dev, probs=self.probs if probs else None,
                  seg=self.seg if seg else None, seg_bounds=self.bounds_dev if seg else None, run=False)
        if self.form != "rotated":
            kw.update(cos=self.cos, sin=self.sin, pos0=self.pos[0], rope_pos=self.rope_pos)
        kw.update(over)
        return ops.attention_probs(self.q_dev, self.k_dev, **kw)

    def reset(self):
        self.p_buf.fill_(SENT)
        self.s_buf.fill_(SENT)

    def check_canaries(self, probs=True, seg=True):
        pb, sb = self.p_buf.cpu(), self.s_buf.cpu()
        assert bool((pb[..., :4] == SENT).all()) and bool((pb[..., 4 + self.p_cols:] == SENT).all()), "probs: wrote outside [0, p_cols)"
        assert bool((sb[:8] == SENT).all()) and bool((sb[-8:] == SENT).all()), "seg: wrote outside the tensor"
        if not probs:
            assert bool((pb == SENT).all())
        if not seg:
            assert bool((sb == SENT).all())

    def check(self, what):
        assert self.smax <= 64.0, f"{what}: the error model's precondition |s'| <= 64 does not hold ({self.smax:.1f})"
        got = self.probs.cpu().double()
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite P"
        P, tail = got[..., :self.Skv], got[..., self.Skv:]
        assert bool((tail == 0).all()), f"{what}: columns [Skv, p_cols) must be 0"
        assert bool((P[self.ref == 0] == 0).all()), f"{what}: a hidden key got weight"
        err, bound = (P - self.ref).abs(), C_P * U * self.ref + FLOOR
        ratio = float((err / bound).max())
        vis_rows = self.ref.sum(-1) > 0
        rowsum = float((P.sum(-1) - 1.0).abs()[vis_rows].max()) if bool(vis_rows.any()) else 0.0
        print(f"attention_probs: {what}: max err/bound {ratio:.4f}, max |s'| {self.smax:.1f}, max |rowsum - 1| {rowsum:.3g} "
              f"({int((~vis_rows).sum())} empty rows)")
        assert ratio <= 1.0, f"{what}: P out of bound, err/bound {ratio:.3g}"
        assert rowsum <= 2.0 ** -9, f"{what}: a row sums to 1 ± {rowsum:.3g}"
        assert bool((P[~vis_rows] == 0).all())
        self.check_seg(what, P)

    def check_seg(self, what, P):
        seg = self.seg.cpu().double()
        assert bool(torch.isfinite(seg).all()), f"{what}: non-finite seg"
        ref = T.segment_sums(P, self.bounds)
        b = self.bounds.clamp(0, self.Skv).to(torch.float64)
        n = (b[:, 1:] - b[:, :-1]).clamp(min=0).view(self.B, 1, 1, self.n_seg)
        bound = n * 2.0 ** -24 * ref + FLOOR
        ratio = float(((seg - ref).abs() / bound).max())
        print(f"attention_probs: {what}: seg max err/bound {ratio:.4f}")
        assert ratio <= 1.0, f"{what}: seg out of bound, err/bound {ratio:.3g}"


def _run(case, what, **kw):
    case.reset()
    case.op(**kw).run()
    torch.cuda.synchronize()
    case.check_canaries()
    case.check(what)


CASES = [
    # B, H, Sq, Skv, causal, mask, form, pos, layout, extra_cols, peaked
    ("one_key", 2, 3, 1, 1, False, None, "rotated", None, "compact", 0, False),
    ("one_key_fused", 2, 3, 1, 1, False, None, "pos0", 263, "fused", 3, False),
    ("decode_37", 1, 2, 1, 37, False, None, "pos0", 263, "fused", 3, False),
    ("decode_37_rot", 1, 2, 1, 37, False, None, "rotated", None, "compact", 0, True),
    ("square_17", 2, 3, 17, 17, True, None, "pos0", 0, "fused", 0, False),
    ("square_17_rot", 2, 3, 17, 17, True, None, "rotated", None, "fused", 6, True),
    ("offset_39", 1, 2, 5, 44, True, None, "pos0", 39, "compact", 0, False),
    ("offset_39_rot", 1, 2, 5, 44, True, None, "rotated", None, "compact", 4, True),
    ("masked_295", 2, 4, 33, 295, True, "pad_hole", "rope_pos", (262, 100), "fused", 1, False),
    ("masked_295_rot", 2, 4, 33, 295, True, "pad_hole", "rotated", None, "compact", 0, True),
    ("empty_row_295", 2, 4, 33, 295, True, "empty_row", "rope_pos", (17, 262), "compact", 5, False),
    ("empty_row_295_rot", 2, 4, 33, 295, True, "empty_row", "rotated", None, "fused", 0, True),
    ("long_2048", 1, 1, 1, 2048, False, None, "rotated", None, "compact", 0, False),
    ("long_2048_peaked", 1, 1, 1, 2048, False, None, "rotated", None, "compact", 0, True),
]


@pytest.mark.parametrize("name,B,H,Sq,Skv,causal,mask,form,pos,layout,extra,peaked", CASES, ids=[c[0] for c in CASES])
def test_probs_and_segments(dev, name, B, H, Sq, Skv, causal, mask, form, pos, layout, extra, peaked):
    case = Case(dev, B, H, Sq, Skv, causal, seed=100 + len(name), mask=mask, form=form, pos=pos, layout=layout, extra_cols=extra,
                peaked=peaked)
    _run(case, name)
    both_p, both_s = case.probs.clone(), case.seg.clone()
    # probs only / seg only: the other tensor is untouched, the one asked for has the same bits
    case.reset()
    case.op(seg=False).run()
    torch.cuda.synchronize()
    case.check_canaries(seg=False)
    assert torch.equal(case.probs, both_p)
    case.reset()
    case.op(probs=False).run()
    torch.cuda.synchronize()
    case.check_canaries(probs=False)
    assert torch.equal(case.seg, both_s)
    if name == "empty_row_295":
        assert bool((both_p[B - 1, :, 0] == 0).all()) and bool((both_s[B - 1, :, 0] == 0).all())


@pytest.mark.parametrize("pos", [(0, 0), (263, 19)])
def test_rotation_on_load_is_bit_exact(dev, pos):
    """q rotated by the kernel equals q rotated on the host and read from memory, bit for bit (rope_pair = apply_rope)."""
    a = Case(dev, 2, 2, 19, 40, True, seed=7, form="rope_pos", pos=pos, layout="fused")
    a.op().run()
    b = Case(dev, 2, 2, 19, 40, True, seed=7, form="rotated", layout="compact")
    b.q_dev = a.q_rot.to(torch.bfloat16).contiguous().to(dev)
    b.op().run()
    torch.cuda.synchronize()
    assert torch.equal(a.probs, b.probs) and torch.equal(a.seg, b.seg)
    if pos[0] == pos[1]:       # one position for the batch: the pos0 argument does what the array does
        a.reset()
        a.op(rope_pos=None, pos0=pos[0]).run()
        torch.cuda.synchronize()
        assert torch.equal(a.probs, b.probs)


def test_rows_are_independent_of_the_launch(dev):
    """One Sq = 33 launch and 33 launches of Sq = 1 over the same rows agree bit for bit."""
    from bridgelang_amd import ops
    B, H, Sq, Skv = 2, 2, 33, 295
    c = Case(dev, B, H, Sq, Skv, True, seed=31, mask="pad_hole", form="pos0", pos=200, layout="fused")
    _run(c, "rows_full")
    D, off = H * HD, Skv - Sq
    p1 = torch.full((B, H, Sq, Skv), SENT, dtype=torch.float32, device=dev)
    s1 = torch.full((Sq, B, H, 1, c.n_seg), SENT, dtype=torch.float32, device=dev)
    q2 = c.q_dev.view(B, Sq, 3 * D)
    for i in range(Sq):
        ops.attention_probs(q2[:, i], c.k_dev, B=B, H=H, Sq=1, Skv=i + off + 1, head_dim=HD, q_strides=c.q_strides,
                            k_strides=c.k_strides, causal=False, scale=SCALE, key_mask=c.mask_dev, cos=c.cos, sin=c.sin,
                            pos0=200 + i, probs=p1[:, :, i:i + 1], seg=s1[i], seg_bounds=c.bounds_dev)
    torch.cuda.synchronize()
    assert torch.equal(p1, c.probs)
    assert torch.equal(s1.squeeze(3).permute(1, 2, 0, 3), c.seg)


def test_graph_replay_follows_mask_and_bounds(dev):
    """The op reads the mask and the bounds at run time and rewrites all of its outputs: a captured graph replayed after both
    were rewritten equals a fresh launch."""
    c = Case(dev, 2, 2, 1, 140, False, seed=41, mask="pad_hole", form="pos0", pos=139, layout="fused", extra_cols=52,
             nan_fill=False)                   # keys hidden now are shown later: their K rows hold real values
    op = c.op()
    op.run()                                   # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        op.run()
    c.mask_dev[:, 30:50] = 0
    c.mask_dev[:, 100:120] = 1
    c.bounds_dev.copy_(torch.tensor([[0, 5, 5, 80, 140, 140], [3, 10, 60, 61, 139, 200]], dtype=torch.int32))
    c.reset()
    g.replay()
    torch.cuda.synchronize()
    c.check_canaries()
    got_p, got_s = c.probs.clone(), c.seg.clone()
    c.reset()
    op.run()
    torch.cuda.synchronize()
    assert torch.equal(got_p, c.probs) and torch.equal(got_s, c.seg)
    assert bool((got_p[:, :, :, 30:50] == 0).all()) and bool(torch.isfinite(got_p).all())
    assert float((got_p.double().sum(-1) - 1).abs().max()) <= 2.0 ** -9


def _rc(op):
    return op.fn(*op.args, torch.cuda.current_stream().cuda_stream)


def test_rejections(dev):
    from bridgelang_amd import _lib, ops
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)
    # Skv = 2049
    q, k, p = z(1, 1, 1, HD), z(1, 1, 2112, HD), z(1, 1, 1, 2112, dt=torch.float32)
    kw = dict(B=1, H=1, Sq=1, head_dim=HD, q_strides=(HD, HD, HD), k_strides=(2112 * HD, 2112 * HD, HD), causal=False, run=False)
    assert _rc(ops.attention_probs(q, k, Skv=2049, probs=p, **kw)) == _lib.BL_E_SHAPE
    assert _rc(ops.attention_probs(q, k, Skv=2048, probs=p, **kw)) == _lib.BL_OK
    # head_dim 64
    kw64 = dict(kw, head_dim=64, q_strides=(64, 64, 64), k_strides=(2112 * 64, 2112 * 64, 64))
    assert _rc(ops.attention_probs(q, k, Skv=16, probs=p, **kw64)) == _lib.BL_E_SHAPE
    # an odd pointer (q moved by one bf16 element), a stride that is no multiple of 8
    q_odd = z(HD + 8)[1:1 + HD].view(1, 1, 1, HD)
    assert _rc(ops.attention_probs(q_odd, k, Skv=16, probs=p, **kw)) == _lib.BL_E_ALIGN
    assert _rc(ops.attention_probs(q, k, Skv=16, probs=p, **dict(kw, q_strides=(HD + 4, HD, HD)))) == _lib.BL_E_ALIGN
    # fewer columns than keys; no output at all
    assert _rc(ops.attention_probs(q, k, Skv=16, probs=p[..., :8], **kw)) == _lib.BL_E_SHAPE
    assert _rc(ops.attention_probs(q, k, Skv=16, **kw)) == _lib.BL_E_ARG
    torch.cuda.synchronize()
