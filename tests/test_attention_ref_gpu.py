"""Every dispatch form of the attention kernels against the fp64 reference of tests/attn_ref64.py.

Forms (attention.hip / attention_bwd.hip):
  seq-nspN  whole-sequence forward attn_seq_kernel (Sq, Skv <= 320), each head split over N = 4 / 2 / 1 workgroups for
            B·H < 64 / < 128 / >= 128; its backward is the whole-sequence pair attn_bwd_dq_kernel / attn_bwd_dkv_kernel
  chunk     chunked online-softmax forward attn_fwd_kernel (64-row query tiles, 64-key chunks) and the chunked backward
            (KC = 256-row chunks) for Sq or Skv > 320
  decode    attn_decode_kernel: keys held in registers up to 320 cached keys ("resident"), streamed above ("stream")
Every output is checked per element with the bound derived in attn_ref64; lse separately. Masking is checked bit for
bit: the K / V rows a query must not see are overwritten with ±3e4 and nothing it computes may change.
"""
import pytest
import torch

from attn_ref64 import (C_DK, C_DQ, C_DV, C_O, FLOOR, assert_attn_close, assert_lse_close, backward, forward, peaked_q)
from conftest import rand_bf16
from oracle import restate as R

pytestmark = pytest.mark.gpu
P = R.Prec(True)
BIG = 3.0e4          # finite stand-in for "anything" in rows that must not be read


def _mask(B, Skv, lens, holes=()):
    if lens is None:
        return None
    m = torch.zeros(B, Skv, dtype=torch.uint8)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    for b, j in holes:
        m[b, j] = 0
    return m


def _valid_rows(B, Sq, lens):
    rows = torch.ones(B, Sq, dtype=torch.bool)
    if lens is not None:
        for b, n in enumerate(lens):
            rows[b, min(n, Sq):] = False
    return rows


def _dev(t, dev):
    return t.to(torch.bfloat16).contiguous().to(dev)


def _strides(t):
    B, H, S, hd = t.shape
    return (H * S * hd, S * hd, hd)


def _run(dev, q, k, v, mask, causal, do=None):
    """Kernel forward (ops.attention and train_ops.attention_lse, which must agree bit for bit) and, given dO, the
    backward. CPU float results: o, lse [B, H, Sq], and delta, dq, dk, dv."""
    from bridgelang_amd import ops
    from bridgelang_amd import train_ops as T
    B, H, Sq, hd = q.shape
    Skv = k.shape[2]
    Q, K, V = _dev(q, dev), _dev(k, dev), _dev(v, dev)
    o1 = torch.zeros(B, H, Sq, hd, dtype=torch.bfloat16, device=dev)
    o = torch.zeros_like(o1)
    pad = (Sq + 31) // 32 * 32
    lse = torch.full((B * H * pad,), float("nan"), device=dev)
    kw = dict(B=B, H=H, Sq=Sq, Skv=Skv, head_dim=hd, q_strides=_strides(Q), k_strides=_strides(K), v_strides=_strides(V),
              o_strides=_strides(o), causal=causal, key_mask=None if mask is None else mask.to(dev))
    ops.attention(Q, K, V, o1, **kw)
    T.attention_lse(Q, K, V, o, lse, **kw)
    out = dict(o=o.cpu().float(), lse=lse.cpu().view(B, H, pad)[:, :, :Sq].clone())
    assert torch.equal(o1.cpu().view(torch.int16), o.cpu().view(torch.int16)), "ops.attention != train_ops.attention_lse"
    if do is not None:
        G = _dev(do, dev)
        delta = torch.full((B * H * pad,), float("nan"), device=dev)
        dq, dk, dv = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
        T.attention_backward(Q, K, V, o, G, lse, delta, dq, dk, dv, **kw)
        out.update(delta=delta.cpu().view(B, H, pad)[:, :, :Sq].clone(), dq=dq.cpu().float(), dk=dk.cpu().float(),
                   dv=dv.cpu().float())
    torch.cuda.synchronize()
    return out


def _perturbed(k, v, mask, causal, Sq, seed):
    """K / V with every row no compared query may see set to ±BIG: masked keys, and for causal runs the keys from
    t = off + Sq // 2 + 5 on. Returns k', v', the perturbed-key set [B, Skv] and the query rows whose inputs are
    unchanged ([B, Sq]: i + off < t)."""
    B, H, Skv, hd = k.shape
    off = Skv - Sq
    pert = torch.zeros(B, Skv, dtype=torch.bool)
    if mask is not None:
        pert |= mask == 0
    rows = torch.ones(B, Sq, dtype=torch.bool)
    t = off + Sq // 2 + 5
    if causal and t < Skv:
        pert[:, t:] = True
        rows[:, Sq // 2 + 5:] = False
    g = torch.Generator().manual_seed(seed)
    sk = (torch.randint(0, 2, k.shape, generator=g) * 2 - 1).float() * BIG
    sv = (torch.randint(0, 2, v.shape, generator=g) * 2 - 1).float() * BIG
    sel = pert.view(B, 1, Skv, 1)
    return torch.where(sel, sk, k), torch.where(sel, sv, v), pert, rows


def _assert_rows_equal(a, b, rows, what):
    sel = rows.view(rows.shape[0], 1, rows.shape[1], *([1] * (a.dim() - 3))).expand_as(a)
    assert torch.equal(a[sel], b[sel]), f"{what}: changed when rows that must not be read were overwritten"


# ---- forward + lse ----------------------------------------------------------------------------------------------------
# id: (B, H, Sq, Skv, hd, causal, key lengths or None, peaked)
FWD = {
    "seq-nsp4-hd64-S257-vit": (2, 4, 257, 257, 64, False, None, False),
    "seq-nsp4-hd72-S256-vit-peaked": (2, 3, 256, 256, 72, False, None, True),
    "seq-nsp4-hd128-causal-S1": (2, 2, 1, 1, 128, True, None, False),
    "seq-nsp4-hd64-S17-mask": (3, 2, 17, 17, 64, False, [17, 9, 1], False),
    "seq-nsp4-hd72-BH63-S261": (7, 9, 261, 261, 72, False, None, False),
    "seq-nsp2-hd64-BH64-S257": (4, 16, 257, 257, 64, False, None, False),
    "seq-nsp2-hd128-causal-BH127-S296": (1, 127, 296, 296, 128, True, None, False),
    "seq-nsp1-hd128-causal-BH128-S296-mask": (4, 32, 296, 296, 128, True, [296, 257, 65, 64], False),
    "seq-nsp1-hd72-BH128-S256-vit": (8, 16, 256, 256, 72, False, None, False),
    "seq-nsp4-hd128-causal-S319-mask-peaked": (2, 4, 319, 319, 128, True, [319, 63], True),
    "seq-nsp4-hd128-causal-S320-mask": (4, 2, 320, 320, 128, True, [320, 319, 64, 63], False),
    "seq-nsp4-hd64-S320-peaked": (2, 2, 320, 320, 64, False, None, True),
    "seq-nsp4-hd128-causal-Sq17-Skv300": (2, 2, 17, 300, 128, True, [300, 257], False),
    "chunk-hd128-causal-S321-mask-peaked": (2, 2, 321, 321, 128, True, [321, 65], True),
    "chunk-hd72-S321-mask": (2, 2, 321, 321, 72, False, [321, 320], False),
    "chunk-hd64-S352-mask": (4, 2, 352, 352, 64, False, [321, 257, 256, 65], False),
    "chunk-hd128-causal-S2048-peaked": (1, 2, 2048, 2048, 128, True, None, True),
    "chunk-hd64-S2048-mask": (1, 2, 2048, 2048, 64, False, [1999], False),
    "chunk-hd128-causal-Sq100-Skv700-mask": (2, 2, 100, 700, 128, True, [700, 641], False),
    "chunk-hd128-causal-Sq300-Skv321-peaked": (1, 2, 300, 321, 128, True, None, True),
}


@pytest.mark.parametrize("case", list(FWD))
def test_forward_and_lse(dev, case):
    B, H, Sq, Skv, hd, causal, lens, peaked = FWD[case]
    seed = 100 + list(FWD).index(case)
    q, k, v = rand_bf16((B, H, Sq, hd), seed), rand_bf16((B, H, Skv, hd), seed + 1), rand_bf16((B, H, Skv, hd), seed + 2)
    mask = _mask(B, Skv, lens)
    if peaked:
        q = peaked_q(q, k, causal, mask)
    rows = _valid_rows(B, Sq, None if lens is None or Sq != Skv else lens)
    got = _run(dev, q, k, v, mask, causal)
    ref = forward(q, k, v, hd ** -0.5, causal, mask)
    assert_attn_close(got["o"], ref["o"], ref["m_o"], C_O, f"fwd O {case}", rows)
    assert_lse_close(got["lse"], ref["lse2"], ref["mag_s"], f"fwd lse {case}", rows)
    # masking invariance: rows that must not be read hold ±3e4; every compared row stays bit-identical
    if mask is not None or causal:
        k2, v2, _, keep = _perturbed(k, v, mask, causal, Sq, seed + 3)
        got2 = _run(dev, q, k2, v2, mask, causal)
        _assert_rows_equal(got["o"], got2["o"], rows & keep, f"fwd O {case}")
        _assert_rows_equal(got["lse"], got2["lse"], rows & keep, f"fwd lse {case}")


# ---- backward -------------------------------------------------------------------------------------------------------
BWD = {
    "bwd-seq-nsp1-hd128-causal-BH128-S296-mask": (4, 32, 296, 296, 128, True, [296, 257, 65, 64], False),
    "bwd-seq-hd64-S257-vit": (2, 4, 257, 257, 64, False, None, False),
    "bwd-seq-hd72-S256-vit-peaked": (2, 3, 256, 256, 72, False, None, True),
    "bwd-seq-hd128-causal-S320-mask-peaked": (2, 2, 320, 320, 128, True, [320, 319], True),
    "bwd-seq-hd128-causal-Sq17-Skv300-mask": (2, 2, 17, 300, 128, True, [300, 257], False),
    "bwd-chunk-hd128-causal-S321-mask-peaked": (2, 2, 321, 321, 128, True, [321, 65], True),
    "bwd-chunk-hd64-S512-mask": (2, 2, 512, 512, 64, False, [512, 257], False),
    "bwd-chunk-hd128-causal-S513-mask": (2, 2, 513, 513, 128, True, [513, 256], False),
    "bwd-chunk-hd72-S513": (1, 2, 513, 513, 72, False, None, False),
    "bwd-chunk-hd128-causal-S1030": (1, 2, 1030, 1030, 128, True, None, False),
    "bwd-chunk-hd128-causal-S2048-peaked": (1, 2, 2048, 2048, 128, True, None, True),
    "bwd-chunk-hd128-causal-Sq100-Skv700-mask": (2, 2, 100, 700, 128, True, [700, 641], False),
}


@pytest.mark.parametrize("case", list(BWD))
def test_backward(dev, case):
    B, H, Sq, Skv, hd, causal, lens, peaked = BWD[case]
    seed = 300 + list(BWD).index(case)
    scale = hd ** -0.5
    q, k, v = rand_bf16((B, H, Sq, hd), seed), rand_bf16((B, H, Skv, hd), seed + 1), rand_bf16((B, H, Skv, hd), seed + 2)
    mask = _mask(B, Skv, lens)
    if peaked:
        q = peaked_q(q, k, causal, mask)
    rows = _valid_rows(B, Sq, None if lens is None or Sq != Skv else lens)
    do = rand_bf16((B, H, Sq, hd), seed + 4) * rows.view(B, 1, Sq, 1)      # padded query rows carry no gradient
    got = _run(dev, q, k, v, mask, causal, do)
    ref = backward(q, k, v, got["o"], do, scale, causal, mask)
    assert_attn_close(got["dq"], ref["dq"], ref["m_dq"], C_DQ, f"bwd dQ {case}", rows)
    assert_attn_close(got["dk"], ref["dk"], ref["m_dk"], C_DK, f"bwd dK {case}")
    assert_attn_close(got["dv"], ref["dv"], ref["m_dv"], C_DV, f"bwd dV {case}")
    # delta = rowsum(dO ∘ O) over the bf16 O: a 1-row fp32 dot of exact products
    dmag = (do.double() * got["o"].double()).abs().sum(-1)
    derr = (got["delta"].double() - ref["delta"]).abs()
    assert bool((derr[rows.view(B, 1, Sq).expand_as(derr)] <= (2.0 ** -16 * dmag + FLOOR)[rows.view(B, 1, Sq).expand_as(derr)]).all()), \
        f"{case}: delta differs from rowsum(dO * O) by {derr.max().item():.3g}"
    if mask is not None:     # masked keys: exactly zero dK and dV
        dead = (mask == 0).view(B, 1, Skv, 1).expand_as(got["dk"])
        assert bool((got["dk"][dead] == 0).all()) and bool((got["dv"][dead] == 0).all()), f"{case}: masked keys got gradient"
    # masking invariance: query rows that see a perturbed key get dO = 0 in both runs, so dK / dV of the untouched keys,
    # and dQ / delta / lse of the untouched rows, must be bit-identical
    if mask is not None or causal:
        k2, v2, pert, keep = _perturbed(k, v, mask, causal, Sq, seed + 3)
        do_k = do * (rows & keep).view(B, 1, Sq, 1)
        base = got if bool(keep.all()) else _run(dev, q, k, v, mask, causal, do_k)
        got2 = _run(dev, q, k2, v2, mask, causal, do_k)
        for t in ("dq", "delta", "lse", "o"):
            _assert_rows_equal(base[t], got2[t], rows & keep, f"bwd {t} {case}")
        for t in ("dk", "dv"):
            _assert_rows_equal(base[t], got2[t], ~pert, f"bwd {t} {case}")
        if mask is not None:
            dead = (mask == 0).view(B, 1, Skv, 1).expand_as(got2["dk"])
            assert bool((got2["dk"][dead] == 0).all()) and bool((got2["dv"][dead] == 0).all()), \
                f"{case}: masked keys holding ±3e4 got gradient"


@pytest.mark.parametrize("case", ["masked-key-zero-grad-seq-hd128-causal-S296", "masked-key-zero-grad-chunk-hd64-S700"])
def test_masked_keys_get_zero_gradient(dev, case):
    """Keys masked INSIDE the visible range (holes on tile and chunk edges, not only a padded tail) get exactly zero dK
    and dV, hold ±3e4 without changing anything else, and the rest matches the fp64 reference."""
    causal, S, hd = (True, 296, 128) if "seq" in case else (False, 700, 64)
    B, H = 2, 2
    holes = [(0, j) for j in (0, 15, 16, 63, 64, 65) if j < S] + [(1, j) for j in (31, 255, 256, 257, 319) if j < S]
    mask = _mask(B, S, [S, S - 10], holes)
    q, k, v, do = (rand_bf16((B, H, S, hd), 520 + i) for i in range(4))
    do = do * _valid_rows(B, S, [S, S - 10]).view(B, 1, S, 1)
    got = _run(dev, q, k, v, mask, causal, do)
    k2, v2, pert, _ = _perturbed(k, v, mask, False, S, 530)
    got2 = _run(dev, q, k2, v2, mask, causal, do)
    dead = (mask == 0).view(B, 1, S, 1).expand_as(got["dk"])
    for g in (got, got2):
        assert bool((g["dk"][dead] == 0).all()) and bool((g["dv"][dead] == 0).all()), f"{case}: masked keys got gradient"
    rows = _valid_rows(B, S, [S, S - 10])
    for t in ("o", "lse", "dq", "delta"):
        _assert_rows_equal(got[t], got2[t], rows, f"{case} {t}")
    for t in ("dk", "dv"):
        _assert_rows_equal(got[t], got2[t], ~pert, f"{case} {t}")
    rb = backward(q, k, v, got["o"], do, hd ** -0.5, causal, mask)
    for t, c in (("dq", C_DQ), ("dk", C_DK), ("dv", C_DV)):
        assert_attn_close(got[t], rb[t], rb["m_" + t], c, f"bwd {t} {case}", rows if t == "dq" else None)


# ---- empty rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["empty-rows-seq-hd128-causal-S100", "empty-rows-chunk-hd64-S400"])
def test_empty_rows(dev, case):
    """A batch element whose keys are all masked: o = 0, lse = +inf, zero gradients; the others finite and correct."""
    causal, S, hd = (True, 100, 128) if "seq" in case else (False, 400, 64)
    B, H = 2, 2
    q, k, v, do = (rand_bf16((B, H, S, hd), 500 + i) for i in range(4))
    mask = _mask(B, S, [S, 0])
    got = _run(dev, q, k, v, mask, causal, do)
    assert bool((got["o"][1] == 0).all()), "empty rows: o != 0"
    assert bool(torch.isposinf(got["lse"][1]).all()), "empty rows: lse != +inf"
    for t in ("dq", "dk", "dv", "delta"):
        assert bool((got[t][1] == 0).all()), f"empty rows: {t} != 0"
        assert bool(torch.isfinite(got[t][0]).all()), f"{t} of the non-empty batch element is not finite"
    ref = forward(q, k, v, hd ** -0.5, causal, mask)
    rb = backward(q, k, v, got["o"], do, hd ** -0.5, causal, mask)
    assert_attn_close(got["o"], ref["o"], ref["m_o"], C_O, f"fwd O {case}")
    assert_lse_close(got["lse"], ref["lse2"], ref["mag_s"], f"fwd lse {case}")
    for t, c in (("dq", C_DQ), ("dk", C_DK), ("dv", C_DV)):
        assert_attn_close(got[t], rb[t], rb["m_" + t], c, f"bwd {t} {case}")


# ---- decode -------------------------------------------------------------------------------------------------------------
DEC_B, DEC_H, HD = 2, 4, 128


def _decode_ref_rope(qkv, kc, vc, cos, sin, pos, mask=None):
    """fp64 reference of one decode step with RoPE and the cache append at `pos`: rotated q / k (the oracle's
    apply_rope, bit-exact bf16 arithmetic), keys 0..pos = cache rows 0..pos-1 and the new key."""
    B, H = qkv.shape[0], DEC_H
    D = H * HD
    t = qkv.view(B, 3, H, 1, HD)
    qr = R.apply_rope(P, t[:, 0], cos, sin, pos)
    kr = R.apply_rope(P, t[:, 1], cos, sin, pos)
    K = torch.cat([kc[:, :, :pos], kr], dim=2)
    V = torch.cat([vc[:, :, :pos], t[:, 2]], dim=2)
    f = forward(qr, K, V, HD ** -0.5, False, None if mask is None else mask[:, :pos + 1])
    return f, kr, t[:, 2]


@pytest.mark.parametrize("Skv,masked", [pytest.param(n, m, id=f"decode-{'resident' if n <= 320 else 'stream'}-Skv{n}-"
                                                    f"{'mask' if m else 'nomask'}")
                                       for n in (1, 64, 65, 320, 321, 385, 1024, 2048) for m in (False, True)])
def test_decode(dev, Skv, masked):
    """ops.attention_decode over a 2048-row cache: keys resident in registers up to 320, streamed above (decode-stream)."""
    from bridgelang_amd import ops
    B, H, cache_len = DEC_B, DEC_H, 2048
    D = H * HD
    form = "resident" if Skv <= 320 else "stream"
    q = rand_bf16((B, H, 1, HD), 600 + Skv)
    kc, vc = rand_bf16((B, H, cache_len, HD), 601), rand_bf16((B, H, cache_len, HD), 602)
    mask = None
    if masked:     # batch 1: a ragged tail and a hole (batch 1 at Skv = 1: an empty row)
        mask = torch.ones(B, cache_len, dtype=torch.uint8)
        mask[1, max(0, Skv - 37):] = 0
        mask[1, Skv // 2] = 0

    def run(kc_, vc_):
        o = torch.zeros(B, D, dtype=torch.bfloat16, device=dev)
        cs = (H * cache_len * HD, cache_len * HD, HD)
        ops.attention_decode(_dev(q, dev).view(B, D), _dev(kc_, dev), _dev(vc_, dev), o, B=B, H=H, Skv=Skv, head_dim=HD,
                             q_strides=(D, HD, D), k_strides=cs, v_strides=cs, o_strides=(D, HD, D),
                             key_mask=None if mask is None else mask.to(dev))
        return o.cpu().float().view(B, H, 1, HD)

    got = run(kc, vc)
    ref = forward(q, kc[:, :, :Skv], vc[:, :, :Skv], HD ** -0.5, False, None if mask is None else mask[:, :Skv])
    assert_attn_close(got, ref["o"], ref["m_o"], C_O, f"decode O decode-{form}-Skv{Skv}-{'mask' if masked else 'nomask'}")
    if masked:
        k2, v2, _, _ = _perturbed(kc, vc, mask, False, 1, 603)
        assert torch.equal(run(k2, v2), got), f"decode-{form}-Skv{Skv}: masked cache rows changed the output"


def _rope_tables(dev):
    cos, sin = R.rope_tables(HD, 2048, 10000.0)
    return cos, sin, _dev(cos, dev), _dev(sin, dev)


@pytest.mark.parametrize("pos", [319, 320, 321, 2047], ids=lambda p: f"decode-rope-{'resident' if p <= 320 else 'stream'}-pos{p}")
def test_decode_rope(dev, pos):
    """ops.attention_decode_rope: n_cache = pos cached keys plus the new one; 320 is the last resident case."""
    from bridgelang_amd import ops
    B, H, cache_len = DEC_B, DEC_H, 2048
    D = H * HD
    cos, sin, C_, S_ = _rope_tables(dev)
    qkv = rand_bf16((B, 3 * D), 700 + pos)
    kc, vc = rand_bf16((B, H, cache_len, HD), 701), rand_bf16((B, H, cache_len, HD), 702)
    Kc, Vc = _dev(kc, dev), _dev(vc, dev)
    o = torch.zeros(B, D, dtype=torch.bfloat16, device=dev)
    ops.attention_decode_rope(_dev(qkv, dev), Kc, Vc, o, C_, S_, B=B, H=H, head_dim=HD, pos=pos)
    ref, kr, vn = _decode_ref_rope(qkv, kc, vc, cos, sin, pos)
    assert_attn_close(o.cpu().float().view(B, H, 1, HD), ref["o"], ref["m_o"], C_O, f"decode O decode-rope-pos{pos}")
    k_exp, v_exp = kc.clone(), vc.clone()
    k_exp[:, :, pos:pos + 1], v_exp[:, :, pos:pos + 1] = kr, vn
    assert torch.equal(Kc.cpu().float(), k_exp), "k cache: appended row != apply_rope, or another row changed"
    assert torch.equal(Vc.cpu().float(), v_exp), "v cache: appended row != v, or another row changed"


@pytest.mark.parametrize("masked", [False, True], ids=["decode-rope_pos-nomask", "decode-rope_pos-cache_mask"])
def test_decode_rope_pos(dev, masked):
    """bl_attention_decode_rope_pos_bf16 (right-padded batch, engine.py decode): sequence b rotates at, appends at and
    attends up to its own position rope_pos[b]; positions straddle 320 in one launch. With the engine's cache_mask
    layout ([B, cache_len], prompt-pad columns off) as the key mask in the masked variant."""
    from bridgelang_amd import ops
    B, H, cache_len = 4, DEC_H, 1024
    D = H * HD
    rp = [318, 320, 321, 700]
    pos = max(rp)
    cos, sin, C_, S_ = _rope_tables(dev)
    qkv = rand_bf16((B, 3 * D), 800)
    kc, vc = rand_bf16((B, H, cache_len, HD), 801), rand_bf16((B, H, cache_len, HD), 802)
    mask = None
    if masked:
        mask = torch.ones(B, cache_len, dtype=torch.uint8)
        for b in range(B):
            mask[b, 200 + 3 * b:230] = 0          # pad columns of a right-padded prompt, below every position
    Kc, Vc = _dev(kc, dev), _dev(vc, dev)
    o = torch.zeros(B, D, dtype=torch.bfloat16, device=dev)
    ops.attention_decode_rope(_dev(qkv, dev), Kc, Vc, o, C_, S_, B=B, H=H, head_dim=HD, pos=pos,
                              rope_pos=torch.tensor(rp, dtype=torch.int32, device=dev),
                              key_mask=None if mask is None else mask.to(dev))
    got = o.cpu().float().view(B, H, 1, HD)
    k_exp, v_exp = kc.clone(), vc.clone()
    for b in range(B):
        ref, kr, vn = _decode_ref_rope(qkv[b:b + 1], kc[b:b + 1], vc[b:b + 1], cos, sin, rp[b],
                                       None if mask is None else mask[b:b + 1])
        assert_attn_close(got[b:b + 1], ref["o"], ref["m_o"], C_O, f"decode O decode-rope_pos-seq{b}-pos{rp[b]}")
        k_exp[b, :, rp[b]], v_exp[b, :, rp[b]] = kr[0, :, 0], vn[0, :, 0]
    assert torch.equal(Kc.cpu().float(), k_exp), "k cache: a row other than each sequence's own position changed"
    assert torch.equal(Vc.cpu().float(), v_exp), "v cache: a row other than each sequence's own position changed"


def test_decode_rope_grouped_straddles_320(dev):
    """ops.attention_decode_rope_grouped: groups on both sides of the resident / streaming edge in one launch, each
    against its own fp64 reference and cache append."""
    from bridgelang_amd import ops
    B, H, cache_len = DEC_B, DEC_H, 1024
    D = H * HD
    pos = [318, 320, 321, 700]
    G = len(pos)
    cos, sin, C_, S_ = _rope_tables(dev)
    qkv = rand_bf16((G * B, 3 * D), 900)
    kc = [rand_bf16((B, H, cache_len, HD), 910 + g) for g in range(G)]
    vc = [rand_bf16((B, H, cache_len, HD), 920 + g) for g in range(G)]
    Kc, Vc = [_dev(t, dev) for t in kc], [_dev(t, dev) for t in vc]
    o = torch.zeros(G * B, D, dtype=torch.bfloat16, device=dev)
    ops.attention_decode_rope_grouped(_dev(qkv, dev), Kc, Vc, o, C_, S_, B=B, H=H, head_dim=HD, pos=pos)
    got = o.cpu().float().view(G * B, H, 1, HD)
    for g in range(G):
        r = slice(g * B, (g + 1) * B)
        ref, kr, vn = _decode_ref_rope(qkv[r], kc[g], vc[g], cos, sin, pos[g])
        assert_attn_close(got[r], ref["o"], ref["m_o"], C_O, f"decode O decode-grouped-g{g}-pos{pos[g]}")
        k_exp, v_exp = kc[g].clone(), vc[g].clone()
        k_exp[:, :, pos[g]:pos[g] + 1], v_exp[:, :, pos[g]:pos[g] + 1] = kr, vn
        assert torch.equal(Kc[g].cpu().float(), k_exp) and torch.equal(Vc[g].cpu().float(), v_exp), f"group {g}: caches"
