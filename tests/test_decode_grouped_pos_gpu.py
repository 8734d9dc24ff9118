"""Grouped decode attention with per-sequence positions (bl_attention_decode_rope_pos_grouped_bf16, the merged decode
iteration of StaggeredDecodePipeline(padded=True)) and the row gather of the padded plan's last layer
(bl_gather_rows_bf16).

Group g carries a device array rope_pos[g][b]: sequence b of group g rotates at, appends at and attends up to its own
position. The positions below put both sides of the 320-key resident / streaming edge into one group, and cover position 0
(no cached key), the last cache row and the 64-key edges of the key loop. Every row is checked against its own fp64
reference with the bound of attn_ref64, the cache writes bit for bit, and the output bit for bit against the un-grouped
per-sequence form and the grouped one-position-per-group form."""
import pytest
import torch

from attn_ref64 import C_O, assert_attn_close
from conftest import rand_bf16
from test_attention_ref_gpu import DEC_H, HD, _decode_ref_rope, _dev, _rope_tables

pytestmark = pytest.mark.gpu

H, CACHE_LEN = DEC_H, 1024
D = H * HD
POS = [[318, 320, 321, 700], [0, 1, 63, 64], [319, 319, 319, 319], [65, 320, 2, 1023]]


def _inputs(G, B, seed):
    qkv = rand_bf16((G * B, 3 * D), seed)
    kc = [rand_bf16((B, H, CACHE_LEN, HD), seed + 10 + g) for g in range(G)]
    vc = [rand_bf16((B, H, CACHE_LEN, HD), seed + 20 + g) for g in range(G)]
    return qkv, kc, vc


def _run_grouped(dev, qkv, kc, vc, tables, B, **at):
    """One grouped launch on fresh device copies of the caches; returns (o, K caches, V caches) on the device."""
    from bridgelang_amd import ops
    Kc, Vc = [_dev(t, dev) for t in kc], [_dev(t, dev) for t in vc]
    o = torch.zeros(qkv.shape[0], D, dtype=torch.bfloat16, device=dev)
    ops.attention_decode_rope_grouped(_dev(qkv, dev), Kc, Vc, o, tables[2], tables[3], B=B, H=H, head_dim=HD, **at)
    return o, Kc, Vc


def _rp(pos, dev):
    return [torch.tensor(p, dtype=torch.int32, device=dev) for p in pos]


@pytest.fixture(scope="module")
def case(dev):
    """The G = 4, B = 4 launch every test below looks at, run once."""
    G, B = len(POS), len(POS[0])
    tables = _rope_tables(dev)
    qkv, kc, vc = _inputs(G, B, 1000)
    o, Kc, Vc = _run_grouped(dev, qkv, kc, vc, tables, B, rope_pos=_rp(POS, dev))
    return dict(G=G, B=B, tables=tables, qkv=qkv, kc=kc, vc=vc, o=o, Kc=Kc, Vc=Vc)


def test_rows_against_fp64_and_cache_writes(case):
    """Each (g, b) against its own fp64 reference at its own position; the caches change at row (g, b, pos) only, where
    they hold apply_rope(k) / v exactly."""
    G, B, (cos, sin, _, _) = case["G"], case["B"], case["tables"]
    got = case["o"].cpu().float().view(G * B, H, 1, HD)
    for g in range(G):
        k_exp, v_exp = case["kc"][g].clone(), case["vc"][g].clone()
        for b in range(B):
            r, pos = g * B + b, POS[g][b]
            ref, kr, vn = _decode_ref_rope(case["qkv"][r:r + 1], case["kc"][g][b:b + 1], case["vc"][g][b:b + 1], cos, sin, pos)
            assert_attn_close(got[r:r + 1], ref["o"], ref["m_o"], C_O, f"decode O decode-grouped_pos-g{g}-seq{b}-pos{pos}")
            k_exp[b, :, pos], v_exp[b, :, pos] = kr[0, :, 0], vn[0, :, 0]
        assert torch.equal(case["Kc"][g].cpu().float(), k_exp), f"group {g}: k cache row != apply_rope(k), or another row changed"
        assert torch.equal(case["Vc"][g].cpu().float(), v_exp), f"group {g}: v cache row != v, or another row changed"


def test_equals_ungrouped_per_sequence_form(dev, case):
    """Per group bit-identical to bl_attention_decode_rope_pos_bf16 on that group alone (fresh copies of its caches)."""
    from bridgelang_amd import ops
    B, (_, _, C_, S_) = case["B"], case["tables"]
    for g in range(case["G"]):
        r = slice(g * B, (g + 1) * B)
        Kc, Vc = _dev(case["kc"][g], dev), _dev(case["vc"][g], dev)
        o = torch.zeros(B, D, dtype=torch.bfloat16, device=dev)
        ops.attention_decode_rope(_dev(case["qkv"][r], dev), Kc, Vc, o, C_, S_, B=B, H=H, head_dim=HD, pos=max(POS[g]),
                                  rope_pos=torch.tensor(POS[g], dtype=torch.int32, device=dev))
        assert torch.equal(case["o"][r], o), f"group {g}: output differs from the un-grouped rope_pos form"
        assert torch.equal(case["Kc"][g], Kc) and torch.equal(case["Vc"][g], Vc), f"group {g}: caches differ"


def test_equal_positions_match_scalar_grouped_form(dev, case):
    """All positions of each group equal: bit-identical to the grouped form that takes one host position per group."""
    G, B = case["G"], case["B"]
    pos = [320, 0, 319, 1023]
    a = _run_grouped(dev, case["qkv"], case["kc"], case["vc"], case["tables"], B, rope_pos=_rp([[p] * B for p in pos], dev))
    b = _run_grouped(dev, case["qkv"], case["kc"], case["vc"], case["tables"], B, pos=pos)
    assert torch.equal(a[0], b[0]), "output differs from attention_decode_rope_grouped(pos=...)"
    for g in range(G):
        assert torch.equal(a[1][g], b[1][g]) and torch.equal(a[2][g], b[2][g]), f"group {g}: caches differ"


@pytest.mark.parametrize("G", [1, 8])
def test_group_counts(dev, G):
    """The smallest and the largest group count run and agree with the un-grouped form."""
    from bridgelang_amd import ops
    B = 2
    tables = _rope_tables(dev)
    qkv, kc, vc = _inputs(G, B, 1100 + G)
    pos = [[(37 * g + 5) % 400, 317 + g] for g in range(G)]
    o, Kc, Vc = _run_grouped(dev, qkv, kc, vc, tables, B, rope_pos=_rp(pos, dev))
    for g in range(G):
        r = slice(g * B, (g + 1) * B)
        K1, V1 = _dev(kc[g], dev), _dev(vc[g], dev)
        o1 = torch.zeros(B, D, dtype=torch.bfloat16, device=dev)
        ops.attention_decode_rope(_dev(qkv[r], dev), K1, V1, o1, tables[2], tables[3], B=B, H=H, head_dim=HD, pos=max(pos[g]),
                                  rope_pos=torch.tensor(pos[g], dtype=torch.int32, device=dev))
        assert torch.equal(o[r], o1) and torch.equal(Kc[g], K1) and torch.equal(Vc[g], V1), f"G={G} group {g}"


def test_argument_errors(dev):
    """Nine groups, and both or neither of pos / rope_pos, are refused before anything is launched."""
    B = 2
    tables = _rope_tables(dev)
    qkv, kc, vc = _inputs(1, B, 1200)
    with pytest.raises(ValueError):
        _run_grouped(dev, qkv.repeat(9, 1), kc * 9, vc * 9, tables, B, rope_pos=_rp([[1, 2]] * 9, dev))
    with pytest.raises(ValueError):
        _run_grouped(dev, qkv, kc, vc, tables, B)
    with pytest.raises(ValueError):
        _run_grouped(dev, qkv, kc, vc, tables, B, pos=[5], rope_pos=_rp([[5, 5]], dev))


@pytest.mark.parametrize("width", [512, 1536])
def test_gather_rows(dev, width):
    """bl_gather_rows_bf16 = src[arange(B), idx], first and last row of a batch included."""
    from bridgelang_amd import ops
    B, R = 3, 5
    src = _dev(rand_bf16((B, R, width), 1300 + width), dev)
    idx = torch.tensor([0, R - 1, 2], dtype=torch.int64, device=dev)
    dst = torch.full((B, width), 7.0, dtype=torch.bfloat16, device=dev)
    ops.gather_rows(src, idx, dst)
    assert torch.equal(dst, src[torch.arange(B, device=dev), idx])
    # rows inside a wider buffer (the q | k | v rows of the prefill: row stride 3 * width)
    wide = _dev(rand_bf16((B, R, 3 * width), 1301 + width), dev)
    ops.gather_rows(wide[:, :, :width], idx, dst)
    assert torch.equal(dst, wide[torch.arange(B, device=dev), idx, :width])
