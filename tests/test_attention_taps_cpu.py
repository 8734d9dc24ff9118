"""bridgelang_amd/attention_taps.py — the host definition behind bl_attention_probs_f32 — and the new symbol's plumbing.
Runs without a GPU."""
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import rand_bf16  # noqa: E402

from bridgelang_amd import _lib  # noqa: E402
from bridgelang_amd import attention_taps as T  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("causal", [False, True])
def test_probs_reference_is_softmax_attention(causal):
    B, H, Sq, Skv, hd = 2, 3, 5, 11, 128
    q, k = rand_bf16((B, H, Sq, hd), 1), rand_bf16((B, H, Skv, hd), 2)
    mask = torch.ones(B, Skv, dtype=torch.uint8)
    mask[0, 8:] = 0
    mask[1, 3] = 0
    scale = hd ** -0.5
    P = T.probs_reference(q, k, scale, causal, mask)
    assert P.dtype == torch.float64 and tuple(P.shape) == (B, H, Sq, Skv)
    s = scale * (q.double() @ k.double().transpose(-1, -2))
    hide = ~mask.bool().view(B, 1, 1, Skv).expand(B, H, Sq, Skv)
    if causal:
        hide = hide | (torch.arange(Skv).view(1, -1) > torch.arange(Sq).view(-1, 1) + (Skv - Sq))
    ref = torch.softmax(s.masked_fill(hide, float("-inf")), dim=-1)
    assert torch.allclose(P, ref, rtol=1e-13, atol=1e-300)
    assert bool((P[hide] == 0).all())
    assert torch.allclose(P.sum(-1), torch.ones(B, H, Sq, dtype=torch.float64), rtol=1e-13)


def test_probs_reference_row_without_visible_key_is_zero():
    q, k = rand_bf16((1, 1, 2, 128), 3), rand_bf16((1, 1, 4, 128), 4)
    mask = torch.tensor([[0, 0, 0, 1]], dtype=torch.uint8)
    P = T.probs_reference(q, k, 0.1, True, mask)      # row 0 sees keys 0..2 only, all masked
    assert bool((P[0, 0, 0] == 0).all())
    assert P[0, 0, 1, 3].item() == 1.0


def test_segment_sums_and_clipping():
    g = torch.Generator().manual_seed(5)
    P = torch.rand(2, 2, 3, 10, generator=g, dtype=torch.float64)
    bounds = torch.tensor([[0, 1, 4, 4, 9], [2, 2, 7, 12, 40]], dtype=torch.int32)     # second row runs past Skv: clipped
    S = T.segment_sums(P, bounds)
    assert tuple(S.shape) == (2, 2, 3, 4)
    assert torch.equal(S[0, :, :, 0], P[0, :, :, 0:1].sum(-1)) and torch.equal(S[0, :, :, 1], P[0, :, :, 1:4].sum(-1))
    assert bool((S[0, :, :, 2] == 0).all()) and torch.equal(S[0, :, :, 3], P[0, :, :, 4:9].sum(-1))
    assert bool((S[1, :, :, 0] == 0).all()) and torch.equal(S[1, :, :, 1], P[1, :, :, 2:7].sum(-1))
    assert torch.equal(S[1, :, :, 2], P[1, :, :, 7:10].sum(-1)) and bool((S[1, :, :, 3] == 0).all())


def test_prompt_segments_unpadded():
    names, b = T.prompt_segments(torch.ones(2, 9, dtype=torch.int64), n_patches=256, n_new=7)
    assert names == ("bos", "image", "text", "generated") == T.DEFAULT_NAMES
    assert b.dtype == torch.int32
    # BOS row 0, patches rows 1..256, the 8 text tokens rows 257..264, generated rows 265..271
    assert b.tolist() == [[0, 1, 257, 265, 272]] * 2


def test_prompt_segments_right_padded_with_splits():
    mask = torch.tensor([[1] * 9, [1] * 6 + [0] * 3])
    names, b = T.prompt_segments(mask, n_patches=4, n_new=3)
    # sequence 1 has 6 real tokens: text rows 5..9, its generated tokens go over its pad rows 10..12; rows 13.. are nobody's
    assert b.tolist() == [[0, 1, 5, 13, 16], [0, 1, 5, 10, 13]]
    # task | description | "\nOut:" — cuts at prompt tokens 4 and 8 (sequence 0), 3 and 5 (sequence 1)
    names, b = T.prompt_segments(mask, 4, 3, text_splits=torch.tensor([[4, 8], [3, 5]]))
    assert names == ("bos", "image", "text0", "text1", "text2", "generated")
    assert b.tolist() == [[0, 1, 5, 8, 12, 13, 16], [0, 1, 5, 7, 9, 10, 13]]
    with pytest.raises(ValueError):
        T.prompt_segments(mask, 4, 3, text_splits=torch.tensor([[4, 8], [3, 7]]))       # 7 > n_real = 6
    with pytest.raises(ValueError):
        T.prompt_segments(torch.tensor([[1, 0, 1]]), 4, 3)                               # not right-padded
    with pytest.raises(ValueError):
        T.prompt_segments(mask, 4, 3, text_splits=torch.tensor([[1, 2, 3, 4, 5, 6]] * 2))   # 10 segments > 8
    assert T.pad_bounds(b, 8).tolist()[1] == [0, 1, 5, 7, 9, 10, 13, 13, 13]


def test_attn_taps_resolve():
    assert T.AttnTaps().resolve(3) == (0, 1, 2)
    assert T.AttnTaps(layers=(-1, 0)).resolve(4) == (0, 3)
    with pytest.raises(ValueError):
        T.AttnTaps(layers=(4,)).resolve(4)
    with pytest.raises(ValueError):
        T.AttnTaps(full=False, segments=False).resolve(4)


def test_symbol_declared_bound_and_exported():
    name = "bl_attention_probs_f32"
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == 15            # desc, cos, sin, rope_rows, pos0, rope_pos, probs + 3 strides + cols, seg, bounds, n_seg, stream
    assert hasattr(_lib.load(), name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"bl_[a-z0-9_]+", line.split()[-1])}
    assert name in exported
    from bridgelang_amd import ops
    assert "attention_probs" in ops.__all__ and callable(ops.attention_probs)
