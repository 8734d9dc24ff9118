"""Where the action tokens attend: the attention probabilities over the prompt, per layer and per head — the host
SPECIFICATION (torch on the CPU, fp64) of `bl_attention_probs_f32` (csrc/attention_probs.hip) and the bookkeeping around it.

The host file is the definition and the kernel is its twin to a tolerance, as `training/value_loss.py` ↔ csrc/value.hip.

Definition. For one (batch, head) with rotated queries q [Sq, hd] and rotated keys k [Skv, hd] (bf16 values):

    visible(i, j) = key_mask[j] != 0  and  (not causal  or  j <= i + Skv - Sq)
    s_ij = scale * <q_i, k_j>                       over the visible j
    P_ij = exp(s_ij - max_j s_ij) / Σ_j exp(s_ij - max_j s_ij)      visible j;  0 for a hidden key

A row without a visible key is all 0. The kernel computes s' = s·log2e from an fp32 accumulation of the 128 exact bf16
products, exp2 and the row sum in fp32, and does NOT round P to bf16; its error against this definition is bounded in
tests/test_attention_probs_gpu.py (C_P = 0.25 in units of 2^-8·P, from the error model of tests/attn_ref64.py).

Segments. The OpenVLA sequence is  BOS | 256 image patches | prompt text | generated tokens, and the KV cache holds it
in that order, so "how much does action token t look at the image / the task / the description" is a sum of P over a
range of cache rows. `prompt_segments` turns an attention mask (and optional cuts of the text) into those ranges;
`segment_sums` is the definition of the kernel's `seg` output.

For a batch of RIGHT-PADDED prompts the engine writes a sequence's generated tokens over its own pad rows (cache row
n_patches + n_real + t for token t, `rope_pos` in engine.py), so the cache of every sequence is laid out as in its own
un-padded run: text ends at n_patches + n_real and `generated` starts there. Rows past the last generated token belong to
no segment.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

DEFAULT_NAMES = ("bos", "image", "text", "generated")
MAX_SEGMENTS = 8          # bl_attention_probs_f32's n_seg limit


@dataclass(frozen=True)
class AttnTaps:
    """What an `OpenVLAEngine(attn_taps=...)` records. layers: indices of the decoder layers to tap (None: all).
    full: keep the probabilities over every cache row. segments: keep their sums over the prompt segments."""
    layers: Optional[Tuple[int, ...]] = None
    full: bool = False
    segments: bool = True

    def resolve(self, n_layers: int) -> Tuple[int, ...]:
        if not (self.full or self.segments):
            raise ValueError("AttnTaps: ask for full, segments or both")
        if self.layers is None:
            return tuple(range(n_layers))
        layers = tuple(sorted({int(l) + n_layers if int(l) < 0 else int(l) for l in self.layers}))
        if not layers or layers[0] < 0 or layers[-1] >= n_layers:
            raise ValueError(f"AttnTaps: layers {self.layers} outside [0, {n_layers})")
        return layers

    def key(self, n_layers: int) -> tuple:
        return (self.resolve(n_layers), bool(self.full), bool(self.segments))


@dataclass
class ActionAttention:
    """Attention of the generated (action) tokens' queries. probs [B, n_new, n_layers_tapped, H, cache_len] fp32 or None:
    row t is the distribution of the query that PRODUCES token t (step 0: the last prompt position) over the cache rows;
    rows the step cannot see are 0. segments [B, n_new, n_layers_tapped, H, n_seg] fp32 or None: its sums over `names`.
    layers: the decoder-layer index of each tapped slot."""
    probs: Optional[torch.Tensor]
    segments: Optional[torch.Tensor]
    names: Tuple[str, ...]
    layers: Tuple[int, ...]


def visible(Sq: int, Skv: int, causal: bool, mask_row: Optional[torch.Tensor]) -> torch.Tensor:
    """[Sq, Skv] bool: key j is visible to query i iff mask_j != 0 and (not causal or j <= i + Skv - Sq)."""
    vis = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        vis &= torch.arange(Skv).view(1, -1) <= torch.arange(Sq).view(-1, 1) + (Skv - Sq)
    if mask_row is not None:
        vis &= mask_row.detach().cpu().to(torch.bool).view(1, Skv)
    return vis


def probs_reference(q: torch.Tensor, k_rotated: torch.Tensor, scale: float, causal: bool,
                    key_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 P [B, H, Sq, Skv] of rotated q [B, H, Sq, hd] against rotated keys [B, H, Skv, hd]; key_mask [B, Skv] (1 = attend)."""
    q, k = q.detach().cpu().double(), k_rotated.detach().cpu().double()
    B, H, Sq, _ = q.shape
    Skv = k.shape[2]
    out = torch.zeros(B, H, Sq, Skv, dtype=torch.float64)
    for b in range(B):
        vis = visible(Sq, Skv, causal, None if key_mask is None else key_mask[b])
        s = (scale * (q[b] @ k[b].transpose(-1, -2))).masked_fill(~vis, float("-inf"))
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        out[b] = e / torch.where(l > 0, l, torch.ones_like(l))
    return out


def segment_sums(P: torch.Tensor, bounds: torch.Tensor) -> torch.Tensor:
    """[B, H, Sq, n_seg]: the sum of P [B, H, Sq, Skv] over keys [bounds[b][s], bounds[b][s+1]), in P's dtype (fp64 for the
    definition). bounds int [B, n_seg + 1], non-decreasing; clipped to [0, Skv] as the kernel clips them."""
    B, H, Sq, Skv = P.shape
    bounds = bounds.detach().cpu().to(torch.int64)
    if bounds.dim() != 2 or bounds.shape[0] != B or bounds.shape[1] < 2:
        raise ValueError(f"segment_sums: bounds must be [B, n_seg + 1], got {tuple(bounds.shape)}")
    n_seg = bounds.shape[1] - 1
    out = torch.zeros(B, H, Sq, n_seg, dtype=P.dtype)
    for b in range(B):
        lo = int(bounds[b, 0].clamp(0, Skv))
        for s in range(n_seg):
            hi = min(max(int(bounds[b, s + 1]), lo), Skv)
            out[b, :, :, s] = P[b, :, :, lo:hi].sum(-1)
            lo = hi
    return out


def prompt_segments(attention_mask: torch.Tensor, n_patches: int, n_new: int,
                    text_splits: Optional[torch.Tensor] = None) -> Tuple[Tuple[str, ...], torch.Tensor]:
    """(names, int32 bounds [B, n_seg + 1]) of the prompt segments in cache coordinates.

    attention_mask [B, L] (1…1 0…0, BOS counted) gives every sequence's number of real tokens n_real. Without splits the
    segments are bos [0, 1), image [1, 1 + P), text [1 + P, P + n_real), generated [P + n_real, P + n_real + n_new).
    text_splits [B, k] are non-decreasing indices into input_ids (BOS counted, each in [1, n_real]) that cut `text` into
    k + 1 pieces text0 … textk: token index i of the prompt sits in cache row P + i."""
    m = torch.as_tensor(attention_mask).detach().cpu().to(torch.int64)
    if m.dim() != 2:
        raise ValueError("prompt_segments: attention_mask must be [B, L]")
    B, L = m.shape
    n_real = m.sum(1)
    if bool((n_real < 1).any()) or not bool((m.bool() == (torch.arange(L)[None, :] < n_real[:, None])).all()):
        raise ValueError("prompt_segments: prompts must be right-padded (attention_mask = 1…1 0…0) with at least one token")
    P = int(n_patches)
    cols = [torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64), torch.full((B,), 1 + P, dtype=torch.int64)]
    names: List[str] = ["bos", "image"]
    if text_splits is None:
        names.append("text")
    else:
        sp = torch.as_tensor(text_splits).detach().cpu().to(torch.int64)
        if sp.dim() == 1:
            sp = sp.view(1, -1).expand(B, -1)
        if sp.dim() != 2 or sp.shape[0] != B:
            raise ValueError(f"prompt_segments: text_splits must be [B, k], got {tuple(sp.shape)}")
        k = sp.shape[1]
        if bool((sp < 1).any()) or bool((sp > n_real[:, None]).any()) or (k > 1 and bool((sp[:, 1:] < sp[:, :-1]).any())):
            raise ValueError("prompt_segments: text_splits must be non-decreasing indices in [1, n_real] of each prompt")
        for j in range(k):
            cols.append(P + sp[:, j])
        names += [f"text{j}" for j in range(k + 1)]
    cols.append(P + n_real)
    cols.append(P + n_real + int(n_new))
    names.append("generated")
    if len(names) > MAX_SEGMENTS:
        raise ValueError(f"prompt_segments: at most {MAX_SEGMENTS} segments, got {len(names)}")
    return tuple(names), torch.stack(cols, dim=1).to(torch.int32)


def pad_bounds(bounds: torch.Tensor, n_seg: int) -> torch.Tensor:
    """bounds [B, k + 1] extended to [B, n_seg + 1] with empty trailing segments (an engine's seg buffers have a fixed width)."""
    B, have = bounds.shape
    if have - 1 > n_seg:
        raise ValueError(f"{have - 1} segments do not fit an engine built for {n_seg}")
    return torch.cat([bounds, bounds[:, -1:].expand(B, n_seg + 1 - have)], dim=1).contiguous()
