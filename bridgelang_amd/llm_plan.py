"""The Llama decoder layer and the generation head as op plans, written once.

`OpenVLAEngine` (one batch of B rows) and `StaggeredDecodePipeline` (the decode iterations of several batches stacked on
the row axis) emit the same layer: they differ only in HOW a linear, a normed linear and the attention are launched, and
pass those in as functions that return lists of Ops. A change of order, epilogue or fusion condition made here reaches
both, which is what "the pipeline equals the plain engine bit for bit" rests on."""
from __future__ import annotations

from typing import Callable, List

from . import ops
from .ops import EPI_F32_BF16R, EPI_NONE, EPI_RES, EPI_SWIGLU, Op

Emit = Callable[..., List[Op]]


def decode_fused(B: int, dims) -> bool:
    """A cached-decode layer takes its fused forms — RMSNorm inside the weight-streaming GEMM, RoPE and the KV append
    inside the attention kernel (head_dim 128 only) — when B rows fit the skinny kernel."""
    return ops.skinny_supported(B, dims.llm_dim, EPI_NONE) and dims.head_dim == 128


def head_fused(B: int, dims) -> bool:
    """The final RMSNorm rides inside the lm_head GEMM when B rows fit the skinny kernel."""
    return ops.skinny_supported(B, dims.llm_dim, EPI_F32_BF16R)


def decode_layer(l: int, lw, x, qkv, ao, act, norm_lin: Emit, lin: Emit, attn: Emit) -> List[Op]:
    """Layer l of a cached-decode step on the residual rows x (modeling_prismatic.py:325-341):
    norm + qkv → attention → o_proj + residual → norm + gate/up SwiGLU → down + residual.
    `norm_lin(x, norm_w, W, out, epi)` emits a linear with an RMSNorm in front, `lin(x, W, out, epi, res)` a plain one,
    `attn(l)` the attention from qkv into ao."""
    return (norm_lin(x, lw.ln1, lw.qkv_w, qkv, EPI_NONE) + attn(l) + lin(ao, lw.o_w, x, EPI_RES, x)
            + norm_lin(x, lw.ln2, lw.gu_w, act, EPI_SWIGLU) + lin(act, lw.down_w, x, EPI_RES, x))


def head(w, x, logits, norm_lin: Emit, pick: List[Op]) -> List[Op]:
    """final RMSNorm → lm_head (bf16-rounded fp32 logits) → `pick`: the argmax | sample | score ops over those logits."""
    return norm_lin(x, w.norm, w.lm_head, logits, EPI_F32_BF16R) + pick


def prefill_layer(lw, x, h, qkv, ao, act, eps: float, lin: Emit, attn: List[Op]) -> List[Op]:
    """A prefill layer over all rows of x: the order of decode_layer with the norms as launches of their own (h is their
    output). `lin(x, name, out, epi, **kw)` emits the linear with the layer's weight `name` — the bf16 GEMM or the e4m3
    pair; `attn` is the attention from qkv into ao, chosen by the caller."""
    return ([ops.rmsnorm(x, lw.ln1, h, eps, run=False)] + lin(h, "qkv_w", qkv, EPI_NONE) + attn
            + lin(ao, "o_w", x, EPI_RES, res=x) + [ops.rmsnorm(x, lw.ln2, h, eps, run=False)]
            + lin(h, "gu_w", act, EPI_SWIGLU) + lin(act, "down_w", x, EPI_RES, res=x))
