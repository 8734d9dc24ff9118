"""Glue between rollouts (`sample_actions` / `score_actions`) and the policy-loss training step
(`TrainStep(loss="policy")`): GRPO's group-normalised advantages, and the training batch of sampled action tokens.
Host-side tensor layout only; the loop that uses it is the caller's.

`policy_batch` serves both ratio levels of the loss unchanged. It gives every sequence one advantage and labels on
exactly its n action tokens, and those labelled tokens are what `PolicyLossConfig(ratio_level="action")` takes as the
sequence's group: the action's ratio π(a)/π_old(a) is formed from the n `old_logprobs` of the row, and
`TrainStep.action_stats()` reports it per sequence."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

IGNORE_INDEX = -100
EMPTY_TOKEN, EOS_TOKEN, PAD_TOKEN = 29871, 2, 32000


def _cpu(x, dtype) -> torch.Tensor:
    return (x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to("cpu", dtype)


def group_advantages(rewards, eps: float = 1e-6) -> torch.Tensor:
    """GRPO normalisation: rewards [B, K] (K rollouts of each of B prompts) → fp32 [B, K] advantages
    (r − mean_K) / (std_K + eps), with the population standard deviation of the group (a group of one, or of equal
    rewards, gets 0)."""
    r = _cpu(rewards, torch.float64)
    if r.dim() != 2 or r.shape[1] < 1:
        raise ValueError(f"group_advantages: rewards [B, K], got shape {tuple(r.shape)}")
    if not bool(torch.isfinite(r).all()):
        raise ValueError("group_advantages: rewards must be finite")
    mean = r.mean(dim=1, keepdim=True)
    std = (r - mean).pow(2).mean(dim=1, keepdim=True).sqrt()
    return ((r - mean) / (std + eps)).to(torch.float32)


def policy_batch(prompt_ids, attention_mask, token_ids, logprobs, advantages, pad_to: Optional[int] = None,
                 token_range: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
    """The training batch of one sampled action per sequence. prompt_ids int64 [B, lp] right-padded with attention_mask
    [B, lp] (None: no padding); token_ids int64 [B, n] and logprobs [B, n] as `sample_actions` reports them (K samples per
    prompt: repeat the prompt rows and flatten to [B·K, n] first); advantages [B], one per sequence, broadcast over its n
    tokens. Every sequence is laid out as

        prompt ‖ 29871 (the empty token, unless the prompt ends with it) ‖ the n action tokens ‖ EOS

    right-padded (pad id 32000, mask 0) to the longest one, or to `pad_to`. Labels cover exactly the n action tokens: the
    EOS position was never sampled and stays ignored. → dict of CPU tensors `input_ids`, `attention_mask`, `labels` (for
    `set_batch`) and `advantages`, `old_logprobs` fp32 [B, l] aligned with the labels (for `set_policy_batch`).
    A non-finite log-probability raises ValueError: a token outside a top-k / top-p support scores -inf, and the policy
    loss is defined for temperature-only rollouts. `token_range=(first, count)` is the learner's
    `PolicyLossConfig.token_range` (`model.action_token_range()`): an action token outside it raises ValueError — it has
    probability 0 under the restricted policy, so the rollouts were not drawn from it."""
    ids, tok = _cpu(prompt_ids, torch.int64), _cpu(token_ids, torch.int64)
    lp, adv = _cpu(logprobs, torch.float64), _cpu(advantages, torch.float64)
    if ids.dim() != 2 or tok.dim() != 2 or tok.shape[0] != ids.shape[0] or tok.shape[1] < 1:
        raise ValueError(f"policy_batch: prompt_ids [B, lp] and token_ids [B, n], got {tuple(ids.shape)} and {tuple(tok.shape)}")
    B, n = tok.shape
    if tuple(lp.shape) != (B, n) or tuple(adv.shape) != (B,):
        raise ValueError(f"policy_batch: logprobs [{B}, {n}] and advantages [{B}], got {tuple(lp.shape)} and {tuple(adv.shape)}")
    if not bool(torch.isfinite(lp).all()):
        raise ValueError("policy_batch: non-finite log-probability — a token outside the rollout's top-k / top-p support scores "
                         "-inf; draw training rollouts with temperature only")
    if not bool(torch.isfinite(adv).all()):
        raise ValueError("policy_batch: advantages must be finite")
    if token_range is not None:
        first, count = int(token_range[0]), int(token_range[1])
        outside = (tok < first) | (tok >= first + count)
        if bool(outside.any()):
            raise ValueError(f"policy_batch: {int(outside.sum())} action token(s) outside token_range [{first}, {first + count}) "
                             f"(first: {int(tok[outside][0])}) — draw rollouts with action_tokens_only=True")
    if attention_mask is None:
        lens = [ids.shape[1]] * B
    else:
        m = _cpu(attention_mask, torch.bool)
        if m.shape != ids.shape:
            raise ValueError("policy_batch: attention_mask must have the shape of prompt_ids")
        lens = [int(v) for v in m.sum(dim=1)]
        if any(not bool(m[b, :lens[b]].all()) for b in range(B)) or min(lens) < 1:
            raise ValueError("policy_batch: prompts must be right-padded and non-empty")
    seqs = []
    for b in range(B):
        p = ids[b, :lens[b]]
        if int(p[-1]) != EMPTY_TOKEN:
            p = torch.cat([p, torch.tensor([EMPTY_TOKEN])])
        seqs.append((p, len(p)))
    l = max(s for _, s in seqs) + n + 1
    if pad_to is not None:
        if pad_to < l:
            raise ValueError(f"policy_batch: pad_to={pad_to} is shorter than the longest sequence ({l})")
        l = pad_to
    out_ids = torch.full((B, l), PAD_TOKEN, dtype=torch.int64)
    out_m = torch.zeros(B, l, dtype=torch.bool)
    labels = torch.full((B, l), IGNORE_INDEX, dtype=torch.int64)
    out_adv, out_lp = torch.zeros(B, l, dtype=torch.float32), torch.zeros(B, l, dtype=torch.float32)
    for b, (p, s) in enumerate(seqs):
        out_ids[b, :s] = p
        out_ids[b, s:s + n] = tok[b]
        out_ids[b, s + n] = EOS_TOKEN
        out_m[b, :s + n + 1] = True
        labels[b, s:s + n] = tok[b]
        out_adv[b, s:s + n] = float(adv[b])
        out_lp[b, s:s + n] = lp[b].to(torch.float32)
    return {"input_ids": out_ids, "attention_mask": out_m, "labels": labels, "advantages": out_adv, "old_logprobs": out_lp}
