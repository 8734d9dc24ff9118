"""Glue between rollouts (`sample_actions` / `score_actions`) and the policy-loss training step
(`TrainStep(loss="policy")`): GRPO's group-normalised advantages, and the training batch of sampled action tokens.
Host-side tensor layout only; the loop that uses it is the caller's.

`policy_batch` serves both ratio levels of the loss unchanged. It gives every sequence one advantage and labels on
exactly its n action tokens, and those labelled tokens are what `PolicyLossConfig(ratio_level="action")` takes as the
sequence's group: the action's ratio π(a)/π_old(a) is formed from the n `old_logprobs` of the row, and
`TrainStep.action_stats()` reports it per sequence. With `rollout_is=True` it is the batch of a learner with the rollout
correction (`PolicyLossConfig.rollout_is_cap`): the sampler's log-probabilities are the behaviour policy's, not π_old.

`gae` is PPO's estimator for trajectories with per-step rewards and a learned critic (`TrainStep(value=...)`): advantages
for `set_policy_batch`, returns for `set_value_batch`.

`pairs_from_rewards` and `preference_batch` are the same glue for `TrainStep(loss="preference")`: the best rollout of a
prompt against the worst, laid out as consecutive chosen / rejected sequences by `policy_batch`.

`distill_batch` and `gaussian_bin_targets` are the glue for `TrainStep(loss="distill")`: a teacher's exact bin distribution
from `score_actions(return_bins=True)`, or a Gaussian round the demonstrated bin, as the [B, l, bins] teacher of
`set_distill_batch`, on `policy_batch`'s layout."""
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


def gae(rewards, values, last_values=None, dones=None, gamma: float = 0.99, lam: float = 0.95) -> Tuple[torch.Tensor, torch.Tensor]:
    """Generalised advantage estimation over N trajectories of T steps: rewards and values [N, T] (V of the state each
    action was taken in: what the rollout itself returned — `predict_action` / `sample_actions(..., return_values="action")`
    with the critic attached to the model (`attach_value_head`) — or, as before, the learner's `forward()` over the rollout
    batch, then `values()`), `last_values` [N] the value of
    the state after the last step (None: 0, the trajectory ended there), `dones` [N, T] true where the episode ended WITH
    step t (None: nowhere), so nothing is bootstrapped or carried across it:

        δ_t = r_t + γ·V_{t+1}·(1 − done_t) − V_t          V_T = last_values
        A_t = δ_t + γ·λ·(1 − done_t)·A_{t+1}              A_T = 0
        returns = A + V

    → fp32 (advantages, returns) [N, T], computed in fp64 on the host: the advantages feed `set_policy_batch` (one per
    sequence, e.g. through `policy_batch`), the returns `set_value_batch`. ValueError on a shape mismatch or a non-finite
    input."""
    r, v = _cpu(rewards, torch.float64), _cpu(values, torch.float64)
    if r.dim() != 2 or r.shape[1] < 1 or v.shape != r.shape:
        raise ValueError(f"gae: rewards and values [N, T], got {tuple(r.shape)} and {tuple(v.shape)}")
    N, T = r.shape
    last = torch.zeros(N, dtype=torch.float64) if last_values is None else _cpu(last_values, torch.float64)
    done = torch.zeros(N, T, dtype=torch.float64) if dones is None else _cpu(dones, torch.float64)
    if tuple(last.shape) != (N,) or tuple(done.shape) != (N, T):
        raise ValueError(f"gae: last_values [{N}] and dones [{N}, {T}], got {tuple(last.shape)} and {tuple(done.shape)}")
    if not all(bool(torch.isfinite(t).all()) for t in (r, v, last, done)) or not (np.isfinite(gamma) and np.isfinite(lam)):
        raise ValueError("gae: rewards, values, last_values, dones, gamma and lam must be finite")
    if bool(((done != 0) & (done != 1)).any()):
        raise ValueError("gae: dones holds 0 / 1 (or booleans)")
    adv = torch.zeros(N, T, dtype=torch.float64)
    nxt_v, nxt_a = last, torch.zeros(N, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        live = 1.0 - done[:, t]
        delta = r[:, t] + gamma * nxt_v * live - v[:, t]
        nxt_a = delta + gamma * lam * live * nxt_a
        adv[:, t] = nxt_a
        nxt_v = v[:, t]
    return adv.to(torch.float32), (adv + v).to(torch.float32)


def policy_batch(prompt_ids, attention_mask, token_ids, logprobs, advantages, pad_to: Optional[int] = None,
                 token_range: Optional[Tuple[int, int]] = None, values=None, returns=None, rollout_is: bool = False,
                 proximal_logprobs=None) -> Dict[str, torch.Tensor]:
    """The training batch of one sampled action per sequence. prompt_ids int64 [B, lp] right-padded with attention_mask
    [B, lp] (None: no padding); token_ids int64 [B, n] and logprobs [B, n] as `sample_actions` reports them (K samples per
    prompt: repeat the prompt rows and flatten to [B·K, n] first); advantages [B], one per sequence, broadcast over its n
    tokens. Repeated that way, the K sequences of a prompt are consecutive and equal up to the action tokens: the group order
    `TrainStep(shared_prompt=K, branch_len=n)` takes (one image per prompt there). Every sequence is laid out as

        prompt ‖ 29871 (the empty token, unless the prompt ends with it) ‖ the n action tokens ‖ EOS

    right-padded (pad id 32000, mask 0) to the longest one, or to `pad_to`. Labels cover exactly the n action tokens: the
    EOS position was never sampled and stays ignored. → dict of CPU tensors `input_ids`, `attention_mask`, `labels` (for
    `set_batch`) and `advantages`, `old_logprobs` fp32 [B, l] aligned with the labels (for `set_policy_batch`).
    A non-finite log-probability raises ValueError: a token outside a top-k / top-p support scores -inf, and the policy
    loss is defined for temperature-only rollouts. `token_range=(first, count)` is the learner's
    `PolicyLossConfig.token_range` (`model.action_token_range()`): an action token outside it raises ValueError — it has
    probability 0 under the restricted policy, so the rollouts were not drawn from it.
    `values` [B] (the critic's V(s) the rollout returned, `return_values="action"`) and `returns` [B] (`gae`'s) are checked
    (shape, finite) and passed through as fp32 `old_values` / `returns`, ready for `ts.set_value_batch(returns, old_values)`
    at value level "action"; a key is added only for the one that is given.
    `rollout_is=True` is the batch of a learner with the rollout correction (`PolicyLossConfig.rollout_is_cap`): the
    sampler's `logprobs` go out as `behaviour_logprobs` instead, and `old_logprobs` is `proximal_logprobs` [B, n] (the
    learner's own log-probabilities of the tokens before the update, finite) laid out the same way — or, when that is not
    given, absent: `ts.set_policy_batch(b["advantages"], b.get("old_logprobs"), behaviour_logprobs=b["behaviour_logprobs"])`
    is then the self-proximal step. `proximal_logprobs` without `rollout_is` raises ValueError."""
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
    if proximal_logprobs is not None and not rollout_is:
        raise ValueError("policy_batch: proximal_logprobs goes with rollout_is=True (without it logprobs ARE old_logprobs)")
    prox = None
    if proximal_logprobs is not None:
        prox = _cpu(proximal_logprobs, torch.float64)
        if tuple(prox.shape) != (B, n) or not bool(torch.isfinite(prox).all()):
            raise ValueError(f"policy_batch: proximal_logprobs [{B}, {n}], finite, got shape {tuple(prox.shape)}")
    extra = {}
    for key, name, x in (("old_values", "values", values), ("returns", "returns", returns)):
        if x is None:
            continue
        x = _cpu(x, torch.float64)
        if tuple(x.shape) != (B,):
            raise ValueError(f"policy_batch: {name} [{B}], one per sequence, got {tuple(x.shape)}")
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"policy_batch: {name} must be finite")
        extra[key] = x.to(torch.float32)
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
    out = {"input_ids": out_ids, "attention_mask": out_m, "labels": labels, "advantages": out_adv}
    if not rollout_is:
        out["old_logprobs"] = out_lp
    elif prox is not None:
        out["old_logprobs"] = torch.zeros(B, l, dtype=torch.float32)
        for b, (p, s) in enumerate(seqs):
            out["old_logprobs"][b, s:s + n] = prox[b].to(torch.float32)
    out.update(extra)
    if rollout_is:
        out["behaviour_logprobs"] = out_lp
    return out


def pairs_from_rewards(rewards, min_gap: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Preference pairs from rewards [B, K] of K rollouts per prompt: the best rollout against the worst. → (chosen index
    int64 [B], rejected index int64 [B], keep bool [B]); among equal rewards the lowest index wins on either side, and a
    prompt whose best and worst rewards tie, or lie closer than `min_gap`, is not kept."""
    r = _cpu(rewards, torch.float64)
    if r.dim() != 2 or r.shape[1] < 1:
        raise ValueError(f"pairs_from_rewards: rewards [B, K], got shape {tuple(r.shape)}")
    if not bool(torch.isfinite(r).all()):
        raise ValueError("pairs_from_rewards: rewards must be finite")
    if not min_gap >= 0:
        raise ValueError("pairs_from_rewards: min_gap must be >= 0")
    K = r.shape[1]
    first = lambda hit: torch.where(hit, torch.arange(K).expand_as(r), torch.full_like(r, K, dtype=torch.int64)).min(dim=1).values
    hi, lo = r.max(dim=1, keepdim=True).values, r.min(dim=1, keepdim=True).values
    gap = (hi - lo)[:, 0]
    return first(r == hi), first(r == lo), (gap > 0) & (gap >= min_gap)


def preference_batch(prompt_ids, attention_mask, chosen_ids, rejected_ids, ref_chosen=None, ref_rejected=None,
                     pad_to: Optional[int] = None, token_range: Optional[Tuple[int, int]] = None, groups=None) -> Dict[str, torch.Tensor]:
    """The training batch of loss="preference" from one chosen and one rejected action per prompt: prompt_ids [B, lp] with
    attention_mask as for `policy_batch`, chosen_ids / rejected_ids int64 [B, n]. Sequence 2k is prompt k with its chosen
    action and sequence 2k + 1 the same prompt with the rejected one, each laid out by `policy_batch`. ref_chosen /
    ref_rejected [B, n] are the reference policy's log-probabilities of those tokens as `score_actions(...,
    use_adapters=False)` reports them (both or neither: neither is the reference-free form). `groups` int [B] (ids dense
    in 1…P, default 1…B) gives prompts that share an id ONE pair — the trajectory form: the chosen actions of all its
    steps against the rejected ones. → dict of CPU tensors `input_ids`, `attention_mask`, `labels` [2B, l] (for
    `set_batch`, with the images repeated twice, `repeat_interleave(2, 0)`), `pair` int32 [2B] and `ref_logprobs` fp32
    [2B, l] or None (for `set_preference_batch`)."""
    ids, ch, rj = _cpu(prompt_ids, torch.int64), _cpu(chosen_ids, torch.int64), _cpu(rejected_ids, torch.int64)
    if ids.dim() != 2 or ch.dim() != 2 or ch.shape != rj.shape or ch.shape[0] != ids.shape[0]:
        raise ValueError(f"preference_batch: prompt_ids [B, lp], chosen_ids and rejected_ids [B, n], got {tuple(ids.shape)}, "
                         f"{tuple(ch.shape)} and {tuple(rj.shape)}")
    B, n = ch.shape
    if (ref_chosen is None) != (ref_rejected is None):
        raise ValueError("preference_batch: ref_chosen and ref_rejected go together")
    if groups is None:
        gid = torch.arange(1, B + 1, dtype=torch.int64)
    else:
        gid = _cpu(groups, torch.int64)
        seen = torch.unique(gid)
        if tuple(gid.shape) != (B,) or seen[0] != 1 or seen[-1] != len(seen):
            raise ValueError(f"preference_batch: groups int [{B}] with ids dense in 1…P")
    two = lambda a, b: torch.stack([a, b], dim=1).reshape(2 * B, *a.shape[1:])           # rows 2k, 2k + 1 = a[k], b[k]
    twice = lambda a: None if a is None else a.repeat_interleave(2, 0)
    have_ref = ref_chosen is not None
    ref = two(_cpu(ref_chosen, torch.float64), _cpu(ref_rejected, torch.float64)) if have_ref else torch.zeros(2 * B, n, dtype=torch.float64)
    if tuple(ref.shape) != (2 * B, n):
        raise ValueError(f"preference_batch: ref_chosen and ref_rejected [{B}, {n}]")
    batch = policy_batch(twice(ids), twice(None if attention_mask is None else _cpu(attention_mask, torch.bool)), two(ch, rj), ref,
                         torch.zeros(2 * B), pad_to=pad_to, token_range=token_range)
    return {"input_ids": batch["input_ids"], "attention_mask": batch["attention_mask"], "labels": batch["labels"],
            "pair": two(gid, -gid).to(torch.int32), "ref_logprobs": batch["old_logprobs"] if have_ref else None}


def distill_batch(prompt_ids, attention_mask, token_ids, bin_wt, wt, smoothing: float = 0.0, pad_to: Optional[int] = None,
                  token_range: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
    """The training batch of loss="distill" from one action per prompt and a teacher's bin distribution of each of its
    tokens: prompt_ids [B, lp] with attention_mask as for `policy_batch`, token_ids int64 [B, n], and bin_wt [B, n, bins] /
    wt [B, n, 2] as `score_actions(return_bins=True, action_tokens_only=True)` reports them for those tokens (integer
    weights over a kept total; the teacher may be the base policy, `use_adapters=False`, a checkpoint or an average). The
    teacher is q = bin_wt / wt[..., 1] in fp64, with `smoothing` = α mixed with the uniform distribution, (1 − α)·q +
    α / bins — what makes kind="reverse_kl" legal when a bin's integer weight is 0 — and rounded to fp32 once. The sequences
    are laid out by `policy_batch` (labels on exactly the n action tokens). → dict of CPU tensors `input_ids`,
    `attention_mask`, `labels` (for `set_batch`) and `teacher_probs` fp32 [B, l, bins] aligned with the labels, zero off them
    (for `set_distill_batch`). `token_range` is the learner's `DistillLossConfig.token_range`: its count must be `bins`."""
    tok = _cpu(token_ids, torch.int64)
    bw, w = _cpu(bin_wt, torch.float64), _cpu(wt, torch.float64)
    if tok.dim() != 2 or bw.dim() != 3 or tuple(bw.shape[:2]) != tuple(tok.shape) or tuple(w.shape) != tuple(tok.shape) + (2,):
        raise ValueError(f"distill_batch: token_ids [B, n], bin_wt [B, n, bins] and wt [B, n, 2], got {tuple(tok.shape)}, "
                         f"{tuple(bw.shape)} and {tuple(w.shape)}")
    B, n, bins = bw.shape
    if token_range is not None and int(token_range[1]) != bins:
        raise ValueError(f"distill_batch: token_range {tuple(token_range)} has not the {bins} bins of bin_wt")
    if not (np.isfinite(smoothing) and 0.0 <= smoothing <= 1.0):
        raise ValueError(f"distill_batch: 0 <= smoothing <= 1, got {smoothing!r}")
    total = w[..., 1]
    if not bool(torch.isfinite(bw).all()) or bool((bw < 0).any()) or not bool(torch.isfinite(total).all()) or bool((total <= 0).any()):
        raise ValueError("distill_batch: bin_wt must be finite and >= 0 and the kept total wt[..., 1] finite and > 0")
    q = (1.0 - smoothing) * (bw / total[..., None]) + smoothing / bins
    batch = policy_batch(prompt_ids, attention_mask, tok, torch.zeros(B, n), torch.zeros(B), pad_to=pad_to, token_range=token_range)
    labels = batch["labels"]
    teacher = torch.zeros(B, labels.shape[1], bins, dtype=torch.float32)
    teacher[labels != IGNORE_INDEX] = q.reshape(B * n, bins).to(torch.float32)      # row-major: sequence b's n tokens in order
    return {"input_ids": batch["input_ids"], "attention_mask": batch["attention_mask"], "labels": labels, "teacher_probs": teacher}


def gaussian_bin_targets(token_ids, sigma: float, token_range: Tuple[int, int]) -> torch.Tensor:
    """Soft ordinal labels for loss="distill": token_ids int64 [B, n] inside token_range = (first, count) → fp32 [B, n,
    count], a Gaussian over the bin index round each token's bin, exp(−(j − bin)² / (2σ²)), truncated at the range's ends
    and normalised in fp64. Neighbouring bins are neighbouring actions, which a one-hot label cannot say; sigma → 0 gives
    the one-hot (sigma = 0 is it exactly)."""
    tok = _cpu(token_ids, torch.int64)
    first, count = int(token_range[0]), int(token_range[1])
    if tok.dim() != 2:
        raise ValueError(f"gaussian_bin_targets: token_ids [B, n], got {tuple(tok.shape)}")
    if not (np.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"gaussian_bin_targets: sigma must be >= 0, got {sigma!r}")
    if bool(((tok < first) | (tok >= first + count)).any()):
        raise ValueError(f"gaussian_bin_targets: token(s) outside token_range [{first}, {first + count})")
    d = torch.arange(count, dtype=torch.float64) - (tok - first)[..., None].to(torch.float64)
    if sigma == 0:
        g = (d == 0).to(torch.float64)
    else:
        g = torch.exp(-0.5 * (d / sigma) ** 2)        # the token's own bin is exp(0) = 1: the sum never vanishes
    return (g / g.sum(dim=-1, keepdim=True)).to(torch.float32)
