"""One optimisation step of OpenVLA training on one MI355X: forward with saved activations, hand-written backward,
global-norm clip and AdamW — the device side of the reference's `TrainingStrategy.run_vla_training` loop body
(prismatic/training/strategies/base_strategy.py:296-346) with the module freezing of `PrismaticVLM.freeze_backbones`
(prismatic/models/vlms/prismatic.py:129-241) and the optimizer grouping of `FSDPStrategy.run_setup`
(prismatic/training/strategies/fsdp.py:195-236).

MI355X-first choices (DESIGN.md "Training step"):
  * no autograd, no tracing: the step is three static lists of prepared C calls (forward, backward, repack) over
    preallocated buffers, so each list replays under a HIP graph;
  * no activation checkpointing (the reference enables it for 80 GB parts, fsdp.py:176-186): every layer's activations
    stay resident — ≈ 4.2 MB / token at 7B, 20 GB for 16 × 290 tokens out of 288 GB;
  * weights live twice in bf16, fragment-major for the forward GEMM ([N,K] packed) and transposed for the dgrad GEMM
    ([K,N] packed); wgrad is the same NT GEMM kernel over transposed, token-padded activations, accumulating in fp32
    straight into the flat fp32 gradient buffer;
  * fp32 master weights and AdamW moments are flat buffers, so the optimizer is a handful of launches; the clip
    coefficient is consumed on the device (no host sync inside the step).
"""
from __future__ import annotations

import contextlib

from typing import Dict, List, Optional, Tuple

import os

import numpy as np
import torch

from .. import ops, train_ops as T
from ..engine import rope_tables
from ..ops import EPI_BIAS, EPI_F32_BF16R, EPI_NONE, EPI_RES, Op
from ..weights import VLAWeights
from .distill_loss import DISTILL_STAT_NAMES, DistillLossConfig, check_teacher
from .linears import Linears, Scratch, ScratchSet
from .param_store import STAGES, ParamStore, no_decay, param_sharded_key, pool_of, trainable_names      # noqa: F401  (re-exported)
from .policy_loss import GROUP_STAT_NAMES, IS_STAT_NAMES, STAT_NAMES, PolicyLossConfig
from .preference_loss import PAIR_STAT_NAMES, PREF_STAT_NAMES, SEQ_STAT_NAMES, PreferenceLossConfig, check_pairs
from . import shared_prompt as SP
from .sharding import ShardComm, comm_order
from .unit_pools import UnitPools
from .value_head import ValueHead
from .value_loss import VALUE_STAT_NAMES, ValueLossConfig

IGNORE_INDEX = -100


class TrainStep:
    """Static-shape training step for batches of B samples with L (padded) text tokens."""

    def __init__(self, weights: VLAWeights, stage: str, batch: int, prompt_len: int, *, max_grad_norm: float = 1.0,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, store: Optional[ParamStore] = None,
                 world: int = 1, rank: int = 0, group=None, reduce_dtype: torch.dtype = torch.float32, lora=None,
                 force_comm: bool = False, recompute: bool = False, shard_params: bool = False, fp8: bool = False,
                 fp8_wgrad: bool = False, loss: str = "ce", policy: Optional[PolicyLossConfig] = None,
                 refresh_adapted: bool = False, preference: Optional[PreferenceLossConfig] = None,
                 value: Optional[ValueLossConfig] = None, value_head: Optional[ValueHead] = None,
                 distill: Optional[DistillLossConfig] = None, shared_prompt: Optional[int] = None,
                 branch_len: Optional[int] = None):
        """`lora`: a training.lora.LoraAdapters → stage "lora": the base model is frozen and only the adapters train.
        `refresh_adapted` (with `lora`): the re-pack plan that follows every optimizer step ends with the ONE batched merge
        launch of `lora.refresh_ops()`, so `lora.adapted_weights()` — the weights an inference engine of the model the adapters
        are attached to reads — are the learner's after every step, eager or graph replay. Off by default: plans unchanged.
        `recompute`: keep only each decoder layer's input and replay its forward inside the backward pass.
        `shard_params`: FSDP FULL_SHARD for every FSDP unit — decoder layers, ViT blocks and stems, projector, token
        embeddings, lm_head (fsdp.py:84-87) — every rank keeps 1/world of each unit's bf16 weights; a unit is all-gathered
        into one of its pool's two slots (and packed into the forward / dgrad layouts there) one unit ahead of its forward
        and again ahead of its backward, on the communication stream; AdamW updates the rank's slice in place. The model's
        own allocations of those units are freed (`materialize_params()` brings them back).
        `fp8`: the decoder layers' forward and input-gradient GEMMs (q/k/v, o, gate/up, down: 2/3 of the step's GEMM work)
        run W8A8 on the e4m3 MFMA path (BASELINE configs[4]) — activations / output gradients quantised per token row,
        weights per output channel (forward) and per input channel (the transposed dgrad copy), fp32 accumulation, bf16
        results; weight gradients stay bf16 x bf16 (TN GEMM), masters and AdamW fp32. No reference counterpart: agreement
        with the bf16 step is to quantisation noise (tests/test_train_step_gpu.py states the bound).
        `fp8_wgrad` (with `fp8`): the decoder layers' WEIGHT-gradient GEMMs run on the e4m3 MFMA path too, so all three GEMM
        families of those layers are fp8: dW[n, k] = Σ_t dy[t, n]·x[t, k] contracts over tokens, so dy and x are transposed
        to token-contiguous rows and quantised per ROW of the transposed matrix — one scale per output channel n of dy and
        per input channel k of x, i.e. along the non-contracted dimensions, where the scales factor out of the sum exactly —
        and dW = s_dy[n]·s_x[k]·(dyT8 · xT8ᵀ) accumulates in fp32 straight into the flat gradient buffer.
        `loss`: "ce" (the shifted cross-entropy of the labelled tokens) or "policy": the clipped-surrogate policy gradient
        of training/policy_loss.py over the same rows, configured by `policy` (a PolicyLossConfig; its defaults if None) and
        fed by `set_policy_batch` after `set_batch`. Only the two ops at the loss boundary differ; everything below the
        logits, and every other option, is shared. With `policy.token_range=(first, count)` the two ops are the ranged
        entry points: the policy — and with it `token_logprobs()` and `policy_stats()` — is the softmax over that token range
        alone, as rollouts drawn with `action_tokens_only=True` need, and dlogits is 0 outside it. With
        `policy.ratio_level="action"` the forward's loss op is the grouped entry point: one importance ratio per sequence
        (its labelled tokens are the action), reported by `action_stats()`; the backward plan is the same. With
        `policy.rollout_is_cap` the forward's loss op is bl_policy_loss_is_f32 (either level): the surrogate carries a
        truncated importance weight between the proximal policy and the one that drew the tokens (`set_policy_batch`'s
        `behaviour_logprobs`), reported by `rollout_stats()` and `token_weights()`; the backward plan is the same.
        `loss="preference"`: the preference-pair loss of training/preference_loss.py (DPO, IPO, hinge; cDPO, SimPO and RPO
        by its options) over the same rows, configured by `preference` (a PreferenceLossConfig; its defaults if None) and fed
        by `set_preference_batch` after `set_batch`: every sequence is the chosen or the rejected side of a pair, or in
        none. The forward's loss op is bl_preference_loss_f32; the backward's is the policy loss's, which divides by the
        number of pairs in `mean_cnt[1]`. `token_range` as for the policy loss.
        `value` (with loss="policy"; a training.value_loss.ValueLossConfig): a critic trains with the policy — the linear
        `value_head` (a training.value_head.ValueHead on the final-norm output; a zero-initialised one is created when None,
        `ts.value_head`) under PPO's clipped value loss, fed by `set_value_batch` after `set_batch`. The head's two tensors
        join the store's extra units beside LoRA's (a caller's `store` must carry them). bl_value_head_f32 follows the
        policy loss op in the forward plan and bl_value_head_backward_f32 sits between lm_head's input-gradient GEMM and the
        final norm's backward, adding the value loss's gradient into `dh`; `forward()` then returns policy loss + coef ·
        value loss. Without `value` both plans are what they were. Critic warm-up needs no mode of its own: advantages of 0
        with entropy_coef = kl_coef = 0 make dlogits exactly 0, so every trunk gradient is the value path's.
        `loss="distill"`: the distribution-matching loss of training/distill_loss.py (forward KL, reverse KL or JSD against
        a teacher's whole row over the token range, plus sft_coef · NLL), configured by `distill` (a DistillLossConfig; its
        defaults if None) and fed by `set_distill_batch` after `set_batch`. The forward plan ends with bl_distill_loss_f32 in
        place of the cross-entropy op and the backward plan starts with bl_distill_loss_backward_f32; the teacher lives in
        a static fp32 buffer [B·S, count] in row layout, so a captured graph serves every batch. `token_range` as for the
        policy loss; `distill_stats()` reports the step statistics. `policy`, `preference` and `value` do not go with it.
        `shared_prompt=G` with `branch_len=nb` (loss "ce" or "policy", either ratio level, with or without the rollout
        correction; every stage, `recompute`, eager and graph replay): the B sequences come in consecutive groups of G that
        share their prompt — what `rl.policy_batch` emits for G samples per prompt — and the step runs each group as ONE row
        of the layout of training/shared_prompt.py, prefix ‖ G branches of nb rows: the towers, the projector and every
        decoder layer see P = B / G images and P·(P0 + G·nb) token rows instead of B and B·S. The decoder's rotary embedding
        and attention are then bl_rope_pos_bf16 / bl_attention_tree_lse_bf16 and their backwards, and the loss kernels take
        the branches as their groups (group_rows = nb); every other op is the replicated step's over fewer rows.
        `set_batch` / `set_batch_frames` take ids / mask / labels [B, l] as ever and pixel values / frames [P, …], one per
        prompt; everything per token that is passed or read [B, l] (`set_policy_batch`, `token_logprobs()`,
        `token_weights()`, `action_stats()` [B]) keeps its shape and order. `preference`, `distill`, `value`, `fp8` and
        world > 1 raise ValueError with it: follow-ups. Without it both plans are what they were."""
        if loss not in ("ce", "policy", "preference", "distill"):
            raise ValueError(f"loss must be 'ce', 'policy', 'preference' or 'distill', got {loss!r}")
        if distill is not None and loss != "distill":
            raise ValueError("`distill` configures loss='distill'")
        if loss == "distill" and (policy is not None or preference is not None or value is not None):
            raise ValueError("loss='distill' takes `distill` alone: `policy`, `preference` and `value` configure other losses")
        if policy is not None and loss != "policy":
            raise ValueError("`policy` configures loss='policy'")
        if preference is not None and loss != "preference":
            raise ValueError("`preference` configures loss='preference'")
        if value is not None and loss != "policy":
            raise ValueError("`value` (the critic) trains with loss='policy'")
        if value_head is not None and value is None:
            raise ValueError("`value_head` goes with `value` (a ValueLossConfig)")
        if value is not None and value_head is not None and value_head.dim != weights.dims.llm_dim:
            raise ValueError(f"value_head.dim {value_head.dim} is not the model's llm_dim {weights.dims.llm_dim}")
        self.shared: Optional[SP.SharedPromptLayout] = None
        if (shared_prompt is None) != (branch_len is None):
            raise ValueError("shared_prompt (the group size G) and branch_len (the rows per branch) go together")
        if shared_prompt is not None:
            for what, on in (("loss='preference'", loss == "preference"), ("loss='distill'", loss == "distill"),
                             ("value= (the critic)", value is not None), ("fp8=True", fp8),
                             ("world > 1 / shard_params", world > 1 or shard_params or (store is not None and store.layout.world > 1))):
                if on:
                    raise ValueError(f"shared_prompt does not run with {what} yet: the shared-prompt step covers loss 'ce' and "
                                     "'policy' on one GPU with bf16 GEMMs")
            if weights.dims.head_dim != 128:
                raise ValueError("shared_prompt: the tree attention kernels are built for head_dim 128")
            self.shared = SP.SharedPromptLayout(int(batch), int(shared_prompt), int(branch_len), int(prompt_len), weights.dims.n_patches)
            self.B_seq, self.L_seq = batch, prompt_len                      # what the caller passes and reads
            batch, prompt_len = self.shared.P, self.shared.text_len         # what the plans run over: P rows of the layout
        self.value = value
        self.value_head = (value_head or ValueHead(weights.dims.llm_dim, weights.embed.device)) if value is not None else None
        self.loss_kind = loss
        self.policy = (policy or PolicyLossConfig()) if loss == "policy" else None
        self.preference = (preference or PreferenceLossConfig()) if loss == "preference" else None
        self.distill = (distill or DistillLossConfig()) if loss == "distill" else None
        self._row_cfg = self.policy or self.preference or self.distill      # whichever loss keeps row_stats: its T and token range
        if self._row_cfg is not None and self._row_cfg.token_range is not None:
            first, count = self._row_cfg.token_range
            if first % 8 or count % 8 or first + count > weights.dims.vocab:
                raise ValueError(f"{loss}.token_range {self._row_cfg.token_range}: multiples of 8 inside the vocabulary "
                                 f"[0, {weights.dims.vocab})")
        if (lora is not None) != (stage == "lora"):
            raise ValueError("stage 'lora' and the `lora` adapters go together")
        if refresh_adapted and lora is None:
            raise ValueError("refresh_adapted goes with stage 'lora' and its `lora` adapters")
        if (recompute or shard_params or fp8) and lora is not None:
            raise ValueError("activation recomputation / parameter sharding / fp8 GEMMs are planned for the full-parameter stages only")
        if fp8 and (weights.dims.llm_dim % 128 or weights.dims.llm_inter % 128):
            raise ValueError("fp8 GEMMs need llm_dim and llm_inter to be multiples of 128")
        if fp8_wgrad and not fp8:
            raise ValueError("fp8_wgrad extends fp8=True (e4m3 forward / dgrad) to the weight-gradient GEMMs")
        self.fp8, self.fp8_wgrad = fp8, fp8_wgrad
        self.recompute, self.shard_params = recompute, shard_params
        self.lora = lora
        self.train_vision = STAGES[stage][0] or lora is not None      # towers need their training-form forward
        self.w, self.dims, self.stage = weights, weights.dims, stage
        d = self.dims
        self.B, self.L, self.S = batch, prompt_len, prompt_len + d.n_patches
        if self.S > d.max_pos:
            raise ValueError(f"sequence of {self.S} positions exceeds the model's {d.max_pos} (model_max_length)")
        self.max_grad_norm, self.weight_decay, self.betas, self.eps = max_grad_norm, weight_decay, betas, eps
        if store is None:
            extra = (lora.plain_units() if lora is not None else []) + (self.value_head.plain_units() if value is not None else [])
            store = ParamStore(weights, stage, world, rank, extra=extra or None, shard_params=shard_params, defer_grads=True)
        elif value is not None:
            for name, live, _, _ in self.value_head.plain_units():
                u = store.by_name.get(name)
                if u is None or u.dst is None or u.dst.data_ptr() != live.data_ptr():
                    raise ValueError(f"the given store does not carry this value head's `{name}`: build it with "
                                     "extra=[... + value_head.plain_units()]")
        self.store = store
        assert self.store.stage == stage and self.store.shard_params == shard_params
        shard_params = self.shard_params = shard_params and bool(self.store.sharded_keys)      # frozen LLM: nothing to shard
        st = self.store
        self.comm = ShardComm(st.layout, group, reduce_dtype, force=force_comm)
        self.world = st.layout.world
        dev = weights.embed.device
        self.device = dev
        self._wide: Dict[int, torch.Tensor] = {}
        self.lin = Linears(weights, st, lora, batch, batch * self.S, self._wide, fp8=fp8, fp8_wgrad=fp8_wgrad, shard_params=shard_params)
        self.fp8_wgrad_gemms = self.lin.fp8_wgrad_gemms
        self.pools: Optional[UnitPools] = None
        if shard_params:                       # first: the model's unit allocations are given back before anything else is reserved
            self.pools = self.lin.pools = UnitPools(weights, st, self.comm, self.lin, recompute, fp8)
        if st.grad is None:
            st.use_grad_slots = self.comm.active
        st.alloc_grads()
        B, S, D, I, V, NL = batch, self.S, d.llm_dim, d.llm_inter, d.vocab, d.llm_layers
        Tn = B * S
        self.T = Tn
        z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype, device=dev)
        # LoRA K-concatenation: the input x of an adapted linear and the gradient dy of its output live in buffers that
        # are R columns wider than the tensor; t = x·Aᵀ / dt = dy·(sB) land in those columns, so y = [x | t]·[W | sB]ᵀ
        # and dx = [dy | dt]·[Wᵀ | Aᵀ]ᵀ are single GEMMs over K + R (no separate rank-R update pass over y / dx).
        R_ = lambda packed: (lora.get(packed).R if (lora is not None and lora.get(packed) is not None) else 0)

        def za(rows: int, cols: int, extra: int) -> torch.Tensor:
            if not extra:
                return z(rows, cols)
            wide = z(rows, cols + extra)
            view = wide[:, :cols]
            self._wide[view.data_ptr()] = wide
            return view
        self._za, self._R = za, R_
        L0 = weights.layers[0]
        # ---- inputs ----
        self.input_ids = z(B, prompt_len, dtype=torch.int64)
        self.key_mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
        self.targets = torch.full((Tn,), IGNORE_INDEX, dtype=torch.int64, device=dev)
        self._group_rows = S                     # rows per group of the loss kernels: a sequence, or a branch
        if self.shared is not None:
            lay = self.shared
            self._group_rows = lay.nb
            self.pos_rows = torch.arange(S, dtype=torch.int32, device=dev).repeat(B)      # rotary position of every row
            per = S // lay.nb                    # groups per prompt row; branch g is group P0 / nb + g of its prompt
            self._branch_groups = (torch.arange(lay.P, device=dev)[:, None] * per + lay.P0 // lay.nb
                                   + torch.arange(lay.G, device=dev)[None, :]).reshape(-1)
            self._token_row = np.full((self.B_seq, 1), -1, dtype=np.int64)
        # ---- frozen vision front end: reuse the inference engine's tower plans (its LLM buffers are not allocated twice:
        #      prompt_len 1, no decode) ----
        from ..engine import OpenVLAEngine
        self._vis = OpenVLAEngine(weights, batch, 1, n_new=1, vision_only=True)
        if self.pools is not None and "vision" in self.pools.slots:
            self._vis.dino_ops = self._vis.siglip_ops = self._vis.vision_ops = []      # the towers' weights live in gather slots
        self.pixel_values = self._vis.pixel_values
        self.feats = self._vis.feats if lora is None else za(B * 256, d.vision_dim, R_(weights.fc1_w))
        # ---- saved activations ----
        Pv = 4 * d.vision_dim
        self.z1, self.z2, self.p3 = z(B * 256, Pv), z(B * 256, D), z(B * 256, D)
        self.p1, self.p2 = za(B * 256, Pv, R_(weights.fc2_w)), za(B * 256, D, R_(weights.fc3_w))
        self.x = [z(Tn, D) for _ in range(NL + 1)]            # residual stream entering layer l (x[NL] = final)
        # per-layer saved activations; with `recompute` (the reference's activation checkpointing of the decoder layers,
        # fsdp.py:171-183) every layer shares ONE set and only the layer inputs x[l] are kept
        def per_layer(make):
            if not recompute:
                return [make() for _ in range(NL)]
            one = make()
            return [one] * NL
        self.xm = per_layer(lambda: z(Tn, D))
        self.h1 = per_layer(lambda: za(Tn, D, R_(L0.qkv_w)))
        self.h2 = per_layer(lambda: za(Tn, D, R_(L0.gu_w)))
        self.qkv = per_layer(lambda: za(Tn, 3 * D, R_(L0.qkv_w)))     # same leading dimension as dqkv (shared strides)
        self.ao = per_layer(lambda: za(Tn, D, R_(L0.o_w)))
        self.gu = per_layer(lambda: z(Tn, 2 * I))
        self.act = per_layer(lambda: za(Tn, I, R_(L0.down_w)))
        pad = (S + 31) // 32 * 32
        self.lse = per_layer(lambda: z(B * d.llm_heads * pad, dtype=torch.float32))
        self.delta = z(B * d.llm_heads * pad, dtype=torch.float32)
        self.hn = z(Tn, D)
        self.logits = z(Tn, V, dtype=torch.float32)
        if self.preference is not None:         # mean_cnt = (loss, P): the backward kernel divides by the number of pairs
            self.ref_logprob = z(Tn, dtype=torch.float32)
            self.row_stats, self.stats = z(Tn, 8, dtype=torch.float32), z(8, dtype=torch.float32)
            self.row_loss, self.mean_cnt = self.row_stats[:, 3], self.stats[:2]
            self.pair, self.n_pairs = z(B, dtype=torch.int32), torch.ones(1, dtype=torch.int32, device=dev)
            self.pair_stats_buf, self.seq_stats_buf = z(max(B // 2, 1), 4, dtype=torch.float32), z(B, 4, dtype=torch.float32)
            self._batch_len, self._pairs_set = prompt_len, False
        elif self.distill is not None:          # the teacher in row layout over the range; mean_cnt = (loss, n_valid)
            count = self.distill.token_range[1] if self.distill.token_range is not None else V
            self.teacher = z(Tn, count, dtype=torch.float32)
            self.row_stats, self.stats = z(Tn, 8, dtype=torch.float32), z(8, dtype=torch.float32)
            self.row_loss, self.mean_cnt = self.row_stats[:, 3], self.stats[:2]
            self._batch_len, self._teacher_set = prompt_len, False
        elif self.policy is None:
            self.row_loss, self.mean_cnt = z(Tn, dtype=torch.float32), z(2, dtype=torch.float32)
        else:                                   # per-row inputs and statistics of the policy loss; mean_cnt = (loss, n_valid)
            self.advantages, self.old_logprob, self.ref_logprob = (z(Tn, dtype=torch.float32) for _ in range(3))
            self.row_stats, self.stats = z(Tn, 8, dtype=torch.float32), z(8, dtype=torch.float32)
            self.row_loss, self.mean_cnt = self.row_stats[:, 3], self.stats[:2]
            if self.policy.ratio_level == "action":      # one group per sequence: its S rows (shared prompt: per nb rows)
                self.group_stats = z(Tn // self._group_rows, 4, dtype=torch.float32)
            if self.policy.rollout_is_cap is not None:   # the rollout correction: μ per row in, (λ, w) per row and 8 means out
                self.behaviour_logprob = z(Tn, dtype=torch.float32)
                self.is_rows, self.is_stats = z(Tn, 2, dtype=torch.float32), z(8, dtype=torch.float32)
                self._self_proximal = False
            self._batch_len = prompt_len
            if value is not None:               # the critic: per-row inputs, the device's list of value rows, per-row outputs
                self.returns, self.old_values = z(Tn, dtype=torch.float32), z(Tn, dtype=torch.float32)
                self.value_rows, self.vstats = z(Tn, 4, dtype=torch.float32), z(8, dtype=torch.float32)
                self.value_index = z(T.value_index_slots(Tn, value.level, S), dtype=torch.int32)
                self.value_count = z(1, dtype=torch.int32)
        self.cos, self.sin = rope_tables(d.head_dim, d.max_pos, d.rope_theta, dev)
        # ---- backward scratch ----
        self.dlogits = z(Tn, V)
        rres = max(R_(L0.down_w), R_(L0.o_w))                  # dx / dx2 are the dy of down_proj and o_proj
        self.dxa, self.dxb, self.dh, self.dao = za(Tn, D, rres), za(Tn, D, rres), z(Tn, D), za(Tn, D, R_(L0.o_w))
        self.dqkv, self.dgu, self.dact = za(Tn, 3 * D, R_(L0.qkv_w)), za(Tn, 2 * I, R_(L0.gu_w)), z(Tn, I)
        self.dp3, self.dz2, self.dz1 = za(B * 256, D, R_(weights.fc3_w)), za(B * 256, D, R_(weights.fc2_w)), za(B * 256, Pv, R_(weights.fc1_w))
        self.dp2, self.dp1 = z(B * 256, D), z(B * 256, Pv)
        towers = (weights.dino, weights.siglip) if self.train_vision else ()
        mv = max((B * tw.dims.tokens for tw in towers), default=0)
        dv_ = max((tw.dims.dim for tw in towers), default=0)
        norm_ws = z(max(((Tn + 15) // 16) * D, 2 * ((mv + 15) // 16) * dv_), dtype=torch.float32)
        col_ws = z(max(((Tn + 31) // 32) * max(Pv, D), 256 * dv_, ((mv + 15) // 16) * dv_ * 4), dtype=torch.float32)
        self._frozen_dw = z(2 * max(D, Pv, dv_), dtype=torch.float32)         # sink for vector grads of frozen tensors
        self.dfeats = z(B * 256, d.vision_dim) if self.train_vision else None
        self.vis = [self._alloc_tower(tw) for tw in towers]
        # ---- the scratch ops bind at plan time; the linears' own buffers and weight layouts ----
        main = ScratchSet(torch.empty(64 << 20, dtype=torch.uint8, device=dev), col_ws, norm_ws,
                          z(8 << 20, dtype=torch.float32) if lora is not None else None)
        self.scratch = Scratch(main, main)
        self.lin.allocate(max(V, 3 * D, 2 * I, Pv) * ((Tn + 63) // 64 * 64), fp8, refresh_adapted)
        # execution order of the vision units (forward; the backward visits each tower's blocks top down, then its stem)
        vkey = lambda tw, i: f"vision.{tw.dims.prefix.split('.')[1]}." + ("stem" if i < 0 else f"block{i:02d}")
        self._vkey = vkey
        self._vseq_fwd = [vkey(tw, i) for tw in towers for i in range(-1, tw.dims.n_run)]
        self._vseq_bwd = [vkey(tw, i) for tw in towers for i in list(range(tw.dims.n_run - 1, -1, -1)) + [-1]]
        # The two towers are independent between the pixels and the projector (forward) and between the projector's input
        # gradient and their own weight gradients (backward): with un-sharded parameters the second tower's plans run on a
        # side stream inside the same graph, as in the inference engine — their K ≈ 1 K GEMMs pay ≈ 14 µs of launch + ramp +
        # epilogue per 25 µs main loop and fill 130–270 of 256 CUs. (The backward only on one GPU: with ranks to reduce over
        # it is issued bucket by bucket on one stream, see backward().) The side tower gets its own scratch (split-K
        # workspace, column-sum / norm / adapter-gradient partials); activations and gradients are per tower anyway. With
        # sharded parameters, fp8 or LoRA dropout the plans stay one list. BL_TRAIN_VISION_STREAMS=0: single stream (A/B).
        self._vis2 = (self.train_vision and len(towers) == 2 and not shard_params and not fp8
                      and (lora is None or lora.dropout == 0.0)      # the dropout buffers serve one adapted linear at a time
                      and os.environ.get("BL_TRAIN_VISION_STREAMS", "1") != "0")
        self._vis_stream = torch.cuda.Stream(device=dev) if self._vis2 else None
        if self._vis2:
            self.scratch.side = main.like()
        self.vision_forward_ops: List[Op] = []
        self._vfwd_tower: List[List[Op]] = []
        for ti, (tw, sv, col) in enumerate(zip(towers, self.vis, (0, d.dino.dim))):
            self._vfwd_tower.append(self._plan_tower_forward(tw, col, sv, self.scratch.side if ti else main))
            self.vision_forward_ops += self._vfwd_tower[-1]
        self.forward_ops = self._plan_forward()
        if self.policy is not None and self.policy.rollout_is_cap is not None:
            # the self-proximal forward: the same ops with the loss op given no proximal input. Both plans are fixed here;
            # `set_policy_batch` only says which one `forward()` runs, and each keeps its own captured graph
            at = next(i for i, op in enumerate(self.forward_ops) if op.name == "bl_policy_loss_is_f32")
            self.forward_ops_self = self.forward_ops[:at] + [self._policy_loss_op(self_proximal=True)] + self.forward_ops[at + 1:]
        self._ready: List[Tuple[int, str]] = []      # (number of backward ops enqueued, bucket key complete at that point)
        self.backward_ops = self._plan_backward()
        self.repack_ops = self._plan_repack()
        self._graphs: Dict[str, torch.cuda.CUDAGraph] = {}
        self._comm_stream = torch.cuda.Stream(device=dev) if (self.comm.active or shard_params) else None
        if self.pools is not None:
            self.pools.start(self._comm_stream, reduce_dtype)

    def materialize_params(self) -> None:
        """Bring every parameter-sharded unit back into the model's own allocation (UnitPools.materialize_params); this
        step object cannot train afterwards."""
        if self.pools is not None:
            self.pools.materialize_params()

    def _planning(self, key: str):
        """Around the backward ops of unit `key`: a parameter-sharded unit's slot views are looked up under its name."""
        return self.pools.planning(key) if self.pools is not None and key in self.pools.units else contextlib.nullcontext()

    def _seq(self, seq: List[str], j: int, backward: bool, body: List[Op]) -> List[Op]:
        """Ops of unit seq[j], inside its gather / release / flush protocol when it is parameter-sharded (UnitPools.seq)."""
        return body if self.pools is None else self.pools.seq(seq, j, backward, body)

    def _gvec(self, name: str, n: int) -> torch.Tensor:
        """fp32 gradient slot of a vector parameter, or a scratch sink when it is frozen."""
        return self.store.grad_view(name) if self.store.trainable(name) else self._frozen_dw[:n]

    def _bias_grad(self, sc: ScratchSet, dy: torch.Tensor, name: str) -> List[Op]:
        """Bias gradient = column sums of dy; nothing when the bias is frozen."""
        return [T.colsum(dy, self.store.grad_view(name), sc.col_ws, run=False)] if self.store.trainable(name) else []

    # ---- plans --------------------------------------------------------------------------------------------------
    def _plan_forward(self) -> List[Op]:
        d, w, B, S, D, sc = self.dims, self.w, self.B, self.S, self.dims.llm_dim, self.scratch.main
        plan: List[Op] = []
        head =self.pools is not None and "projector" in self.pools.units          # the head pool is parameter-sharded: projector, token embeddings, lm_head
        if head:                                   # lm_head keeps its slot (both layouts) from here to its dgrad in the backward pass
            plan += [self.pools.gather("projector"), self.pools.gather("llm.lm_head", both=True), self.pools.await_("projector")]
        # projector with the pre-activations kept (modeling_prismatic.py:151-156)
        plan += self.lin.forward_act(sc, self.feats, w.fc1_w, self.z1, self.p1, "gelu", bias=w.fc1_b)
        plan += self.lin.forward_act(sc, self.p1, w.fc2_w, self.z2, self.p2, "gelu", bias=w.fc2_b)
        plan += self.lin.forward(sc, self.p2, w.fc3_w, self.p3, EPI_BIAS, bias=w.fc3_b)
        if head:                                   # the embeddings share the projector's slot: gathered once it is released
            assert self.pools.slot("llm.embed") is self.pools.slot("projector") and self.pools.slot("llm.lm_head") is not self.pools.slot("projector")
            plan += [self.pools.release("projector"), self.pools.gather("llm.embed")]
        plan.append(T.map_rows(self.p3, self.x[0], rows=B * 256, group=256, stride=S, offset=1, scatter=True, run=False))
        if head:
            plan.append(self.pools.await_("llm.embed"))
        plan.append(ops.embed_splice(self.input_ids, w.embed, self.x[0].view(B, S, D), d.n_patches, run=False))
        if head:
            plan.append(self.pools.release("llm.embed"))
        lseq = [f"llm.layer{l:02d}" for l in range(d.llm_layers)]
        for l in range(d.llm_layers):      # sharded: the next layer's gather runs under this layer's compute
            plan += self._seq(lseq, l, False, self._layer_forward(l))
        if head:
            plan.append(self.pools.await_("llm.lm_head"))
        plan += [ops.rmsnorm(self.x[-1], w.norm, self.hn, d.rms_eps, run=False),
                 self.lin.gemm(sc, self.hn, w.lm_head, self.logits, EPI_F32_BF16R)]
        if self.preference is not None:
            plan.append(T.preference_loss(self.logits, self.targets, self.pair,
                                          None if self.preference.reference_free else self.ref_logprob, self.row_stats,
                                          self.stats, self.pair_stats_buf, self.seq_stats_buf, self.preference, group_rows=self.S,
                                          n_pairs=self.n_pairs, ignore_index=IGNORE_INDEX, run=False))
        elif self.distill is not None:
            plan.append(T.distill_loss(self.logits, self.targets, self.teacher, self.row_stats, self.stats, self.distill,
                                       IGNORE_INDEX, run=False))
        elif self.policy is None:
            plan.append(ops.cross_entropy(self.logits, self.targets, self.row_loss, self.mean_cnt, IGNORE_INDEX, run=False))
        else:
            plan.append(self._policy_loss_op())
            if self.value is not None:
                vh = self.value_head
                plan.append(T.value_head(self.hn, self.targets, vh.weight, vh.bias, self.returns,
                                         self.old_values if self.value.clip is not None else None, self.value, self.value_index,
                                         self.value_count, self.value_rows, self.vstats, policy_stats=self.stats, group_rows=S,
                                         ignore_index=IGNORE_INDEX, run=False))
        return plan

    def _policy_loss_op(self, self_proximal: bool = False) -> Op:
        """The forward's policy-loss op. With the rollout correction it is bl_policy_loss_is_f32, given the proximal
        log-probabilities or (`self_proximal`) none; otherwise the op of the level, as ever."""
        corrected = self.policy.rollout_is_cap is not None
        extra = dict(behaviour_logprob=self.behaviour_logprob, is_rows=self.is_rows, is_stats=self.is_stats) if corrected else {}
        return T.policy_loss(self.logits, self.targets, self.advantages, None if self_proximal else self.old_logprob,
                             self.ref_logprob if self.policy.kl_coef != 0.0 else None, self.row_stats, self.stats,
                             self.policy, IGNORE_INDEX, run=False, group_rows=self._group_rows,
                             group_stats=getattr(self, "group_stats", None), **extra)

    def _layer_forward(self, l: int, with_down: bool = True) -> List[Op]:
        """Forward ops of decoder layer l from its saved input x[l] (modeling_llama.py LlamaDecoderLayer). The backward
        plan replays them (without the down projection, whose output is x[l+1]) when activations are recomputed."""
        d, w, B, S = self.dims, self.w, self.B, self.S
        D, H, hd = d.llm_dim, d.llm_heads, d.head_dim
        lw, sc = w.layers[l], self.scratch.main
        lq, lo = self.qkv[0].stride(0), self.ao[0].stride(0)
        st, so = (S * lq, hd, lq), (S * lo, hd, lo)
        x, xm, qkv = self.x[l], self.xm[l], self.qkv[l]
        plan = [ops.rmsnorm(x, lw.ln1, self.h1[l], d.rms_eps, run=False)] + self.lin.forward(sc, self.h1[l], lw.qkv_w, qkv, EPI_NONE)
        if self.shared is None:
            plan += [T.rope(qkv, self.cos, self.sin, B=B, S=S, H=H, head_dim=hd, run=False),
                     T.attention_lse(qkv, qkv[:, D:], qkv[:, 2 * D:], self.ao[l], self.lse[l], B=B, H=H, Sq=S, Skv=S,
                                     head_dim=hd, q_strides=st, k_strides=st, v_strides=st, o_strides=so,
                                     causal=True, key_mask=self.key_mask, run=False)]
        else:                                  # a prompt row: prefix ‖ branches, every row at its own rotary position
            plan += [T.rope_pos(qkv, self.cos, self.sin, self.pos_rows, rows=B * S, H=H, head_dim=hd, run=False),
                     T.attention_tree_lse(qkv, qkv[:, D:], qkv[:, 2 * D:], self.ao[l], self.lse[l], B=B, H=H, S=S,
                                          prefix=self.shared.P0, branch=self.shared.nb, head_dim=hd, q_strides=st, k_strides=st,
                                          v_strides=st, o_strides=so, key_mask=self.key_mask, run=False)]
        plan += self.lin.forward(sc, self.ao[l], lw.o_w, xm, EPI_RES, res=x)
        plan += [ops.rmsnorm(xm, lw.ln2, self.h2[l], d.rms_eps, run=False)]
        plan += self.lin.forward_act(sc, self.h2[l], lw.gu_w, self.gu[l], self.act[l], "swiglu")
        if with_down:
            plan += self.lin.forward(sc, self.act[l], lw.down_w, self.x[l + 1], EPI_RES, res=xm)
        return plan

    def _plan_backward(self) -> List[Op]:
        d, w, B, S, st, sc = self.dims, self.w, self.B, self.S, self.store, self.scratch.main
        D, H, hd = d.llm_dim, d.llm_heads, d.head_dim
        lm = "language_model.model"
        plan: List[Op] = [T.cross_entropy_backward(self.logits, self.targets, self.mean_cnt, self.dlogits, IGNORE_INDEX, run=False)
                          if self._row_cfg is None else
                          T.distill_loss_backward(self.logits, self.targets, self.teacher, self.row_stats, self.stats, self.dlogits,
                                                  self.distill, IGNORE_INDEX, run=False)
                          if self.distill is not None else
                          T.policy_loss_backward(self.logits, self.targets, self.row_stats, self.stats, self.dlogits,
                                                 self.policy or self.preference.backward_config(), IGNORE_INDEX, run=False)]
        head = self.pools is not None and "projector" in self.pools.units
        if head:
            plan.append(self.pools.await_grad("llm.lm_head"))
        with self._planning("llm.lm_head"):
            plan += self.lin.wgrad(sc, self.dlogits, self.hn, w.lm_head)
            self._ready.append((len(plan), "llm.lm_head"))
            plan.append(self.lin.dgrad(sc, self.dlogits, w.lm_head, self.dh))
        if self.value is not None:                # + the value loss's gradient on the value rows of dh; dw, db of the head
            plan.append(T.value_head_backward(self.hn, self.value_head.weight, self.value_rows, self.value_index, self.value_count,
                                              st.grad_view("value_head.weight"), st.grad_view("value_head.bias")[:1],
                                              None if self.value.detach else self.dh, self.value, group_rows=S,
                                              inv_world=1.0 / self.world if self.comm.active else 1.0, run=False))
        if head:                                  # the projector's dgrad layouts travel under the whole decoder backward
            plan += [self.pools.release("llm.lm_head"), self.pools.flush("llm.lm_head"), self.pools.gather("projector", backward=True)]
        dx, dx2 = self.dxa, self.dxb
        plan.append(T.rmsnorm_backward(self.x[-1], w.norm, self.dh, dx, self._gvec(f"{lm}.norm.weight", D), sc.norm_ws,
                                       d.rms_eps, run=False))
        lq, lo = self.qkv[0].stride(0), self.ao[0].stride(0)
        assert self.dqkv.stride(0) == lq and self.dao.stride(0) == lo
        strides, so = (S * lq, hd, lq), (S * lo, hd, lo)
        stop_layer = self._lowest_needed_layer()
        lseq = [f"llm.layer{l:02d}" for l in range(d.llm_layers - 1, stop_layer - 1, -1)]
        for j, l in enumerate(range(d.llm_layers - 1, stop_layer - 1, -1)):
            lw, b = w.layers[l], f"{lm}.layers.{l}"
            body: List[Op] = []                # this layer's ops: one parameter-sharded unit
            with self._planning(lseq[j]):
                if self.recompute:     # incl. the top layer: the plan stays idempotent (graph capture runs it twice)
                    body += self._layer_forward(l, with_down=False)
                body += self.lin.backward_act(sc, dx, self.act[l], lw.down_w, self.gu[l], self.dgu, self.dact, "swiglu")
                body += self.lin.backward(sc, self.dgu, self.h2[l], lw.gu_w, self.dh)
                body.append(T.rmsnorm_backward(self.xm[l], lw.ln2, self.dh, dx2, self._gvec(f"{b}.post_attention_layernorm.weight", D),
                                               sc.norm_ws, d.rms_eps, dres=dx, run=False))
                body += self.lin.backward(sc, dx2, self.ao[l], lw.o_w, self.dao)
                qkv, dq = self.qkv[l], self.dqkv
                if self.shared is None:
                    body.append(T.attention_backward(qkv, qkv[:, D:], qkv[:, 2 * D:], self.ao[l], self.dao, self.lse[l], self.delta,
                                                     dq, dq[:, D:], dq[:, 2 * D:], B=B, H=H, Sq=S, Skv=S, head_dim=hd,
                                                     q_strides=strides, k_strides=strides, v_strides=strides,
                                                     o_strides=so, causal=True, key_mask=self.key_mask, run=False))
                    body.append(T.rope_backward(dq, self.cos, self.sin, B=B, S=S, H=H, head_dim=hd, run=False))
                else:
                    body.append(T.attention_tree_backward(qkv, qkv[:, D:], qkv[:, 2 * D:], self.ao[l], self.dao, self.lse[l],
                                                          self.delta, dq, dq[:, D:], dq[:, 2 * D:], B=B, H=H, S=S,
                                                          prefix=self.shared.P0, branch=self.shared.nb, head_dim=hd,
                                                          q_strides=strides, k_strides=strides, v_strides=strides, o_strides=so,
                                                          key_mask=self.key_mask, run=False))
                    body.append(T.rope_pos_backward(dq, self.cos, self.sin, self.pos_rows, rows=B * S, H=H, head_dim=hd, run=False))
                body += self.lin.backward(sc, dq, self.h1[l], lw.qkv_w, self.dh)
            plan += self._seq(lseq, j, True, body)             # sharded: the flush reduce-scatters and frees the gradient slot
            self._ready.append((len(plan), lseq[j]))
            plan.append(T.rmsnorm_backward(self.x[l], lw.ln1, self.dh, dx, self._gvec(f"{b}.input_layernorm.weight", D),
                                           sc.norm_ws, d.rms_eps, dres=dx2, run=False))
        if stop_layer > 0:
            return plan
        # dx = gradient of inputs_embeds [B, S, D]
        if st.trainable(f"{lm}.embed_tokens.weight"):
            if head:
                plan.append(self.pools.await_grad("llm.embed"))
            plan.append(T.fill_zero(st.grad_view(f"{lm}.embed_tokens.weight"), run=False))     # accumulated with atomics
            plan.append(T.embed_backward(self.input_ids, dx.view(B, S, D), st.grad_view(f"{lm}.embed_tokens.weight").view(d.vocab, D),
                                         d.n_patches, run=False))
            if head:
                plan.append(self.pools.flush("llm.embed"))
        if head:
            plan += [self.pools.await_("projector"), self.pools.await_grad("projector")]
        if st.trainable("projector.fc3.weight") or self.lora is not None:
            plan.append(T.map_rows(dx, self.dp3, rows=B * 256, group=256, stride=S, offset=1, scatter=False, run=False))
            with self._planning("projector"):
                plan += self._bias_grad(sc, self.dp3, "projector.fc3.bias")
                plan += self.lin.backward_act(sc, self.dp3, self.p2, w.fc3_w, self.z2, self.dz2, self.dp2, "gelu")
                plan += self._bias_grad(sc, self.dz2, "projector.fc2.bias")
                plan += self.lin.backward_act(sc, self.dz2, self.p1, w.fc2_w, self.z1, self.dz1, self.dp1, "gelu")
                plan += self._bias_grad(sc, self.dz1, "projector.fc1.bias")
                plan += self.lin.backward(sc, self.dz1, self.feats, w.fc1_w, self.dfeats if self.train_vision else None)
            self._ready.append((len(plan), "projector"))
            if head:
                plan += [self.pools.release("projector"), self.pools.flush("projector")]
            if self.train_vision:
                self._bwd_tower_at = [len(plan)]                   # [start of tower 0, start of tower 1]: see _vis2
                for ti, (tw, sv, col) in enumerate(zip((w.dino, w.siglip), self.vis, (0, d.dino.dim))):
                    if ti:
                        self._bwd_tower_at.append(len(plan))
                    plan += self._plan_tower_backward(tw, col, sv, len(plan), self.scratch.side if ti else sc)
        return plan

    # ---- vision towers in training form (timm VisionTransformer blocks) ---------------------------
    def _alloc_tower(self, tw) -> dict:
        t, B = tw.dims, self.B
        M, Dm, Hp, n = B * t.tokens, t.dim, t.mlp_pad, t.n_run
        z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype, device=self.device)
        pad = (t.tokens + 31) // 32 * 32
        ls = t.layerscale
        za, R_, b0 = self._za, self._R, tw.blocks[0]
        rr = max(R_(b0.fc2_w), R_(b0.proj_w))                  # dx / dx2 / du are the dy of fc2 and proj
        return dict(
            x=[z(M, Dm) for _ in range(n + 1)], h1=[za(M, Dm, R_(b0.qkv_w)) for _ in range(n)], qkv=[za(M, 3 * Dm, R_(b0.qkv_w)) for _ in range(n)],
            ao=[za(M, Dm, R_(b0.proj_w)) for _ in range(n)], lse=[z(B * t.heads * pad, dtype=torch.float32) for _ in range(n)],
            xm=[z(M, Dm) for _ in range(n)], h2=[za(M, Dm, R_(b0.fc1_w)) for _ in range(n)], zz=[z(M, Hp) for _ in range(n)],
            f=[za(M, Hp, R_(b0.fc2_w)) for _ in range(n)], u1=[z(M, Dm) if ls else None for _ in range(n)],
            u2=[z(M, Dm) if ls else None for _ in range(n)], delta=z(B * t.heads * pad, dtype=torch.float32),
            dxa=za(M, Dm, rr), dxb=za(M, Dm, rr), dh=z(M, Dm), du=za(M, Dm, rr), dao=za(M, Dm, R_(b0.proj_w)), dqkv=za(M, 3 * Dm, R_(b0.qkv_w)),
            df=z(M, Hp), dz=za(M, Hp, R_(b0.fc1_w)),
            dpe=z(B * 256, Dm), tok=z(max(t.n_prefix, 1) * Dm, dtype=torch.float32))

    def _plan_tower_forward(self, tw, feat_col: int, sv: dict, sc: ScratchSet) -> List[Op]:
        t, B, eps = tw.dims, self.B, self.dims.ln_eps
        Tk, Dm, hd = t.tokens, t.dim, t.head_dim
        col = self._vis.vbuf[1 if feat_col else 0]["col"]          # one im2col buffer per tower (kept for the patch wgrad)
        x0 = sv["x"][0]
        seq, j0 = self._vseq_fwd, self._vseq_fwd.index(self._vkey(tw, -1))
        whole: List[Op] = []                       # the tower's plan; `plan` below collects one unit's ops at a time
        plan = [ops.im2col_patch14(self.pixel_values, t.chan0, col, run=False)]
        if tw.prefix is not None:
            plan.append(ops.write_prefix_tokens(tw.prefix, x0, B, Tk, run=False))
        plan.append(self.lin.gemm(sc, col, tw.patch_w, x0, ops.EPI_BIAS_RES, bias=tw.patch_b, res=tw.pos, res_row_mod=256,
                      out_map=(256, Tk, t.n_prefix)))
        whole += self._seq(seq, j0, False, plan)
        lq, lo = sv["qkv"][0].stride(0), sv["ao"][0].stride(0)
        st, so = (Tk * lq, hd, lq), (Tk * lo, hd, lo)
        for i, b in enumerate(tw.blocks):
            if i:
                whole += self._seq(seq, j0 + i, False, plan)
            x, xm, qkv = sv["x"][i], sv["xm"][i], sv["qkv"][i]
            plan = [ops.layernorm(x, b.norm1_w, b.norm1_b, sv["h1"][i], eps, run=False)]
            plan += self.lin.forward(sc, sv["h1"][i], b.qkv_w, qkv, EPI_BIAS, bias=b.qkv_b)
            plan += [T.attention_lse(qkv, qkv[:, Dm:], qkv[:, 2 * Dm:], sv["ao"][i], sv["lse"][i], B=B, H=t.heads, Sq=Tk,
                                     Skv=Tk, head_dim=hd, q_strides=st, k_strides=st, v_strides=st,
                                     o_strides=so, causal=False, run=False)]
            if b.ls1 is not None:
                plan += self.lin.forward(sc, sv["ao"][i], b.proj_w, sv["u1"][i], EPI_BIAS, bias=b.proj_b)
                plan.append(T.scale_residual(sv["u1"][i], b.ls1, x, xm, run=False))
            else:
                plan += self.lin.forward(sc, sv["ao"][i], b.proj_w, xm, ops.EPI_BIAS_RES, bias=b.proj_b, res=x)
            plan.append(ops.layernorm(xm, b.norm2_w, b.norm2_b, sv["h2"][i], eps, run=False))
            plan += self.lin.forward_act(sc, sv["h2"][i], b.fc1_w, sv["zz"][i], sv["f"][i], "gelu", bias=b.fc1_b)
            if b.ls2 is not None:
                plan += self.lin.forward(sc, sv["f"][i], b.fc2_w, sv["u2"][i], EPI_BIAS, bias=b.fc2_b)
                plan.append(T.scale_residual(sv["u2"][i], b.ls2, xm, sv["x"][i + 1], run=False))
            else:
                plan += self.lin.forward(sc, sv["f"][i], b.fc2_w, sv["x"][i + 1], ops.EPI_BIAS_RES, bias=b.fc2_b, res=xm)
        whole += self._seq(seq, j0 + len(tw.blocks), False, plan)
        # tap: patch rows of the last block output → this tower's channels of the fused feature map
        whole.append(T.map_rows(sv["x"][-1], self.feats[:, feat_col:feat_col + Dm], rows=B * 256, group=256, stride=Tk,
                                offset=t.n_prefix, scatter=False, run=False))
        return whole

    def _plan_tower_backward(self, tw, feat_col: int, sv: dict, base: int, sc: ScratchSet) -> List[Op]:
        """`base` = ops already in the backward plan (bucket-ready markers are absolute positions)."""
        t, B, eps, st = tw.dims, self.B, self.dims.ln_eps, self.store
        Tk, Dm, hd, M = t.tokens, t.dim, t.head_dim, B * t.tokens
        p = t.prefix
        tower_key = p.split(".")[1]
        gv = lambda name: self._gvec(name, Dm)
        gb = lambda name: st.grad_view(name) if st.trainable(name) else self._frozen_dw[Dm:2 * Dm]   # 2nd sink: LN dw + db
        dx, dx2 = sv["dxa"], sv["dxb"]
        seq, j0 = self._vseq_bwd, self._vseq_bwd.index(self._vkey(tw, t.n_run - 1))
        whole: List[Op] = [T.fill_zero(self._wide.get(dx.data_ptr(), dx), run=False),
                           T.map_rows(self.dfeats[:, feat_col:feat_col + Dm], dx, rows=B * 256, group=256, stride=Tk,
                                      offset=t.n_prefix, scatter=True, run=False)]
        lq, lo = sv["qkv"][0].stride(0), sv["ao"][0].stride(0)
        assert sv["dqkv"].stride(0) == lq and sv["dao"].stride(0) == lo
        strides, so = (Tk * lq, hd, lq), (Tk * lo, hd, lo)
        for i in range(t.n_run - 1, -1, -1):
            b, bn = tw.blocks[i], f"{p}.blocks.{i}"
            dbr = dx
            plan: List[Op] = []                    # this block's ops: one parameter-sharded unit
            with self._planning(self._vkey(tw, i)):
                if b.ls2 is not None:
                    plan.append(T.layerscale_backward(dx, sv["u2"][i], b.ls2, sv["du"], gv(f"{bn}.ls2.scale_factor"), sc.col_ws, run=False))
                    dbr = sv["du"]
                plan += self._bias_grad(sc, dbr, f"{bn}.mlp.fc2.bias")
                plan += self.lin.backward_act(sc, dbr, sv["f"][i], b.fc2_w, sv["zz"][i], sv["dz"], sv["df"], "gelu")
                plan += self._bias_grad(sc, sv["dz"][:, :t.mlp], f"{bn}.mlp.fc1.bias")
                plan += self.lin.backward(sc, sv["dz"], sv["h2"][i], b.fc1_w, sv["dh"])
                plan.append(T.layernorm_backward(sv["xm"][i], b.norm2_w, sv["dh"], dx2, gv(f"{bn}.norm2.weight"), gb(f"{bn}.norm2.bias"),
                                                 sc.norm_ws, eps, dres=dx, run=False))
                dbr = dx2
                if b.ls1 is not None:
                    plan.append(T.layerscale_backward(dx2, sv["u1"][i], b.ls1, sv["du"], gv(f"{bn}.ls1.scale_factor"), sc.col_ws, run=False))
                    dbr = sv["du"]
                plan += self._bias_grad(sc, dbr, f"{bn}.attn.proj.bias")
                plan += self.lin.backward(sc, dbr, sv["ao"][i], b.proj_w, sv["dao"])
                qkv, dq = sv["qkv"][i], sv["dqkv"]
                plan.append(T.attention_backward(qkv, qkv[:, Dm:], qkv[:, 2 * Dm:], sv["ao"][i], sv["dao"], sv["lse"][i], sv["delta"],
                                                 dq, dq[:, Dm:], dq[:, 2 * Dm:], B=B, H=t.heads, Sq=Tk, Skv=Tk, head_dim=hd,
                                                 q_strides=strides, k_strides=strides, v_strides=strides,
                                                 o_strides=so, causal=False, run=False))
                plan += self._bias_grad(sc, dq, f"{bn}.attn.qkv.bias")
                plan += self.lin.backward(sc, dq, sv["h1"][i], b.qkv_w, sv["dh"])
            whole += self._seq(seq, j0 + (t.n_run - 1 - i), True, plan)
            self._ready.append((base + len(whole), f"vision.{tower_key}.block{i:02d}"))
            whole.append(T.layernorm_backward(sv["x"][i], b.norm1_w, sv["dh"], dx, gv(f"{bn}.norm1.weight"), gb(f"{bn}.norm1.bias"),
                                              sc.norm_ws, eps, dres=dx2, run=False))
        # stem: dx = gradient of [prefix tokens | patch embeddings + pos]
        plan = []
        if st.trainable(f"{p}.pos_embed"):
            dxv = dx.view(B, Tk * Dm)
            plan.append(T.colsum(dxv[:, t.n_prefix * Dm:], st.grad_view(f"{p}.pos_embed"), sc.col_ws, run=False))
            if t.n_prefix:
                plan.append(T.colsum(dxv[:, :t.n_prefix * Dm], sv["tok"], sc.col_ws, run=False))
                plan.append(T.copy_f32(sv["tok"][:Dm], st.grad_view(f"{p}.cls_token"), run=False))
                plan.append(T.copy_f32(sv["tok"][Dm:t.n_prefix * Dm], st.grad_view(f"{p}.reg_token"), run=False))
            plan.append(T.map_rows(dx, sv["dpe"], rows=B * 256, group=256, stride=Tk, offset=t.n_prefix, scatter=False, run=False))
            plan += self._bias_grad(sc, sv["dpe"], f"{p}.patch_embed.proj.bias")
            with self._planning(self._vkey(tw, -1)):
                plan += self.lin.wgrad(sc, sv["dpe"], self._vis.vbuf[1 if feat_col else 0]["col"], tw.patch_w)
        whole += self._seq(seq, j0 + t.n_run, True, plan)
        self._ready.append((base + len(whole), f"vision.{tower_key}.stem"))
        return whole

    def _lowest_needed_layer(self) -> int:
        """Backward stops above the lowest decoder layer that still has a trainable tensor below or inside it."""
        names = self.store.names
        if self.lora is not None:
            return 0
        if any(not n.startswith("language_model.model.layers.") and not n.startswith("language_model.lm_head")
               and not n.startswith("language_model.model.norm") for n in names):
            return 0                     # embeddings / projector / vision sit under layer 0
        lows = [int(n.split(".")[3]) for n in names if n.startswith("language_model.model.layers.")]
        return min(lows) if lows else self.dims.llm_layers

    def _plan_repack(self) -> List[Op]:
        """After AdamW wrote the bf16 copy of every group's logical matrix: refresh the forward and the dgrad layouts."""
        plan: List[Op] = []
        st = self.store
        # plain tensors (norm scales, biases, embeddings, LoRA adapters): updated bf16 values → the live tensors, as prepared
        # byte copies inside the plan (hundreds of them under LoRA: replayed with the graph instead of launched one by one)
        # ONE bl_batched_ops launch for the write-backs of the plain tensors and the re-packs of the GEMM weights (independent of
        # each other: all read the optimizer's bf16 staging copy) — ≈ 800 launches of the full fine-tune's plan, ≈ 700 of LoRA's
        entries = []
        for u in st.units:
            if u.group is None and st.layout.buckets[u.bucket].key not in st.sharded_keys:
                assert u.dst.is_contiguous()
                entries.append(T.be_copy(st.stage_view(u.offset, u.numel), u.dst))
        for u in st.units:
            if u.group is None or st.layout.buckets[u.bucket].key in st.sharded_keys:
                continue                                          # parameter-sharded units are packed when gathered
            n, k = u.group.n, u.group.k
            rm = st.stage_view(u.offset, u.numel).view(n, k)
            entries.append(T.be_pack(rm, u.group.packed))
            plan += self.lin.repack_ops(rm, u.group.packed, entries)
        if entries:
            plan.insert(0, T.batched(entries, self.device, run=False))
        plan += self.lin.adapter_ops                           # LoRA: adapter columns of the K-concatenated weights
        return plan

    # ---- running ------------------------------------------------------------------------------------------------
    def set_batch(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], pixel_values: torch.Tensor,
                  labels: torch.Tensor) -> None:
        """Right-padded batch (PaddedCollatorForActionPrediction, data_utils.py:101-142) → static device inputs. Batches
        shorter than the planned L are padded further (pad id 32000 / mask 0 / label -100: no effect on valid rows)."""
        self._set_text_batch(input_ids, attention_mask, labels)
        self.pixel_values.copy_(pixel_values.to(self.device).to(torch.bfloat16))

    def set_batch_frames(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], frames_u8: torch.Tensor,
                         labels: torch.Tensor, aug_params=None) -> None:
        """`set_batch` for raw uint8 RGB frames [B, H, W, 3] (host or device): they are uploaded as uint8 and the static
        `pixel_values` buffer is filled on the device. Without `aug_params` this is `preprocess_frames_gpu` alone (resize
        included), bit-identical to `set_batch` with the host `apply_transform` of the same frames. With `aug_params`
        ([B, 8] fp32, vla/image_augment.py::draw_params) the frames are resized first if needed, then augmented and
        normalised in one fused op (bl_augment_frames_u8)."""
        if (not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3
                or frames_u8.shape[0] != self.B):
            raise ValueError(f"set_batch_frames: expected uint8 frames [{self.B}, H, W, 3]")
        self._set_text_batch(input_ids, attention_mask, labels)
        frames = frames_u8.to(self.device).contiguous()
        proc = self._frames_processor()
        if aug_params is None:
            proc.preprocess_frames_gpu(frames, out=self.pixel_values)
            return
        h, w = self.pixel_values.shape[-2:]
        if tuple(frames.shape[1:3]) != (h, w):
            frames = ops.resize_bicubic_u8(frames, h, w)
        params = aug_params if torch.is_tensor(aug_params) else torch.from_numpy(np.ascontiguousarray(aug_params, dtype=np.float32))
        params = params.to(frames.device, dtype=torch.float32).contiguous()
        if self._aug_workspace is None:
            self._aug_workspace = torch.empty(self.B, 3, dtype=torch.int64, device=frames.device)
        ops.augment_frames_u8(frames, params, pixel_values=self.pixel_values, mean_std=proc.mean_std(frames.device),
                              workspace=self._aug_workspace)

    _aug_workspace: Optional[torch.Tensor] = None
    _image_processor = None

    def _frames_processor(self):
        """The image processor whose normalisation constants the frames path uses (OpenVLA's fused-backbone defaults)."""
        if self._image_processor is None:
            from ..extern.hf.processing_prismatic import PrismaticImageProcessor
            self._image_processor = PrismaticImageProcessor()
        return self._image_processor

    def _set_text_batch(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], labels: torch.Tensor) -> None:
        if self.shared is not None:
            return self._set_text_batch_shared(input_ids, attention_mask, labels)
        dev, B, L, P, S = self.device, self.B, self.L, self.dims.n_patches, self.S
        b, l = input_ids.shape
        if b != B or l > L:
            raise ValueError(f"batch {tuple(input_ids.shape)} does not fit the planned step ({B}, <= {L})")
        ids = torch.full((B, L), 32000, dtype=torch.int64, device=dev)
        ids[:, :l] = input_ids.to(dev)
        m = torch.zeros(B, L, dtype=torch.uint8, device=dev)
        m[:, :l] = (attention_mask.to(dev) if attention_mask is not None else torch.ones(b, l, device=dev)).to(torch.uint8)
        lab = torch.full((B, L), IGNORE_INDEX, dtype=torch.int64, device=dev)
        lab[:, :l] = labels.to(dev)
        self.input_ids.copy_(ids)
        self.key_mask[:, :1] = m[:, :1]
        self.key_mask[:, 1:1 + P] = 1
        self.key_mask[:, 1 + P:] = m[:, 1:]
        if self._row_cfg is not None and self._row_cfg.token_range is not None:
            first, count = self._row_cfg.token_range
            outside = (lab != IGNORE_INDEX) & ((lab < first) | (lab >= first + count))
            if bool(outside.any()):
                raise ValueError(f"labels: {int(outside.sum())} labelled token(s) outside {self.loss_kind}.token_range [{first}, {first + count}): "
                                 "that action has probability 0 under the restricted policy — draw rollouts with "
                                 "action_tokens_only=True")
        self.targets.copy_(shift_to_rows(lab, P, IGNORE_INDEX).view(-1))
        if self._row_cfg is not None:
            self._batch_len = l
        if self.preference is not None:         # the pair assignment belongs to a batch: the next one brings its own
            self.pair.zero_()
            self._pairs_set = False
        if self.distill is not None:            # the teacher belongs to a batch too
            self._teacher_set = False

    def _set_text_batch_shared(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], labels: torch.Tensor) -> None:
        """`_set_text_batch` of the shared-prompt step: the batch [B, l] is laid out by training/shared_prompt.py::plan_batch
        (which raises before anything here is written) and the static ids / key mask / targets / positions are filled."""
        sb = SP.plan_batch(self.shared, input_ids, attention_mask, labels)
        if self._row_cfg is not None and self._row_cfg.token_range is not None:
            first, count = self._row_cfg.token_range
            lab = sb.targets[sb.targets != IGNORE_INDEX]
            outside = (lab < first) | (lab >= first + count)
            if bool(outside.any()):
                raise ValueError(f"labels: {int(outside.sum())} labelled token(s) outside {self.loss_kind}.token_range [{first}, {first + count}): "
                                 "that action has probability 0 under the restricted policy — draw rollouts with "
                                 "action_tokens_only=True")
        if int(sb.pos.max()) >= self.cos.shape[0]:
            raise ValueError(f"shared_prompt: position {int(sb.pos.max())} exceeds the model's {self.cos.shape[0]} (model_max_length)")
        dev = self.device
        self.input_ids.copy_(torch.from_numpy(sb.ids).to(dev))
        self.key_mask.copy_(torch.from_numpy(sb.key_mask).to(dev))
        self.targets.copy_(torch.from_numpy(sb.targets).to(dev))
        self.pos_rows.copy_(torch.from_numpy(sb.pos).to(dev))
        self._token_row = sb.token_row
        if self._row_cfg is not None:
            self._batch_len = input_ids.shape[1]

    def _from_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """Per-row values [T] of the last forward → [B, l] aligned with the labels of the last `set_batch` (0 off them)."""
        if self.shared is not None:
            return SP.rows_to_tokens(self._token_row, rows)
        return shift_from_rows(rows.view(self.B, self.S), self.dims.n_patches)[:, :self._batch_len]

    def set_policy_batch(self, advantages: torch.Tensor, old_logprobs: Optional[torch.Tensor], ref_logprobs: Optional[torch.Tensor] = None,
                         behaviour_logprobs: Optional[torch.Tensor] = None) -> None:
        """Per-token inputs of loss="policy", [B, l] aligned with the `labels` of the preceding `set_batch`: the advantage
        and the behaviour policy's log-probability of each labelled token, and a reference policy's (needed iff kl_coef is
        set). They get the padding, patch-column insertion and one-position shift the labels got; values on unlabelled
        positions are not read. Non-finite values on labelled positions raise ValueError (a -inf from `score_actions`
        under top-k / top-p: rollouts for training are drawn with temperature only).
        With the rollout correction (`policy.rollout_is_cap`) the sampler's log-probabilities go in as `behaviour_logprobs`
        (required), and `old_logprobs` are the PROXIMAL policy's — the learner's own `token_logprobs()` before the update —
        or None: self-proximal, the forward's own log-probabilities taken as constants, which needs no extra forward when
        a rollout is used for one update. The two are two forward plans built with the step, equal up to the loss op, each
        with its own captured graph; this call only selects which one `forward()` runs. Without the correction both of
        these raise ValueError."""
        if self.policy is None:
            raise RuntimeError("set_policy_batch needs TrainStep(loss='policy')")
        if (ref_logprobs is None) != (self.policy.kl_coef == 0.0):
            raise ValueError("ref_logprobs goes together with a non-zero kl_coef")
        corrected = self.policy.rollout_is_cap is not None
        if corrected != (behaviour_logprobs is not None):
            raise ValueError("behaviour_logprobs goes together with policy.rollout_is_cap (the rollout correction)")
        if old_logprobs is None and not corrected:
            raise ValueError("old_logprobs=None (self-proximal) needs policy.rollout_is_cap (the rollout correction)")
        valid = (self.targets != IGNORE_INDEX).view(self.B, self.S)
        for name, src, dst in (("advantages", advantages, self.advantages), ("old_logprobs", old_logprobs, self.old_logprob),
                               ("ref_logprobs", ref_logprobs, self.ref_logprob),
                               ("behaviour_logprobs", behaviour_logprobs, getattr(self, "behaviour_logprob", None))):
            if src is not None and self.shared is not None:
                dst.copy_(SP.tokens_to_rows(self._token_row, src, self.T, name).to(self.device))
            elif src is not None:
                tokens_to_rows(name, src, dst, self._batch_len, self.dims.n_patches, valid,
                               "on labelled positions — a token outside the rollout's top-k / top-p support scores -inf; draw "
                               "training rollouts with temperature only")
        if corrected:
            self._self_proximal = old_logprobs is None

    def set_value_batch(self, returns: torch.Tensor, old_values: Optional[torch.Tensor] = None) -> None:
        """The critic's targets for the batch of the preceding `set_batch`: the return R of each value position and the
        value the behaviour critic gave it (`values()` of a forward over the rollout batch before the update, as
        `token_logprobs()` supplies on-policy `old_logprobs`). At value.level "action" both are [B], one per sequence; at
        "token" they are [B, l] aligned with the labels, taking the path `set_policy_batch`'s inputs take. `old_values` is
        needed unless value.clip is None. Non-finite values where a value row reads them raise ValueError."""
        if self.value is None:
            raise RuntimeError("set_value_batch needs TrainStep(loss='policy', value=ValueLossConfig(...))")
        if (old_values is None) != (self.value.clip is None):
            raise ValueError("old_values goes together with value.clip (None only for the unclipped loss)")
        B = self.B
        valid = (self.targets != IGNORE_INDEX).view(B, self.S)
        for name, src, dst in (("returns", returns, self.returns), ("old_values", old_values, self.old_values)):
            if src is None:
                continue
            if self.value.level == "token":
                tokens_to_rows(name, src, dst, self._batch_len, self.dims.n_patches, valid, "on labelled positions")
                continue
            src = torch.as_tensor(src)          # one value row per sequence, found on the device: every row carries the sequence's
            if tuple(src.shape) != (B,):
                raise ValueError(f"{name}: shape {tuple(src.shape)}, expected {(B,)}")
            rows = src.to(self.device, dtype=torch.float32)[:, None].expand(B, self.S)
            bad = valid & ~torch.isfinite(rows)
            if bool(bad.any()):
                raise ValueError(f"{name}: {int(bad.any(dim=1).sum())} non-finite value(s) on sequences with a label")
            dst.copy_(torch.where(valid, rows, torch.zeros_like(rows)).reshape(-1))

    def values(self) -> torch.Tensor:
        """V of the last forward: [B] at value.level "action" (the value at each sequence's first labelled position; 0 for
        a sequence without one), [B, l] aligned with the labels at "token" (0 off the labels). This is how a learner values
        its rollout states for `rl.gae`, and where `old_values` come from."""
        if self.value is None:
            raise RuntimeError("values needs TrainStep(loss='policy', value=ValueLossConfig(...))")
        v = self.value_rows[:, 0].view(self.B, self.S)
        if self.value.level == "action":        # at most one non-zero per sequence: the sum is that value, exactly
            return v.sum(dim=1)
        return shift_from_rows(v, self.dims.n_patches)[:, :self._batch_len]

    def set_preference_batch(self, pair, ref_logprobs: Optional[torch.Tensor] = None) -> None:
        """The pair assignment of loss="preference" for the batch of the preceding `set_batch`: `pair` int [B] holds +k for
        a sequence on the chosen side of pair k, −k on the rejected side, 0 for one in no pair, with k dense in 1…P.
        `ref_logprobs` [B, l] are the reference policy's log-probabilities of the labelled tokens, aligned with the labels
        as `set_policy_batch` takes them (`score_actions(use_adapters=False)` through `rl.preference_batch`, or this
        step's own `token_logprobs()` before the first update); needed iff not `preference.reference_free`. ValueError
        for ids that are not dense, a pair without a labelled token on either side, or a non-finite reference on a
        labelled token of a paired sequence. P goes to the loss op through the device scalar `n_pairs`, so a captured
        graph serves any assignment."""
        if self.preference is None:
            raise RuntimeError("set_preference_batch needs TrainStep(loss='preference')")
        if (ref_logprobs is None) != self.preference.reference_free:
            raise ValueError("ref_logprobs is given unless preference.reference_free")
        B = self.B
        pr = torch.as_tensor(pair).detach().cpu()
        if pr.dim() != 1 or pr.shape[0] != B or pr.dtype.is_floating_point or pr.dtype == torch.bool:
            raise ValueError(f"pair: an integer vector [{B}], got {pr.dtype} {tuple(pr.shape)}")
        valid = (self.targets != IGNORE_INDEX).view(B, self.S)
        n_pairs = check_pairs(pr.to(torch.int64).numpy(), valid.sum(dim=1).cpu().numpy())
        if ref_logprobs is not None:
            tokens_to_rows("ref_logprobs", ref_logprobs, self.ref_logprob, self._batch_len, self.dims.n_patches, valid,
                           "on labelled positions of paired sequences — a token outside a top-k / top-p support scores -inf; "
                           "score the reference with temperature only", refuse=valid & (pr != 0).to(self.device)[:, None])
        self.pair.copy_(pr.to(torch.int32))
        self.n_pairs.fill_(n_pairs)
        self._pairs_set = True

    def set_distill_batch(self, teacher_probs) -> None:
        """The teacher of loss="distill" for the batch of the preceding `set_batch`: `teacher_probs` [B, l, count], one
        distribution over the token range (the vocabulary without one) per token position, aligned with the `labels` as
        `set_policy_batch`'s inputs are (`rl.distill_batch`, `rl.gaussian_bin_targets`). It takes the padding,
        patch-column insertion and one-position shift the labels took; rows on unlabelled positions are not read by a
        kernel and may hold anything. On labelled positions the teacher must be finite, >= 0, sum to 1 within 1e-3, and
        be > 0 everywhere under kind="reverse_kl": ValueError otherwise."""
        if self.distill is None:
            raise RuntimeError("set_distill_batch needs TrainStep(loss='distill')")
        valid = (self.targets != IGNORE_INDEX).view(self.B, self.S)
        tokens_to_rows("teacher_probs", teacher_probs, self.teacher, self._batch_len, self.dims.n_patches, valid,
                       "on labelled positions", check=lambda rows: check_teacher(rows[valid].double().cpu().numpy(),
                                                                                 np.ones(int(valid.sum()), dtype=bool),
                                                                                 self.distill.kind, "set_distill_batch"))
        self._teacher_set = True

    def distill_stats(self) -> Dict[str, torch.Tensor]:
        """The 8 step statistics of the last forward (distill_loss.DISTILL_STAT_NAMES) as device scalars."""
        return self._stats("distill_stats", self.distill is not None, "TrainStep(loss='distill')", DISTILL_STAT_NAMES, "stats")

    def _stats(self, reader: str, have: bool, needs: str, names, buf: str) -> Dict[str, torch.Tensor]:
        """{name: entry i along the last dimension of buffer `buf`} — device scalars for a vector of step statistics, device
        vectors for a per-sequence / per-pair table; RuntimeError when the step was built without what the reader `needs`."""
        if not have:
            raise RuntimeError(f"{reader} needs {needs}")
        return {name: getattr(self, buf).select(-1, i) for i, name in enumerate(names)}

    def value_stats(self) -> Dict[str, torch.Tensor]:
        """The 8 statistics of the value loss of the last forward (value_loss.VALUE_STAT_NAMES) as device scalars."""
        return self._stats("value_stats", self.value is not None, "TrainStep(loss='policy', value=ValueLossConfig(...))",
                           VALUE_STAT_NAMES, "vstats")

    def policy_stats(self) -> Dict[str, torch.Tensor]:
        """The 8 step statistics of the last forward (policy_loss.STAT_NAMES) as device scalars."""
        return self._stats("policy_stats", self.policy is not None, "TrainStep(loss='policy')", STAT_NAMES, "stats")

    def rollout_stats(self) -> Dict[str, torch.Tensor]:
        """The statistics of the rollout correction of the last forward (policy_loss.IS_STAT_NAMES) as device scalars: mean
        weight and mean π_prox/μ, the truncated and masked fractions, and the k3 / k1 estimates of KL(μ‖π_prox). Per rank."""
        return self._stats("rollout_stats", self.policy is not None and self.policy.rollout_is_cap is not None,
                           "TrainStep(loss='policy') with policy.rollout_is_cap", IS_STAT_NAMES, "is_stats")

    def token_weights(self) -> torch.Tensor:
        """The importance weight w of the last forward at the labelled positions, [B, l] aligned with `labels` (0
        elsewhere, and on masked tokens; the action's weight on each of its tokens at ratio_level="action"), shifted back
        as `token_logprobs()` is."""
        if self.policy is None or self.policy.rollout_is_cap is None:
            raise RuntimeError("token_weights needs TrainStep(loss='policy') with policy.rollout_is_cap")
        return self._from_rows(self.is_rows[:, 1])

    def action_stats(self) -> Dict[str, torch.Tensor]:
        """The per-sequence statistics of the last forward under policy.ratio_level="action" (policy_loss.GROUP_STAT_NAMES)
        as device tensors [B]: the action's log-ratio, its ratio, its number of labelled tokens and its log π."""
        stats = self._stats("action_stats", self.policy is not None and self.policy.ratio_level == "action",
                            "TrainStep(loss='policy') with policy.ratio_level='action'", GROUP_STAT_NAMES, "group_stats")
        if self.shared is not None:               # the groups are runs of nb rows: a sequence's is its branch
            stats = {name: t[self._branch_groups] for name, t in stats.items()}
        return stats

    def preference_stats(self) -> Dict[str, torch.Tensor]:
        """The 8 step statistics of the last forward (preference_loss.PREF_STAT_NAMES) as device scalars."""
        return self._stats("preference_stats", self.preference is not None, "TrainStep(loss='preference')", PREF_STAT_NAMES, "stats")

    def pair_stats(self) -> Dict[str, torch.Tensor]:
        """The per-pair statistics of the last forward (preference_loss.PAIR_STAT_NAMES) as device tensors [B // 2]; the
        entries from the batch's number of pairs on are 0."""
        return self._stats("pair_stats", self.preference is not None, "TrainStep(loss='preference')", PAIR_STAT_NAMES, "pair_stats_buf")

    def sequence_stats(self) -> Dict[str, torch.Tensor]:
        """The per-sequence statistics of the last forward (preference_loss.SEQ_STAT_NAMES) as device tensors [B]."""
        return self._stats("sequence_stats", self.preference is not None, "TrainStep(loss='preference')", SEQ_STAT_NAMES, "seq_stats_buf")

    def token_logprobs(self) -> torch.Tensor:
        """log π(token) of the last forward at the labelled positions, [B, l] aligned with `labels` (0 elsewhere): the row
        statistics shifted back. This is how a learner gets on-policy `old_logprobs`, or a frozen model's `ref_logprobs`,
        from the training forward itself."""
        if self._row_cfg is None:
            raise RuntimeError("token_logprobs needs TrainStep(loss='policy'), TrainStep(loss='preference') or TrainStep(loss='distill')")
        return self._from_rows(self.row_stats[:, 0])

    def _run_forked(self, main_ops: List[Op], side_ops: List[Op]) -> None:
        """main_ops on the current stream, side_ops on the vision side stream, joined at the end (fork / join with stream
        waits, which HIP-graph capture records as parallel branches)."""
        main = torch.cuda.current_stream()
        self._vis_stream.wait_stream(main)
        with torch.cuda.stream(self._vis_stream):
            ops.run_all(side_ops)
        ops.run_all(main_ops)
        main.wait_stream(self._vis_stream)

    def _replay(self, key: str, plan, graph: bool) -> None:
        if self.pools is not None and self.pools.materialized:
            raise RuntimeError("materialize_params() ended this step object's training (its plans address the gather slots)")
        run = plan if callable(plan) else (lambda: ops.run_all(plan))      # a callable issues its own (forked) launches
        if not graph or (self.shard_params and key in ("vfwd", "fwd", "fwd_self", "bwd")):      # per-unit collectives stay out of HIP graphs
            run()
            return
        gr = self._graphs.get(key)
        if gr is None:
            run()                                                  # warm (lazy hipFuncSetAttribute etc.) outside capture
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                run()
            self._graphs[key] = gr
        gr.replay()

    def forward(self, graph: bool = False) -> torch.Tensor:
        """Vision towers (frozen) → projector → decoder → loss. Returns the device scalar loss (with a critic: policy loss +
        value.coef · value loss, `value_stats()["total"]`)."""
        if self.lora is not None and self.lora.dropout > 0.0:
            self.lin.drop_seed.add_(1)            # a fresh mask per forward pass; the backward pass recomputes it from the same value
        if self.train_vision and self._vis2:
            self._replay("vfwd", lambda: self._run_forked(self._vfwd_tower[0], self._vfwd_tower[1]), graph)
        elif self.train_vision:
            self._replay("vfwd", self.vision_forward_ops, graph)
        else:
            self._vis.run_vision()
        if self.distill is not None and not self._teacher_set:
            raise RuntimeError("loss='distill': set_distill_batch comes after set_batch and before the forward pass")
        if getattr(self, "_self_proximal", False):
            self._replay("fwd_self", self.forward_ops_self, graph)
        else:
            self._replay("fwd", self.forward_ops, graph)
        return self.mean_cnt[0] if self.value is None else self.vstats[7]

    def backward(self, graph: bool = False) -> None:
        """Hand-written backward into the flat fp32 gradient buffer. Sharded runs (world > 1) issue each bucket's
        reduce-scatter on a side stream as soon as its last wgrad is enqueued (overlapping the rest of the backward)."""
        st, lay = self.store, self.store.layout
        if self.preference is not None and not self._pairs_set:
            raise RuntimeError("loss='preference': set_preference_batch comes after set_batch and before the backward pass")
        if self.distill is not None and not self._teacher_set:
            raise RuntimeError("loss='distill': set_distill_batch comes after set_batch and before the backward pass")
        if not self.comm.active:
            if self._vis2 and getattr(self, "_bwd_tower_at", None) and len(self._bwd_tower_at) == 2:
                a, b = self._bwd_tower_at
                bo = self.backward_ops
                self._replay("bwd", lambda: (ops.run_all(bo[:a]), self._run_forked(bo[a:b], bo[b:])), graph)
            else:
                self._replay("bwd", self.backward_ops, graph)
            if self.shard_params:                                  # the per-layer gradient flushes ran on the side stream
                torch.cuda.current_stream().wait_stream(self._comm_stream)
            return
        self.mean_cnt[1].mul_(self.world)                          # dlogits / world: the SUM over ranks is the DDP mean
        main = torch.cuda.current_stream()
        by_key = {b.key: b for b in lay.buckets}
        done, reduced = 0, set()

        def reduce(b):
            reduced.add(b.key)
            if b.key in st.sharded_keys:                           # reduced by the flush step inside the plan
                return
            self._comm_stream.wait_stream(main)
            with torch.cuda.stream(self._comm_stream):
                self.comm.reduce_scatter_bucket(st.grad_range(b.offset, b.numel), b, st.stage_view(b.offset, b.numel))
        for upto, key in self._ready:
            ops.run_all(self.backward_ops[done:upto])
            done = upto
            b = by_key.get(key) or by_key.get("lora." + key)
            if b is not None:
                reduce(b)
        ops.run_all(self.backward_ops[done:])
        for i in comm_order(lay.buckets):                          # whatever has no marker (plain tensors) goes last
            if lay.buckets[i].key not in reduced:
                reduce(lay.buckets[i])
        main.wait_stream(self._comm_stream)

    def accumulate(self, scale: float = 1.0) -> None:
        """Gradient accumulation: add scale × (this micro-batch's gradients) to the accumulator (allocated on first use).
        `use_accumulated()` then makes the accumulated sum the gradient the optimizer step sees."""
        st, lay = self.store, self.store.layout
        if getattr(st, "grad_acc", None) is None:
            st.grad_acc = torch.zeros(max(lay.local_total, 8), dtype=torch.float32, device=self.device)
        # after backward() every bucket's gradient is reduced over the ranks and this rank's slice is in place: the
        # accumulator holds slices only (1/world of the model), so accumulation works unchanged under the sharded optimizer
        for b in lay.buckets:
            o, n = lay.local_offset(b), lay.shard_numel(b)
            T.axpy(st.grad_acc[o:o + n], st.reduced_grad(b), scale)

    def use_accumulated(self) -> None:
        st, lay = self.store, self.store.layout
        for b in lay.buckets:               # D2D copies (plumbing); the accumulator is cleared for the next window
            o, n = lay.local_offset(b), lay.shard_numel(b)
            T.copy_f32(st.grad_acc[o:o + n], st.reduced_grad(b))
        T.fill_zero(st.grad_acc)

    def clip_grad_norm(self) -> torch.Tensor:
        """Global L2 norm over every trainable gradient + clip coefficient min(1, max_norm / (norm + 1e-6)), kept on
        the device (fsdp.py:238-240 → FSDP.clip_grad_norm_). Each rank sums its own slices; the partial sums are
        all-reduced. Returns the device scalar total norm."""
        st, lay, nb = self.store, self.store.layout, self.store.blocks_per_bucket
        for i, b in enumerate(lay.buckets):
            T.sumsq_partial(st.reduced_grad(b), st.partial[i * nb:(i + 1) * nb])
        self.comm.all_reduce_sum(st.partial)
        T.clip_coef(st.partial, self.max_grad_norm, st.norm_coef)
        return st.norm_coef[0]

    def optimizer_step(self, lr: float, graph: bool = False) -> None:
        """AdamW on this rank's slice of the fp32 masters (decay classes per fsdp.py:200-212), all-gather of the updated
        bf16 slices, re-pack into the forward / dgrad layouts."""
        st, lay = self.store, self.store.layout
        st.step_count += 1
        main = torch.cuda.current_stream()
        for i in comm_order(lay.buckets):
            b = lay.buckets[i]
            lo, hi = lay.shard_range(b)
            sl = slice(lay.local_offset(b), lay.local_offset(b) + hi - lo)
            sharded = b.key in st.sharded_keys                     # parameter-sharded: the rank's bf16 slice IS the parameter
            T.adamw(st.master[sl], st.m[sl], st.v[sl], st.reduced_grad(b), st.step_count, lr, betas=self.betas, eps=self.eps,
                    weight_decay=self.weight_decay if b.decay else 0.0, norm_coef=st.norm_coef,
                    p_bf16=st.own_slice(b) if sharded else st.stage_view(lo, hi - lo))
            if self.comm.active and not sharded:                   # gather bucket i while AdamW runs on bucket i+1
                self._comm_stream.wait_stream(main)
                with torch.cuda.stream(self._comm_stream):
                    self.comm.all_gather_params(st.stage_view(b.offset, b.numel), b)
        if self.comm.active:
            main.wait_stream(self._comm_stream)
        self._replay("repack", self.repack_ops, graph)
        if self.pools is not None:
            self.pools.params_updated.record(main)

    def step(self, lr: float, graph: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """forward → backward → clip → AdamW. Returns (loss, grad norm) as device scalars (no host sync here)."""
        loss = self.forward(graph)
        self.backward(graph)
        norm = self.clip_grad_norm()
        self.optimizer_step(lr, graph)
        return loss, norm


def shift_to_rows(values: torch.Tensor, n_patches: int, fill) -> torch.Tensor:
    """Per-token values [B, L] aligned with the text tokens → per-row values [B, L + n_patches] aligned with the logits rows:
    the patch columns are inserted behind the first token (filled with `fill`), and everything moves one position to the
    left, because position t predicts token t + 1 (the last row gets `fill`). The labels and the policy loss's per-token
    inputs all take this one path."""
    B, L = values.shape[:2]                   # a trailing dimension (a vector per token) rides along
    full = torch.full((B, L + n_patches) + tuple(values.shape[2:]), fill, dtype=values.dtype, device=values.device)
    full[:, :1] = values[:, :1]
    full[:, 1 + n_patches:] = values[:, 1:]
    out = torch.full_like(full, fill)
    out[:, :-1] = full[:, 1:]
    return out


def tokens_to_rows(name: str, src, dst: torch.Tensor, l: int, n_patches: int, select: torch.Tensor, where: str,
                   refuse: Optional[torch.Tensor] = None, check=None) -> None:
    """Per-token values `src` [B, l], aligned with the labels of a batch of l ≤ L tokens → `dst` [B·S] fp32, aligned with the
    logits rows (S = L + n_patches): padded to L with zeros, through `shift_to_rows`, zeroed outside the rows that `select`
    [B, S] marks, copied. A non-finite value on a row of `refuse` (default: `select`) is a ValueError that names the input and
    says `where`; the rows outside `select` are never read by a kernel, so what they hold does not matter.
    A `dst` [B·S, C] takes `src` [B, l, C] — a vector per token (the distillation teacher) — along the same path; `check`
    (optional) is called with the shifted rows [B, S, C] before anything is copied and raises what it has to."""
    B, S = select.shape
    src = torch.as_tensor(src)
    tail = tuple(dst.shape[1:])
    if tuple(src.shape) != (B, l) + tail:
        raise ValueError(f"{name}: shape {tuple(src.shape)}, expected {(B, l) + tail} (aligned with the labels of set_batch)")
    pad = torch.zeros((B, S - n_patches) + tail, dtype=torch.float32, device=dst.device)
    pad[:, :l] = src.to(dst.device, dtype=torch.float32)
    rows = shift_to_rows(pad, n_patches, 0.0)
    sel = lambda m: m.reshape(B, S, *([1] * len(tail)))
    bad = sel(select if refuse is None else refuse) & ~torch.isfinite(rows)
    if bool(bad.any()):
        raise ValueError(f"{name}: {int(bad.sum())} non-finite value(s) {where}")
    if check is not None:
        check(rows)
    dst.copy_(torch.where(sel(select), rows, torch.zeros_like(rows)).view(dst.shape))


def shift_from_rows(rows: torch.Tensor, n_patches: int) -> torch.Tensor:
    """Inverse of `shift_to_rows` on the text positions: per-row values [B, S] → per-token values [B, S - n_patches]; the
    first token, which no row predicts, gets 0."""
    B, S = rows.shape
    out = torch.zeros(B, S - n_patches, dtype=rows.dtype, device=rows.device)
    out[:, 1:] = rows[:, n_patches:S - 1]
    return out


def is_uint8_frames(pixel_values) -> bool:
    """A collated batch of raw RGB frames [B, H, W, 3] uint8 (an `image_transform` that returns the frame itself)."""
    return (torch.is_tensor(pixel_values) and pixel_values.dtype == torch.uint8 and pixel_values.dim() == 4
            and pixel_values.shape[-1] == 3)


def set_loader_batch(engine, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], pixel_values, labels: torch.Tensor,
                     image_aug: bool = False, seed: int = 7, rank: int = 0, step: int = 0) -> None:
    """What both training loops do with a collated batch: uint8 frames take the device path (`set_batch_frames`), with one
    augmentation parameter table per micro-batch drawn from (seed, rank, step) when `image_aug` is set; already-normalised
    float pixel values go through `set_batch` as before, and cannot be augmented any more."""
    if is_uint8_frames(pixel_values):
        params = None
        if image_aug:
            from ..vla.image_augment import draw_params
            params = draw_params(pixel_values.shape[0], seed, rank, step)
        engine.set_batch_frames(input_ids, attention_mask, pixel_values, labels, aug_params=params)
        return
    if image_aug:
        raise ValueError("image_aug needs uint8 frames [B, H, W, 3] under batch['pixel_values'] (the augmentation runs on raw "
                         "frames, on the device): this loader yields already-normalised float pixel values — give the dataset "
                         "an image_transform that returns the uint8 HWC frame")
    engine.set_batch(input_ids, attention_mask, pixel_values, labels)
