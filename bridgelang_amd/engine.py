"""OpenVLA inference engine: static-shape op plans over the HIP kernels, replayed eagerly or as one HIP graph.

The reference's `predict_action` = HF `generate(max_new_tokens=7)` over `PrismaticForConditionalGeneration.forward`
(modeling_prismatic.py:506-536, 291-447): one multimodal prefill (vision towers → projector → splice → 32 Llama layers)
and 6 cached decode steps, with a host round trip per token. Here the whole sequence — prefill, 6 decode steps, the
greedy argmax of every step — is a fixed list of kernel launches on one stream with all intermediate buffers
preallocated (activations for B=16 are < 1 GB of the 288 GB HBM), so it can be captured once and replayed with no host
synchronisation until the 7 token ids are read back. Batched generation is an extension over the reference (batch 1
only, modeling_prismatic.py:326,460-463); per-sample results equal independent batch-1 calls.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Tuple

import torch

from . import ops, train_ops
from .attention_taps import MAX_SEGMENTS, ActionAttention, AttnTaps, pad_bounds, prompt_segments
from .beam import MAX_BEAMS, start_scores
from .llm_plan import decode_fused, decode_layer, head, head_fused, prefill_layer
from .ops import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_F32_BF16R, EPI_NONE, EPI_RES, EPI_SWIGLU, Fp8Weight, Op
from .weights import TowerW, VLAWeights


def rope_tables(head_dim: int, max_pos: int, theta: float, device) -> tuple:
    """HF LlamaRotaryEmbedding on the host, exactly as the reference computes it (fp32 trig, cast to bf16), uploaded
    once: [max_pos, head_dim/2] cos and sin tables."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().to(torch.bfloat16).to(device), fr.sin().to(torch.bfloat16).to(device)


def _fp8_layers(weights: VLAWeights) -> list:
    """e4m3 copies ([{name: ops.Fp8Weight}] per layer) of the Llama projection weights, quantised once per weight set from the packed
    bf16 arena (ops.quantize_weight_fp8) and kept on the weights object: shared by every engine built over these weights.
    (Quantised from the weights as they are NOW: call `weights.__dict__.pop("_fp8_layers", None)` after loading others.)"""
    cache = weights.__dict__.get("_fp8_layers")
    if cache is None:
        cache = [{n: Fp8Weight(*ops.quantize_weight_fp8(ops.unpack_weight(getattr(lw, n))))
                  for n in ("qkv_w", "o_w", "gu_w", "down_w")} for lw in weights.layers]
        weights.__dict__["_fp8_layers"] = cache
    return cache


class EngineResult(NamedTuple):
    """What one run of a generation plan offers, in the order every public call documents (`OpenVLAEngine.result`);
    None: not part of this engine's plan."""
    ids: torch.Tensor                                   # int64 [B, n_new]
    wt: Optional[torch.Tensor] = None                   # int64 [B, n_new, 2]: sample=True / score=True
    range_wt: Optional[torch.Tensor] = None             # int32 [B, n_new, count]: score_range
    values: Optional[torch.Tensor] = None               # fp32 [B] / [B, n_new]: value=
    attention: Optional[ActionAttention] = None         # attn_taps on a generation plan


class BeamTrace(NamedTuple):
    """A beams= engine's run step by step (`OpenVLAEngine.beam_trace`): slot k of prompt e is column e·W + k."""
    tokens: torch.Tensor                                # int64 [n_new, B]: the survivors' tokens
    parents: torch.Tensor                               # int32 [n_new, B]: the slot of the same prompt each descends from
    wt: torch.Tensor                                    # int64 [n_new, B, 2]: the token's weight pair on its parent's row
    scores: torch.Tensor                                # fp32 [n_new, B]: the joint log-probability so far


def present(*parts):
    """The one formatter of every public return: `parts` in their documented order, the None ones dropped; the bare
    element when one is left, else a tuple."""
    out = tuple(p for p in parts if p is not None)
    return out[0] if len(out) == 1 else out


class OpenVLAEngine:
    def __init__(self, weights: VLAWeights, batch: int, prompt_len: int, n_new: int = 7, all_rows: bool = False,
                 use_mask: bool = False, splitk: bool = False, fp8: bool = False, padded: bool = False,
                 vision_only: bool = False, text_only: bool = False, sample: bool = False, score: bool = False,
                 score_range: Optional[Tuple[int, int]] = None, vocab_range: Optional[Tuple[int, int]] = None,
                 attn_taps: Optional[AttnTaps] = None, value: Optional[str] = None, value_head=None,
                 beams: Optional[int] = None, group: Optional[int] = None):
        """all_rows=True builds the training/eval-style forward instead of generation: logits for every position
        (`logits_all` [B*S, vocab] fp32) and no decode steps. use_mask=True threads a [B, S] uint8 key-padding mask
        (`key_mask`, 1 = attend) through the Llama attention (modeling_prismatic.py:387-390). splitk=True lets
        bl_gemm_bf16 split the K range of the last, partially filled round of tiles (≈ +2 % throughput at 7B) — OFF by
        default because those rows then sum in a different fp32 order than the rest, so a sequence's result would depend
        on its batch slot (it breaks "batch-B ≡ B × batch-1 bit for bit", tests/test_full_size_gpu.py). fp8=True runs the
        Llama prefill projections (qkv, o, gate/up, down of every layer but the last) as W8A8 e4m3 GEMMs on the
        block-scaled MFMA (BASELINE configs[4]; per-token × per-channel scales, ops.gemm_fp8) — an extension with no
        reference counterpart: results agree with the bf16 path to quantisation noise, not bit for bit. padded=True builds
        the generation plan for a batch of RIGHT-PADDED prompts (`set_padded_inputs`; HF generation with an attention
        mask, modeling_prismatic.py:387-390): pad positions are hidden from every attention, each sequence's first token
        comes from ITS last real position, and the new tokens are rotated at the sequence's own position — every
        sequence gets exactly the ids and logits it gets alone, un-padded (tests/test_hf_boundary_gpu.py).
        vision_only=True plans the towers alone (the training step's frozen front end): no Llama plans, so nothing here
        holds the decoder-layer weights (parameter-sharded training frees them). text_only=True plans the reference's
        language-only forward (`pixel_values is None`, modeling_prismatic.py:343-359): no towers, no projector, S = L.
        sample=True ends every generation step in bl_sample_f32 instead of bl_argmax_f32 (sampling.py is its
        specification): per-sequence temperature / top-k / top-p / seed live in device buffers filled by `set_sampling`
        (so one captured graph serves any settings; a sequence at temperature 0 is greedy, bit for bit), and `gen_wt`
        [n_new, B, 2] receives each drawn token's integer weight and the kept total (its probability = their quotient).
        Step t of a sequence draws from Philox(key = its seed, counter = t): the draw does not depend on the batch slot.
        score=True is the opposite direction (sampling.score_rows is its specification): the plan is the greedy plan with
        every bl_argmax_f32 replaced by bl_score_f32, which READS `gen_ids[t]` — the forced tokens of `set_forced_ids` —
        and writes their weight pairs to `gen_wt[t]` under the settings of `set_sampling` (no seed); nothing writes
        `gen_ids`, so decode step t consumes the forced token t-1 and every step's logits are the cached decode path's,
        the ones a sample=True engine saw when it drew those tokens. score_range=(first, count) also keeps the kept
        weights of tokens first … first + count - 1 of every step in `gen_range_wt` [n_new, B, count] int32.
        vocab_range=(first, count), with sample=True or score=True, restricts the policy to that token range (the 256
        action bins): the plan ends in bl_sample_range_f32 / bl_score_range_f32, the softmax, top-k, top-p, the draw and a
        greedy sequence's argmax are taken over the range alone, and a score_range must lie inside it. Fixed per engine,
        like score_range.
        attn_taps=AttnTaps(layers, full, segments) adds one read-only bl_attention_probs_f32 after the attention of every
        tapped layer (attention_taps.py): in a generation plan on the query row of the token being produced (step 0: the
        last prompt position), into `tap_probs` / `tap_seg` (`action_attention()`; the segment bounds are the device
        tensor `seg_bounds`, filled by `set_segments`); in an all_rows plan on all S rows, into one [B, H, S, S] buffer
        per tapped layer (`attention_maps()`). The taps read qkv and the KV cache and write nothing the plan reads: every
        id, logit and weight is what the engine without them gives, and with attn_taps=None every plan is op for op the
        one it was.
        value="action" | "token" with value_head=<training.value_head.ValueHead> adds the critic to a generation plan: one
        bl_value_predict_f32 beside the pick of the prefill's head (and, at "token", of every decode step's), over the
        residual rows the lm_head reads — final RMSNorm and head in one launch, since the norm's output is normally never
        written at inference. `values` fp32 [1 | n_new, B]: values[0] is V(s) of the state the action is taken in (the row
        that predicts the first action token, the learner's level="action" value row), values[t] the row that predicts
        action token t + 1 (level="token"). The op reads the head's live weight / bias tensors in place: a learner's
        write-back shows on the next replay of the same captured graph. It writes nothing the plan reads, and with
        value=None every plan is op for op the one it was.
        beams=W turns the plain generation plan into beam search over the new tokens (beam.py is its specification).
        `batch` stays the number of rows: batch % W == 0 and prompt e owns rows e·W … e·W + W - 1; `set_inputs` /
        `set_padded_inputs` take the batch / W prompts and replicate each W times. The W rows of a prompt run the prefill
        as identical rows — W copies are prefilled, as `sample_actions` prefills its copies — and get identical logits:
        that rests on the project's batch-invariance rule (a sequence's bits do not depend on the rows around it), so the
        static start scores [0, -inf, …] make every survivor of step 0 a child of beam 0. Every pick is one
        bl_beam_step_f32 fed by `beam_scores[t - 1]`, writing `gen_ids[t]`, `beam_parent[t]`, `gen_wt[t]` and
        `beam_scores[t]` (all [n_new, B, …], slot-major within a prompt, best first); after the head of decode step t,
        1 <= t <= n_new - 2, ONE bl_beam_reorder_kv_bf16 moves the generated cache rows S … S + t - 1 (padded: from each
        sequence's own `rope_pos[1]` on) of all 2 · layers caches by `beam_parent[t]`. Nothing else carries state from step
        to step: decode step t + 1 starts from the embedding of `gen_ids[t]`. `result()` backtracks: `ids` / `wt` are the W
        finished sequences of every prompt, best first; `beam_trace()` hands out the per-step tokens, parents, pairs and
        scores. Static buffers and launches only, so the plan is capturable like the sampling plan. `vocab_range`
        restricts the continuations to that token range. beams goes with the plain generation plan: not with sample,
        score, all_rows, attn_taps (the taps would have to be reordered too) or value="token" (value="action" is one
        state, so one V(s)). With beams=None every plan is op for op the one it was.
        group=G shares one prefill among the G rows of a prompt: `batch` stays the number of decode rows, batch
        % G == 0, prompt p owns rows p·G … p·G + G - 1, and `set_inputs` takes the P = batch / G prompts. The towers, the
        projector and the prefill are planned on P rows and the prompt caches hold P sequences; the residual rows of step
        0 are replicated G-fold (bl_repeat_rows_bf16) in front of the head, and every decode step is today's decode layer
        on batch rows whose attention (bl_attention_decode_rope_shared_bf16) reads the prompt's cache rows in place and
        keeps the row's own tokens in `k_gen` / `v_gen` [batch, H, n_new - 1, hd]. Seeds, settings, forced ids and beam
        start scores stay per row. Every id, weight and logit is the one the engine without group= gives on
        `repeat_interleave`d inputs, bit for bit: a prefilled row does not depend on the rows around it, and the shared
        kernel restates the decode kernel per row. Goes with sample, score (score_range), greedy, vocab_range, beams == G (the
        reorder then runs over the gen caches from row 0; the prompt caches are never reordered) and value="action" (the
        critic on the P prompt rows: `values` [1, P]). Not with padded, fp8, attn_taps, value="token", all_rows,
        vision_only, text_only, beams != G, or a batch past the fused decode forms (16 rows, head_dim 128). With group=None
        every plan is op for op the one it was."""
        self.w, self.dims = weights, weights.dims
        self.group, self.P = None, batch
        if group is not None:
            if isinstance(group, bool) or int(group) != group or not 1 <= int(group) <= 16:
                raise ValueError(f"group must be an integer in 1 … 16, got {group!r}")
            for on, why in ((padded, "padded prompts put every row at its own position; the shared kernel has one"),
                            (fp8, "the e4m3 prefill is not bit-identical to the path group= is specified against"),
                            (attn_taps is not None, "attn_taps read one cache per row; the prompt rows are shared here"),
                            (value == "token", 'value="token" is not built for shared prefills (value="action" is)'),
                            (all_rows or vision_only or text_only, "a shared prefill belongs to the multimodal generation plan"),
                            (beams is not None and int(beams) != int(group), f"beams={beams}: the beams of a prompt are its group"),
                            (batch % int(group) != 0, f"batch {batch} is the number of rows and must be a multiple of the group"),
                            (not decode_fused(batch, weights.dims), f"the shared decode attention is the fused form only: "
                                                                     f"head_dim 128 and at most 16 rows, got batch {batch}")):
                if on:
                    raise ValueError(f"group={group}: {why}")
            self.group, self.P = int(group), batch // int(group)
        self.beams = None
        if beams is not None:
            if isinstance(beams, bool) or int(beams) != beams or not 1 <= int(beams) <= MAX_BEAMS:
                raise ValueError(f"beams must be an integer in 1 … {MAX_BEAMS}, got {beams!r}")
            for on, why in ((sample, "sample=True draws tokens, beam search ranks them"),
                            (score, "score=True scores given tokens, beam search chooses its own"),
                            (all_rows or vision_only, "beam search belongs to a generation plan"),
                            (attn_taps is not None, "attn_taps would have to be reordered with the beams: not built"),
                            (value == "token", 'value="token" follows one sequence per row; beams change rows every step '
                                               '(value="action" is fine)')):
                if on:
                    raise ValueError(f"beams={beams}: {why}")
            if batch % int(beams):
                raise ValueError(f"beams={beams}: batch {batch} is the number of rows and must be a multiple of the beams")
            self.beams = int(beams)
        self.vision_only, self.text_only = vision_only, text_only
        if text_only and (vision_only or padded or fp8):
            raise ValueError("text_only is the plain bf16 language-model plan")
        self.epoch = 0            # bumped by every prefill that overwrites the KV caches (cache handles check it)
        if not vision_only and not weights.layers_resident:
            raise RuntimeError("the decoder-layer weights are sharded out of the model (parameter-sharded training in progress): "
                               "call the strategy's finish() / TrainStep.materialize_params() before building an inference engine")
        self.padded, self.sample, self.score_mode = padded, sample, score
        if sample and score:
            raise ValueError("sample=True draws tokens, score=True scores given ones: build one engine for each")
        if (sample or score) and (all_rows or vision_only):
            raise ValueError("sample=True / score=True belong to a generation plan")
        if score_range is not None and not score:
            raise ValueError("score_range goes with score=True")
        self.vocab_range = None
        if vocab_range is not None:
            if not (sample or score or self.beams):
                raise ValueError("vocab_range goes with sample=True, score=True or beams=")
            first, count = int(vocab_range[0]), int(vocab_range[1])
            if first < 0 or count < 1 or first + count > self.dims.vocab or first % 4 or count % 4:
                raise ValueError(f"vocab_range {vocab_range}: multiples of 4 inside the vocabulary [0, {self.dims.vocab})")
            self.vocab_range = (first, count)
        if self.beams and self.beams > (self.dims.vocab if self.vocab_range is None else self.vocab_range[1]):
            raise ValueError(f"beams={self.beams} exceeds the number of tokens a step chooses from")
        use_mask = use_mask or padded
        if padded and (all_rows or fp8):
            raise ValueError("padded generation is built for the bf16 generation plan")
        d = self.dims
        if all_rows:
            n_new = 1
        self.all_rows, self.use_mask = all_rows, use_mask
        self.B, self.L, self.n_new = batch, prompt_len, n_new
        self.n_patches = 0 if text_only else d.n_patches
        self.S = prompt_len + self.n_patches
        self.cache_len = (self.S + n_new + 63) // 64 * 64
        if self.cache_len > d.max_pos:
            raise ValueError("sequence exceeds max_position_embeddings")
        dev = weights.embed.device
        self.device = dev
        B, S, D, I = batch, self.S, d.llm_dim, d.llm_inter
        Bp = self.P               # rows of the towers, the projector and the prefill (group=: the prompts; else the batch)
        z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype, device=dev)
        # inputs / outputs (static addresses so a captured graph can be replayed)
        self.pixel_values = z(Bp, 6, 224, 224)
        self.input_ids = z(Bp, prompt_len, dtype=torch.int64)
        self.gen_ids = z(n_new, B, dtype=torch.int64)
        self.logits = z(n_new, B, d.vocab, dtype=torch.float32)
        if sample:      # settings of the sequences now in the buffers (zeros: temperature 0 = greedy) and the weight pairs
            self.samp_temperature, self.samp_top_k = z(B, dtype=torch.float32), z(B, dtype=torch.int32)
            self.samp_top_p, self.samp_seed = torch.ones(B, dtype=torch.float32, device=dev), z(B, dtype=torch.int64)
            self.gen_wt = z(n_new, B, 2, dtype=torch.int64)
        if self.beams:  # per step and row: the survivor's parent slot, weight pair and score; step 0 reads the static start row
            self.beam_scores, self.beam_parent = z(n_new, B, dtype=torch.float32), z(n_new, B, dtype=torch.int32)
            self.gen_wt = z(n_new, B, 2, dtype=torch.int64)
            self.beam_start = torch.from_numpy(start_scores(self.beams)).repeat(B // self.beams).to(dev)
        self.score_range, self.gen_range_wt = None, None
        if score:       # the same settings without a seed; gen_ids holds the forced tokens
            self.samp_temperature, self.samp_top_k = z(B, dtype=torch.float32), z(B, dtype=torch.int32)
            self.samp_top_p = torch.ones(B, dtype=torch.float32, device=dev)
            self.gen_wt = z(n_new, B, 2, dtype=torch.int64)
            if score_range is not None:
                first, count = int(score_range[0]), int(score_range[1])
                if first < 0 or count < 1 or first + count > d.vocab:
                    raise ValueError(f"score_range {score_range} leaves the vocabulary [0, {d.vocab})")
                if self.vocab_range is not None and (first < self.vocab_range[0] or first + count > sum(self.vocab_range)):
                    raise ValueError(f"score_range {score_range} leaves vocab_range {self.vocab_range}")
                self.score_range = (first, count)
                self.gen_range_wt = z(n_new, B, count, dtype=torch.int32)
        # vision buffers (sized for the larger tower, shared by both: they run back to back on one stream)
        tmax = max(d.dino.tokens, d.siglip.tokens)
        dmax = max(d.dino.dim, d.siglip.dim)
        hmax = max(d.dino.mlp_pad, d.siglip.mlp_pad)
        # one private set per tower: the two towers run concurrently on two streams
        self.vbuf = [dict(col=z(Bp * 256, (d.patch_k + 63) // 64 * 64), x=z(Bp * tmax * dmax), h=z(Bp * tmax * dmax),
                          ao=z(Bp * tmax * dmax), qkv=z(Bp * tmax * 3 * dmax), mlp=z(Bp * tmax * hmax),
                          ws=None) for _ in range(2)]   # ViT GEMMs never reach the split-K regime (K <= 4352)
        self.feats = z(Bp * 256, d.vision_dim)
        self.p1, self.p2 = z(Bp * 256, 4 * d.vision_dim), z(Bp * 256, D)
        # llm buffers
        if not vision_only:
            self.x = z(Bp, S, D)
            self.h, self.ao = z(Bp * S, D), z(Bp * S, D)
            self.qkv = z(Bp * S, 3 * D)
            self.act = z(Bp * S, I)
            self.k_cache = [z(Bp, d.llm_heads, self.cache_len, d.head_dim) for _ in range(d.llm_layers)]
            self.v_cache = [z(Bp, d.llm_heads, self.cache_len, d.head_dim) for _ in range(d.llm_layers)]
            self.xd, self.hd, self.aod = z(B, D), z(B, D), z(B, D)
            self.qkvd, self.actd = z(B, 3 * D), z(B, I)
            if self.group:      # the rows' own tokens, and the P-row buffers of the prefill's last-row layer
                gen_len = max(1, n_new - 1)
                self.k_gen = [z(B, d.llm_heads, gen_len, d.head_dim) for _ in range(d.llm_layers)]
                self.v_gen = [z(B, d.llm_heads, gen_len, d.head_dim) for _ in range(d.llm_layers)]
                self.xp, self.aop, self.actp = z(Bp, D), z(Bp, D), z(Bp, I)
            if self.beams and self.beams > 1:       # the base pointers of all 2 · layers caches: one reorder launch per step
                self.kv_table = ops.cache_table(self.k_gen + self.v_gen if self.group else self.k_cache + self.v_cache)
        self.cos, self.sin = rope_tables(d.head_dim, d.max_pos, d.rope_theta, dev)
        self.ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev) if splitk else None   # split-K scratch (opt-in)
        if padded:        # one mask over the whole cache: real prompt rows and every generated row are visible
            if d.head_dim != 128 or not ops.skinny_supported(B, D, EPI_NONE):
                raise NotImplementedError("padded generation needs head_dim 128 and a batch of at most 16")
            self.cache_mask = torch.ones(B, self.cache_len, dtype=torch.uint8, device=dev)
            self.key_mask = self.cache_mask[:, :S]
            self.last_row = torch.full((B,), S - 1, dtype=torch.int64, device=dev)      # index of the last real position
            self.rope_pos = torch.zeros(n_new, B, dtype=torch.int32, device=dev)        # rotation position of new token t
            self.q_last, self.x_last = z(B, D), z(B, D)
        else:
            self.key_mask = torch.ones(Bp, S, dtype=torch.uint8, device=dev) if use_mask else None
        self.logits_all = z(B * S, d.vocab, dtype=torch.float32) if all_rows else None
        self.fp8 = fp8
        if fp8:
            if d.llm_dim % 128 or d.llm_inter % 128:
                raise ValueError("fp8 prefill needs llm_dim and llm_inter to be multiples of 128")
            self.w8 = _fp8_layers(weights)
            self.h8, self.act8 = z(B * S, D, dtype=torch.uint8), z(B * S, I, dtype=torch.uint8)
            self.sq = z(B * S, dtype=torch.float32)
        self.value, self.value_head, self.values = value, value_head, None
        if value is not None:
            if value not in ("action", "token"):
                raise ValueError(f"value is None, 'action' or 'token', got {value!r}")
            if all_rows or vision_only:
                raise ValueError("value= belongs to a generation plan")
            if value_head is None or value_head.dim != D:
                raise ValueError(f"value={value!r} needs a value_head of dim {D}, got "
                                 f"{None if value_head is None else value_head.dim}")
            if value_head.weight.device != dev:
                raise ValueError(f"value_head lives on {value_head.weight.device}, the weights on {dev}")
            self.values = z(n_new if value == "token" else 1, Bp, dtype=torch.float32)
        elif value_head is not None:
            raise ValueError("value_head goes with value='action' or 'token'")
        self.attn_taps, self.tap_slot = attn_taps, {}
        if attn_taps is not None:
            if vision_only:
                raise ValueError("attn_taps tap the Llama attention: a vision_only engine has none")
            if d.head_dim != 128 or self.cache_len > 2048:
                raise NotImplementedError("attn_taps need head_dim 128 and a cache of at most 2048 rows")
            self.tap_layers = attn_taps.resolve(d.llm_layers)
            self.tap_slot = {l: i for i, l in enumerate(self.tap_layers)}
            nt, Hh = len(self.tap_layers), d.llm_heads
            self.tap_probs = self.tap_seg = self.tap_maps = self.tap_mask = None
            if all_rows:
                self.tap_maps = [z(B, Hh, S, S, dtype=torch.float32) for _ in range(nt)]
            else:
                # step-major so that one (step, layer) slab is the kernel's contiguous [B, H, 1, n]; action_attention() permutes
                if attn_taps.full:
                    self.tap_probs = z(n_new, nt, B, Hh, self.cache_len, dtype=torch.float32)
                if attn_taps.segments:
                    self.tap_seg = z(n_new, nt, B, Hh, MAX_SEGMENTS, dtype=torch.float32)
                    self.seg_bounds = z(B, MAX_SEGMENTS + 1, dtype=torch.int32)
                if padded:      # keys of decode step t: rows 0 .. rope_pos[t][b] of sequence b's cache
                    self.tap_mask = z(n_new, B, self.cache_len, dtype=torch.uint8)
                    self.q_tap = z(B, D)
                self.set_segments(*prompt_segments(torch.ones(B, prompt_len, dtype=torch.int64), self.n_patches, n_new))

        self.dino_ops = [] if text_only else self._plan_tower(weights.dino, 0, self.vbuf[0])
        self.siglip_ops = [] if text_only else self._plan_tower(weights.siglip, d.dino.dim, self.vbuf[1])
        self.vision_ops = self.dino_ops + self.siglip_ops      # serial order (profiling / single-stream use)
        self._side = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        if vision_only:
            self.projector_ops, self.prefill_ops, self.decode_ops = [], [], []
        else:
            self.projector_ops = [] if text_only else self._plan_projector()
            self.prefill_ops = self._plan_prefill()
            self.decode_ops = [self._plan_decode(t) for t in range(1, n_new)]
        self._graph: Optional[torch.cuda.CUDAGraph] = None

    def _g(self, *args, **kw):
        return ops.gemm(*args, workspace=self.ws, **kw)

    # ---- plans ----------------------------------------------------------------------------------------------------
    def _plan_tower(self, tw: TowerW, feat_col: int, vb: dict) -> List[Op]:
        """timm VisionTransformer up to the tap: K1-K9 of SURVEY §2.4."""
        t, B = tw.dims, self.P
        T, Dm, Hp, hd = t.tokens, t.dim, t.mlp_pad, t.head_dim
        M = B * T
        x = vb["x"][:M * Dm].view(M, Dm)
        h = vb["h"][:M * Dm].view(M, Dm)
        ao = vb["ao"][:M * Dm].view(M, Dm)
        qkv = vb["qkv"][:M * 3 * Dm].view(M, 3 * Dm)
        mlp = vb["mlp"][:M * Hp].view(M, Hp)
        v_col = vb["col"]
        g = lambda *a, **k: ops.gemm(*a, workspace=vb["ws"], **k)     # private split-K scratch per stream
        plan = [ops.im2col_patch14(self.pixel_values, t.chan0, v_col, run=False)]
        if tw.prefix is not None:
            plan.append(ops.write_prefix_tokens(tw.prefix, x, B, T, run=False))
        # patch-embed GEMM + bias + pos-embed, rows written behind the prefix tokens
        plan.append(g(v_col, tw.patch_w, x, EPI_BIAS_RES, bias=tw.patch_b, res=tw.pos, res_row_mod=256,
                             out_map=(256, T, t.n_prefix), algo_nk=(Dm, self.dims.patch_k), run=False))
        st = (T * 3 * Dm, hd, 3 * Dm)
        for i, b in enumerate(tw.blocks):
            plan.append(ops.layernorm(x, b.norm1_w, b.norm1_b, h, self.dims.ln_eps, run=False))
            plan.append(g(h, b.qkv_w, qkv, EPI_BIAS, bias=b.qkv_b, run=False))
            plan.append(ops.attention(qkv, qkv[:, Dm:], qkv[:, 2 * Dm:], ao, B=B, H=t.heads, Sq=T, Skv=T, head_dim=hd,
                                      q_strides=st, k_strides=st, v_strides=st, o_strides=(T * Dm, hd, Dm),
                                      causal=False, run=False))
            plan.append(g(ao, b.proj_w, x, EPI_BIAS_RES, bias=b.proj_b, scale=b.ls1, res=x, run=False))
            plan.append(ops.layernorm(x, b.norm2_w, b.norm2_b, h, self.dims.ln_eps, run=False))
            plan.append(g(h, b.fc1_w, mlp, EPI_BIAS_GELU, bias=b.fc1_b, algo_nk=(t.mlp, Dm), run=False))
            if i + 1 < len(tw.blocks):
                plan.append(g(mlp, b.fc2_w, x, EPI_BIAS_RES, bias=b.fc2_b, scale=b.ls2, res=x, algo_nk=(Dm, t.mlp),
                                     run=False))
            else:   # tap: drop the prefix tokens and write this tower's channels of the fused feature map
                plan.append(g(mlp, b.fc2_w, self.feats[:, feat_col:feat_col + Dm], EPI_BIAS_RES, bias=b.fc2_b,
                                     scale=b.ls2, res=x, out_map=(T, 256, -t.n_prefix), algo_nk=(Dm, t.mlp), run=False))
        return plan

    def _plan_projector(self) -> List[Op]:
        """PrismaticProjector (modeling_prismatic.py:151-156); fc3 writes straight into LLM embedding rows 1..256."""
        w, B, S, D = self.w, self.P, self.S, self.dims.llm_dim
        return [self._g(self.feats, w.fc1_w, self.p1, EPI_BIAS_GELU, bias=w.fc1_b, run=False),
                self._g(self.p1, w.fc2_w, self.p2, EPI_BIAS_GELU, bias=w.fc2_b, run=False),
                self._g(self.p2, w.fc3_w, self.x.view(B * S, D), EPI_BIAS, bias=w.fc3_b, out_map=(256, S, 1), run=False)]

    def _tap(self, l: int, t: int, q: torch.Tensor, q_strides, Skv: int, rope: Optional[tuple], key_mask, b0: int = 0,
             b1: Optional[int] = None) -> List[Op]:
        """The attention tap of layer l for generation step t (nothing if the layer is not tapped): the probabilities of
        the step's one query row per sequence over cache rows [0, Skv). rope = None: q is rotated in memory; else
        (pos0, rope_pos): rotated on load. Writes every column of its tap_probs rows (zeros past Skv) and its tap_seg rows."""
        if l not in self.tap_slot:
            return []
        if (b0, self.B if b1 is None else b1) != (0, self.B):
            raise ValueError("attention taps are built for the whole batch (no batch ranges: the staggered pipeline has no taps)")
        d, i = self.dims, self.tap_slot[l]
        H, hd = d.llm_heads, d.head_dim
        kw = {} if rope is None else dict(cos=self.cos, sin=self.sin, pos0=rope[0], rope_pos=rope[1])
        return [ops.attention_probs(q, self.k_cache[l], B=self.B, H=H, Sq=1, Skv=Skv, head_dim=hd, q_strides=q_strides,
                                    k_strides=(H * self.cache_len * hd, self.cache_len * hd, hd), causal=False, key_mask=key_mask,
                                    probs=None if self.tap_probs is None else self.tap_probs[t, i].unsqueeze(2),
                                    seg=None if self.tap_seg is None else self.tap_seg[t, i].unsqueeze(2),
                                    seg_bounds=None if self.tap_seg is None else self.seg_bounds, run=False, **kw)]

    def _plan_prefill(self, b0: int = 0, b1: Optional[int] = None) -> List[Op]:
        """Llama prefill + first token for batch rows [b0, b1) (default: the whole batch). Every buffer is batch-major, so
        a batch range is a contiguous slice of each; results do not depend on the range a sequence is run in."""
        d, w, S = self.dims, self.w, self.S
        b1 = self.P if b1 is None else b1
        B, D, H, hd = b1 - b0, d.llm_dim, d.llm_heads, d.head_dim
        rows, x3 = slice(b0 * S, b1 * S), self.x[b0:b1]
        x, h, qkv, ao, act = x3.view(B * S, D), self.h[rows], self.qkv[rows], self.ao[rows], self.act[rows]
        key_mask = self.key_mask[b0:b1] if self.key_mask is not None else None
        cs = (H * self.cache_len * hd, self.cache_len * hd, hd)
        rope_in_attention = hd == 128 and S <= 320
        fp8 = self.fp8 and rope_in_attention       # the e4m3 linears are built for the layers of the fused attention

        def lin(l, x, name, out, epi, **kw):
            if not fp8:
                return [self._g(x, getattr(w.layers[l], name), out, epi, run=False, **kw)]
            q8 = (self.act8 if name == "down_w" else self.h8)[rows]
            return ops.linear_fp8(x, q8, self.sq[rows], *self.w8[l][name], out, epi, **kw)

        def tap(l):
            """After layer l's attention: qkv still holds its q (un-rotated under the fused attention, rotated in place
            otherwise) and k_cache[l] its rotated keys."""
            if l not in self.tap_slot:
                return []
            if self.all_rows:       # every row, HF's `attentions` entry of the layer
                kw = dict(cos=self.cos, sin=self.sin, pos0=0) if rope_in_attention else {}
                return [ops.attention_probs(qkv, self.k_cache[l][b0:b1], B=B, H=H, Sq=S, Skv=S, head_dim=hd,
                                            q_strides=(S * 3 * D, hd, 3 * D), k_strides=cs, causal=True, key_mask=key_mask,
                                            probs=self.tap_maps[self.tap_slot[l]][b0:b1], run=False, **kw)]
            if self.padded:         # the row that produces the first token is each sequence's last REAL one: gather it
                rope = (0, self.rope_pos[0]) if rope_in_attention else None
                return ([ops.gather_rows(qkv.view(B, S, 3 * D)[:, :, :D], self.last_row[b0:b1], self.q_tap[b0:b1], run=False)]
                        + self._tap(l, 0, self.q_tap, (D, hd, D), S, rope, key_mask, b0, b1))
            rope = (S - 1, None) if rope_in_attention else None
            return self._tap(l, 0, qkv.view(B, S, 3 * D)[:, S - 1], (S * 3 * D, hd, 3 * D), S, rope, key_mask, b0, b1)

        def attn(l):
            kc, vc = self.k_cache[l][b0:b1], self.v_cache[l][b0:b1]
            if rope_in_attention:   # RoPE and the KV-cache write ride inside the attention kernel's q / k / v loads
                return [ops.attention_rope(qkv, kc, vc, ao, self.cos, self.sin, B=B, S=S, H=H, head_dim=hd, pos0=0,
                                           key_mask=key_mask, run=False)] + tap(l)
            return [ops.rope_kvcache(qkv, self.cos, self.sin, kc, vc, B=B, S=S, H=H, head_dim=hd, pos0=0, run=False),
                    ops.attention(qkv, kc, vc, ao, B=B, H=H, Sq=S, Skv=S, head_dim=hd, q_strides=(S * 3 * D, hd, 3 * D),
                                  k_strides=cs, v_strides=cs, o_strides=(S * D, hd, D), causal=True, key_mask=key_mask,
                                  run=False)] + tap(l)

        plan = [ops.embed_splice(self.input_ids[b0:b1], w.embed, x3, self.n_patches, run=False)]
        self.layer_ends: List[int] = []       # len(plan) after each decoder layer (hidden-state taps of the all_rows plan)
        # Generation consumes only the last position of the last layer (the reference materialises all S rows of every
        # layer): _plan_last_rows.
        last_rows_only = not self.all_rows and d.llm_layers > 1
        for l in range(d.llm_layers - int(last_rows_only)):
            plan += prefill_layer(w.layers[l], x, h, qkv, ao, act, d.rms_eps, functools.partial(lin, l), attn(l))
            self.layer_ends.append(len(plan))
        if last_rows_only:
            return plan + self._plan_last_rows(b0, b1)
        if self.all_rows:   # HF semantics: logits for every position (what forward()/training consume)
            return plan + [ops.rmsnorm(x, w.norm, h, d.rms_eps, run=False),
                           self._g(h, w.lm_head, self.logits_all[rows], EPI_F32_BF16R, run=False)]
        # final norm + lm_head on the last position only (the reference materialises all S rows)
        return plan + self._first_token(x3[:, S - 1, :], b0, b1)

    def _first_token(self, x_rows: torch.Tensor, b0: int, b1: int) -> List[Op]:
        """The head of step 0 over the prefill's last residual rows. group=: the P rows are replicated G-fold into `xd`
        first (a copy), so the head, and every per-row pick behind it, runs on all rows; the critic reads the P rows."""
        if not self.group:
            return self._head(x_rows, 0, b0, b1)
        return [ops.repeat_rows(x_rows, self.xd, self.group, run=False)] + self._head(self.xd, 0, value_rows=x_rows)

    def _plan_last_rows(self, b0: int, b1: int) -> List[Op]:
        """The last decoder layer of a generation prefill + the first token: it still projects K/V for every position (the
        decode steps attend to them), but its attention, o_proj and MLP run on the B last rows only — single-query
        attention + weight-streaming GEMMs."""
        d, S, B, lw = self.dims, self.S, b1 - b0, self.w.layers[-1]
        D, H, hd = d.llm_dim, d.llm_heads, d.head_dim
        x3, xd, aod, actd = self.x[b0:b1], self.xd[b0:b1], self.aod[b0:b1], self.actd[b0:b1]
        if self.group:      # P rows of their own: xd takes their G-fold copies in front of the head
            xd, aod, actd = self.xp, self.aop, self.actp
        h, qkv = self.h[b0 * S:b1 * S], self.qkv[b0 * S:b1 * S]
        kc, vc = self.k_cache[-1][b0:b1], self.v_cache[-1][b0:b1]
        cs = (H * self.cache_len * hd, self.cache_len * hd, hd)
        plan = [ops.rmsnorm(x3.view(B * S, D), lw.ln1, h, d.rms_eps, run=False), self._g(h, lw.qkv_w, qkv, EPI_NONE, run=False),
                ops.rope_kvcache(qkv, self.cos, self.sin, kc, vc, B=B, S=S, H=H, head_dim=hd, pos0=0, run=False)]
        if self.padded:
            # each sequence's last REAL position: gather its (rotated) q row and residual row (bl_gather_rows_bf16: a
            # copy, no arithmetic), then the same single-query attention / weight-streaming GEMMs as the un-padded plan
            q_last, x_last, last_row = self.q_last[b0:b1], self.x_last[b0:b1], self.last_row[b0:b1]
            q_strides, mask = (D, hd, D), self.cache_mask[b0:b1]
            plan += [ops.gather_rows(qkv.view(B, S, 3 * D)[:, :, :D], last_row, q_last, run=False),   # the q third
                     ops.gather_rows(x3, last_row, x_last, run=False)]
        else:
            q_last, x_last = qkv.view(B, S, 3 * D)[:, S - 1], x3[:, S - 1, :]      # roped in place; row stride S·3D
            q_strides, mask = (S * 3 * D, hd, 3 * D), None
        plan.append(ops.attention_decode(q_last, kc, vc, aod, B=B, H=H, Skv=S, head_dim=hd, q_strides=q_strides,
                                         k_strides=cs, v_strides=cs, o_strides=(D, hd, D), key_mask=mask, run=False))
        plan += self._tap(d.llm_layers - 1, 0, q_last, q_strides, S, None, mask, b0, b1)      # q_last is rotated
        plan.append(self._g(aod, lw.o_w, xd, EPI_RES, res=x_last, run=False))
        plan += self._norm_lin(xd, lw.ln2, lw.gu_w, actd, EPI_SWIGLU, ops.skinny_supported(B, D, EPI_SWIGLU), b0, b1)
        return plan + [self._g(actd, lw.down_w, xd, EPI_RES, res=xd, run=False)] + self._first_token(xd, b0, b1)

    def _norm_lin(self, x, norm_w, W, out, epi, fused: bool, b0: int = 0, b1: Optional[int] = None) -> List[Op]:
        """A linear on B rows with an RMSNorm in front: fused into the weight-streaming GEMM (`a_norm`), or a launch of
        its own into `hd` ahead of the GEMM."""
        if fused:
            return [self._g(x, W, out, epi, a_norm=(norm_w, self.dims.rms_eps), run=False)]
        return [ops.rmsnorm(x, norm_w, self.hd[b0:b1], self.dims.rms_eps, run=False), self._g(self.hd[b0:b1], W, out, epi, run=False)]

    def _head(self, x_rows: torch.Tensor, t: int, b0: int = 0, b1: Optional[int] = None,
              value_rows: Optional[torch.Tensor] = None) -> List[Op]:
        """final RMSNorm → lm_head (bf16-rounded fp32 logits) → the token of generation step t. `value_rows`: the rows the
        critic reads where they are not `x_rows` (group=: the P prompt rows)."""
        logits = self.logits[t][b0:b1]
        norm_lin = functools.partial(self._norm_lin, fused=head_fused(logits.shape[0], self.dims), b0=b0, b1=b1)
        return head(self.w, x_rows, logits, norm_lin,
                    [self._pick(logits, t, b0, b1)] + self._value(x_rows if value_rows is None else value_rows, t, b0, b1))

    def _value(self, x_rows: torch.Tensor, t: int, b0: int = 0, b1: Optional[int] = None) -> List[Op]:
        """The critic over the residual rows generation step t's lm_head reads, into values[t] (nothing without a head, and
        nothing past step 0 at level "action"). The pipeline calls it with its own rows for this engine's batch."""
        if self.value is None or (t > 0 and self.value != "token"):
            return []
        vh = self.value_head
        return [train_ops.value_predict(x_rows, self.w.norm, self.dims.rms_eps, vh.weight, vh.bias, self.values[t][b0:b1], run=False)]

    def _pick(self, logits: torch.Tensor, t: int, b0: int = 0, b1: Optional[int] = None) -> Op:
        """Generation step t's token from its logits: greedy argmax (sample=True: the seeded draw; score=True: the score
        of the forced token). The pipeline calls it with its own logits rows for this engine's batch."""
        ids = self.gen_ids[t][b0:b1]
        if self.beams:
            if (b0, self.B if b1 is None else b1) != (0, self.B):
                raise ValueError("beam search is built for the whole batch (no batch ranges: the staggered pipeline has no beams)")
            return ops.beam_step(logits, self.beams, self.beam_start if t == 0 else self.beam_scores[t - 1], ids,
                                 self.beam_parent[t], self.gen_wt[t], self.beam_scores[t], run=False, vocab=self.vocab_range)
        if self.sample:
            return ops.sample(logits, self.samp_temperature[b0:b1], self.samp_top_k[b0:b1], self.samp_top_p[b0:b1],
                              self.samp_seed[b0:b1], t, ids, self.gen_wt[t][b0:b1], run=False, vocab=self.vocab_range)
        if self.score_mode:
            rng = (0, None) if self.score_range is None else (self.score_range[0], self.gen_range_wt[t][b0:b1])
            return ops.score(logits, self.samp_temperature[b0:b1], self.samp_top_k[b0:b1], self.samp_top_p[b0:b1], ids,
                             self.gen_wt[t][b0:b1], *rng, run=False, vocab=self.vocab_range)
        return ops.argmax(logits, ids, run=False)

    def _decode_attn(self, l: int, t: int, qkv, ao, fused: bool, rope: Optional[tuple] = None) -> List[Op]:
        """Attention of decode step t in layer l: this batch's token at position S+t-1 against its own KV cache, from
        qkv [B, 3D] into ao [B, D] (the pipeline passes its rows for this batch, and one pair of rope tables for all)."""
        d, B, pos = self.dims, self.B, self.S + t - 1
        D, H, hd = d.llm_dim, d.llm_heads, d.head_dim
        (cos, sin), kc, vc = rope or (self.cos, self.sin), self.k_cache[l], self.v_cache[l]
        if self.group:      # the prompt's rows in place, the row's own tokens in its gen cache (fused form only: checked at build)
            return [ops.attention_decode_rope_shared(qkv, kc, vc, self.k_gen[l], self.v_gen[l], ao, cos, sin, group=self.group, H=H,
                                                     head_dim=hd, prefix_len=self.S, pos=pos, run=False)]
        if fused:
            # padded: every sequence appends at its own position (over its pad rows): the cache layout, and with
            # it every sum, is the one of the sequence's un-padded run
            pad_kw = dict(rope_pos=self.rope_pos[t]) if self.padded else {}
            tap = []
            if l in self.tap_slot:      # qkv keeps the un-rotated q; padded: sequence b's keys are rows 0 .. rope_pos[t][b]
                tap = self._tap(l, t, qkv, (3 * D, hd, 3 * D), pos + 1, (pos, pad_kw.get("rope_pos")),
                                self.tap_mask[t] if self.padded else None)
            return [ops.attention_decode_rope(qkv, kc, vc, ao, cos, sin, B=B, H=H, head_dim=hd, pos=pos, run=False, **pad_kw)] + tap
        cs = (H * self.cache_len * hd, self.cache_len * hd, hd)
        return [ops.rope_kvcache(qkv, cos, sin, kc, vc, B=B, S=1, H=H, head_dim=hd, pos0=pos, run=False),
                ops.attention_decode(qkv, kc, vc, ao, B=B, H=H, Skv=pos + 1, head_dim=hd, q_strides=(3 * D, hd, 3 * D),
                                     k_strides=cs, v_strides=cs, o_strides=(D, hd, D), run=False)] \
            + self._tap(l, t, qkv, (3 * D, hd, 3 * D), pos + 1, None, None)      # q was rotated in place

    def _plan_decode(self, t: int) -> List[Op]:
        """Cached-generation step t (modeling_prismatic.py:325-341): token gen_ids[t-1] at position S+t-1. Five
        launches per layer when B rows fit the skinny kernel: qkv (RMSNorm fused) → attention (RoPE + KV append fused) →
        o_proj+residual → gate/up (RMSNorm + SwiGLU fused) → down+residual."""
        B, D, w = self.B, self.dims.llm_dim, self.w
        fused = decode_fused(B, self.dims)
        norm_lin = functools.partial(self._norm_lin, fused=fused)
        lin = lambda x, W, out, epi, res: [self._g(x, W, out, epi, res=res, run=False)]
        attn = lambda l: self._decode_attn(l, t, self.qkvd, self.aod, fused)
        plan = [ops.embed_splice(self.gen_ids[t - 1].view(B, 1), w.embed, self.xd.view(B, 1, D), 0, run=False)]
        for l, lw in enumerate(w.layers):
            plan += decode_layer(l, lw, self.xd, self.qkvd, self.aod, self.actd, norm_lin, lin, attn)
        return plan + self._head(self.xd, t) + self._beam_reorder(t)

    def _beam_reorder(self, t: int) -> List[Op]:
        """Behind the head of decode step t: slot k of every prompt takes the t generated cache rows of slot
        beam_parent[t][k], in all caches at once. Nothing without beams, for one beam (the identity) and behind the last
        step (no step reads the caches any more)."""
        if not self.beams or self.beams == 1 or not 1 <= t <= self.n_new - 2:
            return []
        if self.group:      # the generated rows live in the gen caches, from row 0; the prompt caches are never reordered
            return [ops.beam_reorder_kv(self.kv_table, self.k_gen + self.v_gen, self.beams, self.beam_parent[t], 0, t, run=False)]
        return [ops.beam_reorder_kv(self.kv_table, self.k_cache + self.v_cache, self.beams, self.beam_parent[t],
                                    self.rope_pos[1] if self.padded else self.S, t, run=False)]

    def _per_beam(self, t: Optional[torch.Tensor], what: str) -> Optional[torch.Tensor]:
        """A beam engine's inputs are given per prompt: [B / W, …] → every prompt's W rows (group=: the prompts stay as they
        are, one prefill row each)."""
        if not self.beams or t is None or self.group:
            return t
        if t.shape[0] != self.B // self.beams:
            raise ValueError(f"engine built for {self.B // self.beams} prompts of {self.beams} beams, got {what} {tuple(t.shape)}")
        return t.repeat_interleave(self.beams, dim=0)

    # ---- execution ------------------------------------------------------------------------------------------------
    def all_ops(self) -> List[Op]:
        out = self.vision_ops + self.projector_ops + self.prefill_ops
        for step in self.decode_ops:
            out = out + step
        return out

    def run_vision(self) -> None:
        """The two towers are independent until the projector: DINOv2 on the current stream, SigLIP on a side stream
        (fork/join with stream waits, which HIP-graph capture records as parallel branches). Their GEMMs often fill only
        part of the chip (e.g. 264 tiles on 512 slots), so running them side by side recovers the idle CUs."""
        if self._side is None:
            ops.run_all(self.vision_ops)
            return
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            ops.run_all(self.siglip_ops)
        ops.run_all(self.dino_ops)
        main.wait_stream(self._side)

    def _run_all_stages(self) -> None:
        self.run_vision()
        ops.run_all(self.projector_ops + self.prefill_ops)
        for step in self.decode_ops:
            ops.run_all(step)

    def run_eager(self) -> None:
        self._run_all_stages()

    def capture(self) -> None:
        """Capture the whole action-sequence computation into one HIP graph (after one eager warm-up launch)."""
        self.run_eager()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._run_all_stages()
        self._graph = g

    def replay(self) -> None:
        if self._graph is None:
            self.run_eager()
        else:
            self._graph.replay()

    def set_inputs(self, input_ids: torch.Tensor, pixel_values: torch.Tensor) -> None:
        """The batch's prompts and images (beams=W: the B / W prompts, each replicated to its W rows; group=G: the B / G
        prompts as they are)."""
        self._fill_inputs(self._per_beam(input_ids, "input_ids"), self._per_beam(pixel_values, "pixel_values"))

    def _fill_inputs(self, input_ids: torch.Tensor, pixel_values: torch.Tensor) -> None:
        if tuple(input_ids.shape) != (self.P, self.L):
            raise ValueError(f"engine built for input_ids {(self.P, self.L)}, got {tuple(input_ids.shape)}")
        if self.text_only:
            if pixel_values is not None:
                raise ValueError("a text_only engine takes no pixel_values")
            self.input_ids.copy_(input_ids)
            self.epoch += 1
            return
        if tuple(pixel_values.shape) != (self.P, 6, 224, 224):
            raise ValueError(f"pixel_values must be [{self.P}, 6, 224, 224]")
        self.input_ids.copy_(input_ids)
        self.pixel_values.copy_(pixel_values.to(torch.bfloat16))
        self.epoch += 1

    def set_padded_inputs(self, input_ids: torch.Tensor, pixel_values: torch.Tensor, attention_mask: torch.Tensor,
                          check: bool = True) -> None:
        """Right-padded prompts [B, L] with attention_mask [B, L] (1 = real token; the collator's layout,
        util/data_utils.py:101-142). Fills the cache mask, the per-sequence last position and rotation positions.
        check=False skips the test of the mask's layout (a host synchronisation) for a caller that has made it 1…1 0…0
        with at least one token itself; positions come from the mask's row sums (at most L), so they stay inside the cache either way."""
        if not self.padded:
            raise ValueError("engine was not built with padded=True")
        input_ids, pixel_values = self._per_beam(input_ids, "input_ids"), self._per_beam(pixel_values, "pixel_values")
        m = self._per_beam(attention_mask, "attention_mask").to(self.device).bool()
        if tuple(m.shape) != (self.B, self.L):
            raise ValueError(f"attention_mask must be {(self.B, self.L)}")
        n_real = m.sum(dim=1)
        if check and (bool((n_real < 1).any()) or not bool((m == (torch.arange(self.L, device=self.device)[None, :] < n_real[:, None])).all())):
            raise ValueError("generate(): prompts must be right-padded (attention_mask = 1…1 0…0) with at least one token")
        self._fill_inputs(input_ids, pixel_values)
        P = self.dims.n_patches
        self.cache_mask.fill_(1)
        self.cache_mask[:, 1 + P:self.S] = m[:, 1:].to(torch.uint8)          # column 0 (BOS) and the 256 patch columns stay on
        self.last_row.copy_(P + n_real - 1)
        self.rope_pos.copy_((P + n_real)[None, :].to(torch.int32) + torch.arange(self.n_new, device=self.device, dtype=torch.int32)[:, None] - 1)
        if self.attn_taps is not None:
            if self.tap_mask is not None:
                self.tap_mask.copy_(torch.arange(self.cache_len, device=self.device)[None, None, :] <= self.rope_pos[:, :, None])
            self.set_segments(*prompt_segments(m.cpu(), P, self.n_new))      # the default segments of these prompts

    def set_segments(self, names, bounds: torch.Tensor) -> None:
        """The key segments the taps sum over: `names` and int32 bounds [B, len(names) + 1] in cache rows
        (attention_taps.prompt_segments). They live in the device tensor `seg_bounds`, which the taps read when they run,
        so a captured graph serves any segments; they stay until the next call (set_padded_inputs resets them to the
        defaults of its prompts)."""
        if self.attn_taps is None or self.all_rows:
            raise ValueError("engine was not built with attn_taps on a generation plan")
        names, bounds = tuple(names), torch.as_tensor(bounds).to(torch.int32)
        if tuple(bounds.shape) != (self.B, len(names) + 1):
            raise ValueError(f"set_segments: bounds must be [{self.B}, {len(names) + 1}] for {len(names)} names, got {tuple(bounds.shape)}")
        if bool((bounds[:, 1:] < bounds[:, :-1]).any()) or bool((bounds < 0).any()):
            raise ValueError("set_segments: bounds must be non-negative and non-decreasing")
        self.seg_names = names
        if self.tap_seg is not None:
            self.seg_bounds.copy_(pad_bounds(bounds.cpu(), MAX_SEGMENTS))

    def action_attention(self, own=lambda x: x) -> ActionAttention:
        """What the taps of the last run recorded, as views of the static buffers (device tensors; no host sync) — or, with
        `own=torch.clone`, as copies."""
        if self.attn_taps is None or self.all_rows:
            raise ValueError("engine was not built with attn_taps on a generation plan")
        probs = None if self.tap_probs is None else own(self.tap_probs.permute(2, 0, 1, 3, 4))
        seg = None if self.tap_seg is None else own(self.tap_seg.permute(2, 0, 1, 3, 4)[..., :len(self.seg_names)])
        return ActionAttention(probs=probs, segments=seg, names=self.seg_names, layers=self.tap_layers)

    def attention_maps(self) -> tuple:
        """all_rows plan: HF's `attentions` — one entry per decoder layer, fp32 [B, H, S, S], None for a layer not tapped."""
        if self.attn_taps is None or not self.all_rows:
            raise ValueError("engine was not built with attn_taps on an all_rows plan")
        return tuple(self.tap_maps[self.tap_slot[l]] if l in self.tap_slot else None for l in range(self.dims.llm_layers))

    def value_result(self) -> torch.Tensor:
        """The critic's values of the last run, as a view of the static buffer (device tensor; no host sync): fp32 [B] at
        value="action", [B, n_new] at "token"."""
        if self.values is None:
            raise ValueError("engine was not built with value=")
        return self.values[0] if self.value == "action" else self.values.t()

    def set_sampling(self, params) -> None:
        """Fill the per-sequence settings buffers from a `sampling.SamplingParams` (scalars or one value per sequence;
        seed=None draws the seeds from torch's default CPU generator). They stay until the next call."""
        if self.score_mode:                      # a score has no seed: none is drawn from the generator, a given one is ignored
            from dataclasses import replace
            T, k, p, _ = replace(params, seed=0).resolve(self.B)
            for buf, a in ((self.samp_temperature, T), (self.samp_top_k, k), (self.samp_top_p, p)):
                buf.copy_(torch.from_numpy(a.copy()))
            return
        if not self.sample:
            raise ValueError("engine was not built with sample=True or score=True")
        T, k, p, seed = params.resolve(self.B)
        for buf, a in ((self.samp_temperature, T), (self.samp_top_k, k), (self.samp_top_p, p), (self.samp_seed, seed)):
            buf.copy_(torch.from_numpy(a))

    def set_forced_ids(self, forced_ids: torch.Tensor, check: bool = True) -> None:
        """The tokens a score=True engine scores and conditions its decode steps on: int64 [B, n_new], copied into the
        static `gen_ids` buffer (valid before eager and captured runs alike). The ids are checked against the vocabulary
        (the next step's embedding lookup must not see one outside it), which for ids on the device costs a host
        synchronisation; check=False skips it for a caller that has made sure itself."""
        if not self.score_mode:
            raise ValueError("engine was not built with score=True")
        if tuple(forced_ids.shape) != (self.B, self.n_new) or forced_ids.dtype != torch.int64:
            raise ValueError(f"forced_ids must be int64 {(self.B, self.n_new)}, got {forced_ids.dtype} {tuple(forced_ids.shape)}")
        if check and (bool((forced_ids < 0).any()) or bool((forced_ids >= self.dims.vocab).any())):
            raise ValueError(f"forced_ids must lie in [0, {self.dims.vocab})")
        self.gen_ids.copy_(forced_ids.t())

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, pixel_values: torch.Tensor, sampling=None) -> torch.Tensor:
        """n_new tokens for every sequence: greedy, or on a sample=True engine drawn under `sampling` (None: the settings
        already in the buffers; the weight pairs are left in `gen_wt`). Returns int64 [B, n_new] (device tensor; no host
        sync inside)."""
        if sampling is not None:
            self.set_sampling(sampling)
        self.set_inputs(input_ids, pixel_values)
        self.replay()
        return self.result().ids if self.beams else self.gen_ids.t()

    @torch.no_grad()
    def score(self, input_ids: torch.Tensor, pixel_values: torch.Tensor, forced_ids: torch.Tensor, sampling=None):
        """The counterpart of `generate` on a score=True engine: run the plan conditioned on `forced_ids` [B, n_new] under
        `sampling` (None: the settings already in the buffers). Returns wt int64 [B, n_new, 2] = every forced token's
        (kept weight, kept total) — with score_range, the pair (wt, range_wt int32 [B, n_new, count]) — as views of the
        static buffers (device tensors; no host sync inside)."""
        if sampling is not None:
            self.set_sampling(sampling)
        self.set_forced_ids(forced_ids)
        self.set_inputs(input_ids, pixel_values)
        self.replay()
        r = self.result()
        return present(r.wt, r.range_wt)

    def beam_trace(self, own=lambda x: x) -> BeamTrace:
        """The last run's survivors step by step, as views of the static buffers (`own=torch.clone`: copies): what
        `beam.backtrack` takes, and the scores that rank the finished sequences (`scores[-1]`)."""
        if not self.beams:
            raise ValueError("engine was not built with beams=")
        return BeamTrace(tokens=own(self.gen_ids), parents=own(self.beam_parent), wt=own(self.gen_wt), scores=own(self.beam_scores))

    def _backtrack(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """`beam.backtrack` on the device (index copies on the current stream, no host sync): ids int64 [B, n_new] and wt
        int64 [B, n_new, 2] of every prompt's W finished sequences, best first."""
        rows = torch.arange(self.B, device=self.device)
        first, slot = rows // self.beams * self.beams, rows
        ids, wt = torch.empty_like(self.gen_ids.t()), torch.empty_like(self.gen_wt.permute(1, 0, 2))
        for t in range(self.n_new - 1, -1, -1):
            ids[:, t], wt[:, t] = self.gen_ids[t][slot], self.gen_wt[t][slot]
            slot = first + self.beam_parent[t][slot]
        return ids, wt

    def result(self, own=lambda x: x) -> EngineResult:
        """The last run as one record; `own` is applied to every tensor (identity: views of the static buffers, which the
        next run overwrites; `torch.clone`: copies). Device tensors, no host sync. A beam engine's `ids` / `wt` are the
        backtracked sequences (new tensors either way): row e·W + k is prompt e's k-th best."""
        ids, wt = self._backtrack() if self.beams else (self.gen_ids.t(), self.gen_wt.permute(1, 0, 2) if self.sample or self.score_mode else None)
        return EngineResult(ids=own(ids), wt=None if wt is None else own(wt),
                            range_wt=None if self.gen_range_wt is None else own(self.gen_range_wt.permute(1, 0, 2)),
                            values=None if self.values is None else own(self.value_result()),
                            attention=self.action_attention(own) if self.attn_taps is not None and not self.all_rows else None)
