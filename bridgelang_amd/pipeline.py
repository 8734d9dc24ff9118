"""Software pipelines over batches for throughput serving: `TwoStagePipeline` (two batches in flight) and
`StaggeredDecodePipeline` (n_new batches in flight, their decode iterations merged into one weight pass per step).


A `predict_action` batch has two very different halves: vision + prefill is MFMA-bound (≈ 65 ms at B = 16) but leaves
CUs idle in partial GEMM rounds and between dependent launches; the 6 cached decode steps are HBM-bound weight streaming
(≈ 27 ms). `TwoStagePipeline` keeps two engines (two sets of activations / KV caches over ONE set of weights) and, per
step, runs stage 1 (vision → projector → prefill → first token) of the batch submitted NOW on one stream while stage 2
(decode steps 1..6) of the batch submitted ONE STEP EARLIER runs on a second stream; the step completes one batch.
Work per step is exactly one batch's full computation; only the latency of an individual batch is two steps.
Each of the two stage pairings is captured once as a HIP graph with fork/join stream dependencies.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .engine import OpenVLAEngine, present
from .llm_plan import decode_fused, decode_layer, head, head_fused
from .ops import Op
from .weights import VLAWeights


class TwoStagePipeline:
    def __init__(self, weights: VLAWeights, batch: int, prompt_len: int, n_new: int = 7):
        self.engines = [OpenVLAEngine(weights, batch, prompt_len, n_new) for _ in range(2)]
        self.device = weights.embed.device
        self._decode_stream = torch.cuda.Stream(device=self.device)
        self._graphs: List[Optional[torch.cuda.CUDAGraph]] = [None, None]
        self._tick = 0

    def _run_pair(self, k: int) -> None:
        """stage 1 of engine k ‖ stage 2 of engine 1-k."""
        e1, e2 = self.engines[k], self.engines[1 - k]
        main = torch.cuda.current_stream()
        self._decode_stream.wait_stream(main)
        with torch.cuda.stream(self._decode_stream):
            for step in e2.decode_ops:
                ops.run_all(step)
        e1.run_vision()
        ops.run_all(e1.projector_ops + e1.prefill_ops)
        main.wait_stream(self._decode_stream)

    def capture(self) -> None:
        for k in (0, 1):
            self._run_pair(k)          # eager warm-up (also sets kernel attributes outside capture)
        torch.cuda.synchronize()
        for k in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run_pair(k)
            self._graphs[k] = g

    @torch.no_grad()
    def step(self, input_ids: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Submit a batch (or re-use the inputs already resident in the engine's buffers when None) and return the
        [B, n_new] token ids of the batch submitted one step earlier (garbage on the very first call)."""
        k = self._tick & 1
        if input_ids is not None:
            self.engines[k].set_inputs(input_ids, pixel_values)
        if self._graphs[k] is not None:
            self._graphs[k].replay()
        else:
            self._run_pair(k)
        self._tick += 1
        return self.engines[1 - k].gen_ids.t()

    def flush(self) -> torch.Tensor:
        """Finish the batch still in stage 1 (drain the pipeline); returns its ids."""
        k = (self._tick - 1) & 1
        for step in self.engines[k].decode_ops:
            ops.run_all(step)
        return self.engines[k].gen_ids.t()


class StaggeredDecodePipeline:
    """n_new batches in flight, one submitted and one completed per step (continuous batching for a fixed-length decode).

    A cached decode iteration streams all 13.2 GB of Llama weights for B = 16 rows, six times per batch. With one batch
    submitted per step, the batches submitted 1, 2, … n_new-1 steps ago are exactly at decode iterations 1, 2, … n_new-1:
    their rows are stacked into ONE (n_new-1)·B-row iteration, so every weight matrix is streamed once per step instead of
    n_new-1 times (the rows go through the tiled GEMMs; only attention — own KV cache, own position — runs per batch).
    Per step: vision + projector + prefill of the new batch on one stream ‖ the merged decode iteration on another; the
    work per step is exactly one batch's full computation, a batch's latency is n_new steps. Slot s of the n_new slots
    (KV caches, ids, prefill activations = one OpenVLAEngine each) holds the batch submitted at step ≡ s (mod n_new); the
    n_new slot rotations are captured as n_new HIP graphs.

    Results per sequence equal the plain engine's bit for bit: the stacked rows go through kernels that reproduce the
    per-batch kernels' fp32 summation order (_plan_merged; tests/test_pipeline_gpu.py).

    padded=True serves prompts of DIFFERENT lengths (up to prompt_len) from the one set of slots and graphs: every slot is
    an `OpenVLAEngine(padded=True)`, a batch arrives right-padded with its attention mask (`step(..., attention_mask)`),
    and in the merged iteration every sequence rotates, appends and attends at its own position — the slot engine's
    device-side `rope_pos` rows, read by bl_attention_decode_rope_pos_grouped_bf16. Every sequence gets the ids and logits
    of its own un-padded batch-1 run, bit for bit (tests/test_pipeline_padded_gpu.py).
    """

    def __init__(self, weights: VLAWeights, batch: int, prompt_len: int, n_new: int = 7, split_vision: bool = False,
                 fp8: bool = False, padded: bool = False, sample: bool = False, score: bool = False,
                 score_range: Optional[Tuple[int, int]] = None, vocab_range: Optional[Tuple[int, int]] = None,
                 attn_taps=None, value: Optional[str] = None, value_head=None):
        """split_vision=True adds a third stage: the vision towers + projector of the batch submitted NOW run beside the
        Llama prefill of the batch submitted one step earlier (n_new + 1 slots, latency n_new + 1 steps).
        score=True (with score_range, as OpenVLAEngine's) scores given tokens instead of producing them: every slot is an
        `OpenVLAEngine(score=True)`, `step(..., forced_ids=, sampling=)` fills the slot's forced ids and settings, and the
        merged iteration ends in bl_score_f32 per group where a sampling pipeline draws. vocab_range=(first, count), with
        sample=True or score=True, is OpenVLAEngine's: every draw and score is under the policy restricted to that range.
        value="action" | "token" with value_head= is OpenVLAEngine's critic: every slot engine's prefill carries its
        bl_value_predict_f32, at "token" the merged iteration adds one per group beside that group's pick, over the group's
        rows of the stacked residual; step() / flush() append the finished batch's values ([B] / [B, n_new])."""
        if attn_taps is not None:
            raise ValueError("StaggeredDecodePipeline has no attention taps: its merged decode iteration runs several batches' "
                             "rows in one launch; use OpenVLAEngine(attn_taps=...)")
        if n_new < 2:
            raise ValueError("StaggeredDecodePipeline needs at least one decode iteration (n_new >= 2)")
        if padded and fp8:
            raise ValueError("padded generation is built for the bf16 generation plan")
        self.padded, self.sample, self.score = padded, sample, score
        self.w, self.dims, self.B, self.n_new = weights, weights.dims, batch, n_new
        self.split_vision = split_vision
        self.lag = 1 if split_vision else 0         # steps between a batch's submission and its prefill
        self.slots = n_new + self.lag
        self.engines = [OpenVLAEngine(weights, batch, prompt_len, n_new, fp8=fp8, padded=padded, sample=sample, score=score,
                                      score_range=score_range, vocab_range=vocab_range, value=value, value_head=value_head)
                        for _ in range(self.slots)]
        self.value = value
        self.vocab_range = self.engines[0].vocab_range
        self.device = dev = weights.embed.device
        d = self.dims
        G = n_new - 1
        M = G * batch
        z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype, device=dev)
        self.xd, self.hd, self.aod = z(M, d.llm_dim), z(M, d.llm_dim), z(M, d.llm_dim)
        self.qkvd, self.actd = z(M, 3 * d.llm_dim), z(M, d.llm_inter)
        self.logits = z(M, d.vocab, dtype=torch.float32)       # rows (g-1)·B … g·B: decode iteration g of this step
        # fp32 partials of the merged decode GEMMs of the narrow layers (N = llm_dim: four workgroups share K — an exact
        # split of the skinny order's binary tree, see bl_gemm_skinny_rows_bf16)
        self.ws = torch.empty(4 * min(M, 128) * d.llm_dim * 4, dtype=torch.uint8, device=dev)
        self._decode_stream = torch.cuda.Stream(device=dev)
        self._vision_stream = torch.cuda.Stream(device=dev)
        self._main_stream = torch.cuda.Stream(device=dev)    # capture stream (stream priorities were tried: no effect)
        self.merged_ops: List[List[Op]] = [self._plan_merged(k) for k in range(self.slots)]
        self._graphs: List[Optional[torch.cuda.CUDAGraph]] = [None] * self.slots
        self._tick = 0

    def _plan_merged(self, k: int) -> List[Op]:
        """Decode iteration g = 1 … n_new-1 of the batch in slot (k - g) mod n_new, all in one pass over the weights:
        llm_plan.decode_layer and llm_plan.head — the layer and head OpenVLAEngine._plan_decode emits for ONE batch —
        over the stacked rows, with the launch forms below."""
        d, w, B, D, e0, M = self.dims, self.w, self.B, self.dims.llm_dim, self.engines[0], self.xd.shape[0]
        fused = decode_fused(B, d)
        groups = [(g, self.engines[(k - g - self.lag) % self.slots], slice((g - 1) * B, g * B)) for g in range(1, self.n_new)]

        def lin(A, W, out, epi, res=None):
            """One Linear over the stacked rows, in the arithmetic the engine uses for B rows: where the engine streams
            weights through bl_gemm_skinny_bf16 (B <= 16), the stacked rows go through bl_gemm_skinny_rows_bf16 in slices
            of 128 rows (same 8-way K partition and combine order); where the engine falls back to the tiled kernels, so
            does this plan (no split-K workspace: the tiled kernels' K order does not depend on the row count)."""
            if not ops.skinny_supported(B, A.shape[1], epi):
                return [ops.gemm(A, W, out, epi, res=res, skinny=False, run=False)]
            return [ops.gemm(A[r0:r0 + 128], W, out[r0:r0 + 128], epi, res=None if res is None else res[r0:r0 + 128],
                             skinny_rows=True, workspace=self.ws, run=False) for r0 in range(0, M, 128)]

        def norm_lin(x, norm_w, W, out, epi, fused=fused):
            """The engine's fused a_norm becomes bl_rmsnorm_skinny_bf16 (its arithmetic) ahead of the linear; its separate
            RMSNorm stays bl_rmsnorm_bf16. Hence ids and logits equal the plain engine's bit for bit
            (tests/test_pipeline_gpu.py, tests/test_full_size_gpu.py)."""
            return [(ops.rmsnorm_skinny if fused else ops.rmsnorm)(x, norm_w, self.hd, d.rms_eps, run=False)] + lin(self.hd, W, out, epi)

        def attn(l):
            """Own KV cache, own position: attention runs per batch, as each slot engine's own (against the one pair of
            rope tables) — or, for up to 8 fused iterations, all of them in one launch."""
            if not (fused and len(groups) <= 8):
                return [op for g, e, r in groups for op in e._decode_attn(l, g, self.qkvd[r], self.aod[r], fused, (e0.cos, e0.sin))]
            # padded: group g's sequences sit at their own positions, row g of the slot engine's device-side rope_pos
            at = (dict(rope_pos=[e.rope_pos[g] for g, e, _ in groups]) if self.padded else
                  dict(pos=[e.S + g - 1 for g, e, _ in groups]))
            return [ops.attention_decode_rope_grouped(
                self.qkvd, [e.k_cache[l] for _, e, _ in groups], [e.v_cache[l] for _, e, _ in groups], self.aod,
                e0.cos, e0.sin, B=B, H=d.llm_heads, head_dim=d.head_dim, run=False, **at)]

        plan = [ops.embed_splice(e.gen_ids[g - 1].view(B, 1), w.embed, self.xd[r].view(B, 1, D), 0, run=False)
                for g, e, r in groups]
        for l, lw in enumerate(w.layers):
            plan += decode_layer(l, lw, self.xd, self.qkvd, self.aod, self.actd, norm_lin, lin, attn)
        # iteration g of a batch draws with ITS slot's settings at Philox counter g, as its engine would — or scores ITS
        # slot's forced token g, which the next iteration's embedding consumes unchanged
        return plan + head(w, self.xd, self.logits, functools.partial(norm_lin, fused=head_fused(B, d)),
                           [e._pick(self.logits[r], g) for g, e, r in groups]
                           + [op for g, e, r in groups for op in e._value(self.xd[r], g)])

    def _run_tick(self, k: int) -> None:
        """stage 1 of slot k ‖ the merged decode iteration over the other slots."""
        e1 = self.engines[k]
        main = torch.cuda.current_stream()
        self._decode_stream.wait_stream(main)
        with torch.cuda.stream(self._decode_stream):
            ops.run_all(self.merged_ops[k])
        if self.split_vision:
            vs, ss = self._vision_stream, e1._side      # both towers fork from the main stream (no nested fork)
            vs.wait_stream(main)
            ss.wait_stream(main)
            with torch.cuda.stream(ss):
                ops.run_all(e1.siglip_ops)
            with torch.cuda.stream(vs):
                ops.run_all(e1.dino_ops)
                vs.wait_stream(ss)
                ops.run_all(e1.projector_ops)
            ops.run_all(self.engines[(k - 1) % self.slots].prefill_ops)
            main.wait_stream(vs)
        else:
            e1.run_vision()
            ops.run_all(e1.projector_ops + e1.prefill_ops)
        main.wait_stream(self._decode_stream)

    def capture(self) -> None:
        for k in range(self.slots):
            self._run_tick(k)          # eager warm-up (also sets kernel attributes outside capture)
        torch.cuda.synchronize()
        for k in range(self.slots):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self._main_stream):
                self._run_tick(k)
            self._graphs[k] = g

    @torch.no_grad()
    def step(self, input_ids: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
             attention_mask: Optional[torch.Tensor] = None, mask_checked: bool = False, sampling=None,
             forced_ids: Optional[torch.Tensor] = None, ids_checked: bool = False):
        """Submit a batch (None: re-use the inputs resident in the slot's buffers) and return the [B, n_new] ids of the
        batch submitted n_new-1 steps earlier, which this step completed (garbage until the pipeline has filled). The
        returned view is overwritten by the next step() — copy it first. A padded pipeline takes right-padded prompts with
        their `attention_mask` [B, prompt_len] (1…1 0…0; None: all ones); the slot keeps the masks and positions derived
        from it until its batch completes (with split_vision its prefill reads them one step later). The mask's layout is
        checked on the device, which costs a host synchronisation per step; `mask_checked=True` skips it for a caller
        that built the masks itself (the server), so submission stays asynchronous like the un-padded one.
        A sample=True pipeline takes the submitted batch's `sampling` (a SamplingParams; None: every sequence greedy) into
        the slot's settings buffers, where they stay until the batch completes, and returns the pair (ids [B, n_new],
        wt [B, n_new, 2]) — both views that the next step() overwrites.
        A score=True pipeline takes the submitted batch's `forced_ids` [B, n_new] (required with input_ids; checked
        against the vocabulary unless `ids_checked=True`, a host synchronisation for ids on the device) and `sampling`
        into the slot, and returns the completed batch's wt [B, n_new, 2] — with score_range the pair (wt, range_wt
        [B, n_new, count]) — again views.
        A pipeline built with value= appends the completed batch's values (fp32 [B] at "action", [B, n_new] at "token") as
        the last element of whatever it returns otherwise, a view like the others."""
        k = self._tick % self.slots
        if sampling is not None and (not (self.sample or self.score) or input_ids is None):
            raise ValueError("sampling goes with the input_ids of a pipeline built with sample=True or score=True")
        if (forced_ids is not None) != (self.score and input_ids is not None):
            raise ValueError("forced_ids goes with the input_ids of a pipeline built with score=True, and every batch "
                             "submitted to such a pipeline needs them")
        if input_ids is not None and (self.sample or self.score):
            from .sampling import SamplingParams
            self.engines[k].set_sampling(sampling if sampling is not None else SamplingParams(temperature=0.0))
        if forced_ids is not None:
            self.engines[k].set_forced_ids(forced_ids, check=not ids_checked)
        if attention_mask is not None and (not self.padded or input_ids is None):
            raise ValueError("attention_mask goes with the input_ids of a pipeline built with padded=True")
        if input_ids is not None and self.padded:
            mask = attention_mask if attention_mask is not None else torch.ones_like(input_ids)
            self.engines[k].set_padded_inputs(input_ids, pixel_values, mask, check=not (mask_checked or attention_mask is None))
        elif input_ids is not None:
            self.engines[k].set_inputs(input_ids, pixel_values)
        if self._graphs[k] is not None:
            self._graphs[k].replay()
        else:
            self._run_tick(k)
        self._tick += 1
        return self._result(self.engines[(k + 1) % self.slots], lambda x: x)

    def _result(self, e: OpenVLAEngine, own):
        """What step() / flush() hand out for a slot's finished batch (`own`: identity for views, clone for copies)."""
        r = e.result(own)
        return present(None if self.score else r.ids, r.wt, r.range_wt, r.values)

    def flush(self, ticks: Optional[Sequence[int]] = None) -> List[Optional[torch.Tensor]]:
        """Drain: finish the batches still in flight with each slot's own per-batch plans; returns their ids oldest
        first (copies), one entry per step of the last `slots - 1` steps. `ticks`: finish only the batches submitted at
        these step indices (None entries for the others) — a server that already answered the older slots skips them.
        A sample=True pipeline returns (ids, wt) pairs, a score=True pipeline what its step() returns."""
        out: List[Optional[torch.Tensor]] = []
        for a in range(min(self.slots - 2, self._tick - 1), -1, -1):    # a = steps since the batch was submitted
            tick = self._tick - 1 - a
            if ticks is not None and tick not in ticks:
                out.append(None)
                continue
            e = self.engines[tick % self.slots]
            j = a - self.lag                                            # decode iterations already done (-1: not prefilled)
            if j < 0:
                ops.run_all(e.prefill_ops)
                j = 0
            for step in e.decode_ops[j:]:
                ops.run_all(step)
            out.append(self._result(e, torch.clone))
        return out
