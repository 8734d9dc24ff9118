"""`OpenVLAForActionPrediction` on MI355X: the reference's HF-style model surface over the HIP engine.

Drop-in for prismatic/extern/hf/modeling_prismatic.py: same class names, `forward()` keyword list and output dataclass
(:291-304, :162-173), `predict_action(input_ids, unnorm_key, **kwargs)` (:506-536), `get_action_dim` /
`get_action_stats` / `_check_unnorm_key` (:538-562) and the attributes callers read (`norm_stats`, `bins`,
`bin_centers`, `vocab_size`, `config.image_sizes`, `vision_backbone.featurizer.patch_embed.num_patches` —
finetune.py:219,270). What sits behind it is not timm/transformers/flash-attn but bridgelang_amd.engine (hand-written
gfx950 kernels); there is no eager/PyTorch fallback, so constructing the model without a GPU + built library raises.

The classes are real `transformers.PreTrainedModel` subclasses, so the reference's callers load them the way they load
the reference (`AutoConfig.register` / `AutoModelForVision2Seq.register` + `from_pretrained(local_dir, torch_dtype=
torch.bfloat16, low_cpu_mem_usage=True, trust_remote_code=True)`, finetune.py:151-166, deploy.py:66-75,
run_openvla_demo.py:21-28 — `register_auto_classes()` below; transformers >= 5 renamed the Auto class to
`AutoModelForImageTextToText`, both are served). `from_pretrained` reads the safetensors shards straight into the packed
weight arena on the GPU (no nn.Parameter copies of the 15 GB checkpoint); `.to()` / `.eval()` / `.device` / `.dtype`
behave as on any HF model as long as the target is the GPU the weights already live on and bf16. The model owns no
nn.Parameters (the weights are the arena), so autograd-based wrappers (PEFT, DDP) have nothing to hook: training goes
through bridgelang_amd.training (vla-scripts/finetune.py, vla-scripts/train.py keep the reference scripts' flags).

Differences from the reference, all deliberate:
  * batched `predict_action` is supported (returns [B, 7]); batch 1 returns the reference's 1-D array.
  * batched generation takes RIGHT-padded prompts + attention_mask (the collator's layout); every sequence gets the ids
    it gets alone (the reference asserts batch 1 in its cached branch, :326, :460-463).
  * the greedy loop runs on-device (no per-token host sync). Sampling runs on the device too, through `sampling=
    SamplingParams(...)` (seeded Philox draws with temperature / top-k / top-p, bridgelang_amd/sampling.py) and
    `sample_actions`; `do_sample=True` alone is rejected: HF draws from torch's global device RNG stream, which this path
    does not reproduce. The opposite direction runs there as well: `score_actions` / `generate(forced_ids=)` return the
    log-probabilities of GIVEN action tokens under the same warped distribution, bit for bit what the sampler reports
    when it draws them (`token_ids_from_actions` is the action tokenizer's encoding, for candidates given as actions).
  * when 29871 is appended to the prompt the attention mask is extended with it (reference quirk C.1).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from transformers import PreTrainedModel

from ...attention_taps import ActionAttention, AttnTaps, prompt_segments
from ...beam import MAX_BEAMS
from ...engine import EngineResult, OpenVLAEngine, present
from ...sampling import SamplingParams, derive_seed, logprob
from ...weights import TowerDims, VLADims, VLAWeights, allocate
from .configuration_prismatic import OpenVLAConfig, PrismaticConfig

IGNORE_INDEX = -100

# timm id → tower geometry (timm 0.9.10 model definitions)
_TIMM_GEOMETRY = {
    "vit_large_patch14_reg4_dinov2.lvd142m": dict(dim=1024, depth=24, heads=16, mlp=4096, n_prefix=5, layerscale=True),
    "vit_so400m_patch14_siglip_224": dict(dim=1152, depth=27, heads=16, mlp=4304, n_prefix=0, layerscale=False),
}


def dims_from_config(config: PrismaticConfig) -> VLADims:
    if not config.use_fused_vision_backbone or len(config.timm_model_ids) != 2:
        raise NotImplementedError("only the fused DINOv2+SigLIP backbone is on the MI355X path")
    a, b = (_TIMM_GEOMETRY[i] for i in config.timm_model_ids)
    tc = config.text_config
    if tc.num_key_value_heads not in (None, tc.num_attention_heads):
        raise NotImplementedError("grouped-query attention is not on the Llama-2 path")
    return VLADims(dino=TowerDims("vision_backbone.featurizer", chan0=0, **a),
                   siglip=TowerDims("vision_backbone.fused_featurizer", chan0=3, **b),
                   llm_dim=tc.hidden_size, llm_layers=tc.num_hidden_layers, llm_heads=tc.num_attention_heads,
                   llm_inter=tc.intermediate_size, vocab=tc.vocab_size, rms_eps=tc.rms_norm_eps,
                   rope_theta=float(getattr(tc, "rope_theta", None) or 10000.0),
                   max_pos=min(tc.max_position_embeddings, config.llm_max_length), name=config.llm_backbone_id)


@dataclass
class PrismaticCausalLMOutputWithPast:
    """Field-for-field the reference's output class (modeling_prismatic.py:162-173)."""
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Optional[Any] = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor]] = None
    projector_features: Optional[torch.Tensor] = None

    def to_tuple(self) -> tuple:
        return tuple(v for v in (self.loss, self.logits, self.past_key_values, self.hidden_states, self.attentions,
                                 self.projector_features) if v is not None)


class PrismaticPreTrainedModel(PreTrainedModel):
    """modeling_prismatic.py:176-213: the HF base class of the reference's models (config class, support flags)."""
    config_class = PrismaticConfig
    base_model_prefix = "model"
    supports_gradient_checkpointing = False
    _no_split_modules = ["PrismaticProjector"]
    _skip_keys_device_placement = "past_key_values"
    _supports_flash_attn_2 = True      # attention is this package's own kernel: every attn_implementation request is
    _supports_flash_attn = True        # accepted and means the same thing
    _supports_sdpa = True
    _supports_attention_backend = True

    def _init_weights(self, module) -> None:   # weights come from a checkpoint or init_synthetic(); nothing to initialise
        return


class PrismaticForConditionalGeneration(PrismaticPreTrainedModel):
    config_class = PrismaticConfig
    _ENGINE_CACHE = 8          # captured engines kept per model (LRU): each holds KV caches + activations + a HIP graph

    def __init__(self, config: PrismaticConfig, device: Union[str, torch.device, None] = None,
                 dims: Optional[VLADims] = None) -> None:
        super().__init__(config)
        if config.use_fused_vision_backbone is None:
            raise ValueError("Missing config field `use_fused_vision_backbone`")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self._device = torch.device(device)
        self.dims = dims if dims is not None else dims_from_config(config)
        self.weights: VLAWeights = allocate(self.dims, self._device)
        self.vocab_size = self.dims.vocab
        self.pad_token_id = config.pad_token_id
        self._engines: "OrderedDict[tuple, OpenVLAEngine]" = OrderedDict()
        self._forward_engines: "OrderedDict[tuple, OpenVLAEngine]" = OrderedDict()
        # attribute path read by finetune.py:270
        self.vision_backbone = SimpleNamespace(
            featurizer=SimpleNamespace(patch_embed=SimpleNamespace(num_patches=self.dims.n_patches)),
            embed_dim=self.dims.vision_dim)
        self.post_init()

    # ---- HF plumbing over the arena ----
    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def dtype(self) -> torch.dtype:
        return torch.bfloat16

    def to(self, *args, **kwargs):
        """nn.Module.to for a model whose weights are a packed bf16 arena on one GPU: a no-op for the device / dtype it
        already has (what `from_pretrained(...).to("cuda:0")` asks for), an error otherwise — load with `device=` instead."""
        device, dtype, _, _ = torch._C._nn._parse_to(*args, **kwargs)
        if dtype is not None and dtype != torch.bfloat16:
            raise NotImplementedError(f"the MI355X path computes in bfloat16; .to({dtype}) is not available")
        if device is not None:
            want = torch.device(device)
            if want.type == "cuda" and want.index is None:
                want = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
            if want != self._device:
                raise NotImplementedError(f"weights live on {self._device}; pass device={want!s} to from_pretrained() / the "
                                          f"constructor instead of moving the arena")
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device) if isinstance(device, int) else (device or "cuda"))

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("this class is the inference surface; training runs through bridgelang_amd.training "
                                      "(vla-scripts/train.py, vla-scripts/finetune.py)")
        return super().train(False)

    # ---- weights ----
    def init_synthetic(self, seed: int = 0, recipe: str = "init") -> "PrismaticForConditionalGeneration":
        self.weights.fill_synthetic(seed, recipe)
        return self

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True, assign: bool = False):
        self.weights.load_state_dict(state_dict, strict=strict)
        return self

    def state_dict(self, *args, **kwargs) -> Dict[str, torch.Tensor]:
        """HF-named tensors (unpacked copies), incl. the never-executed ones the reference loads strictly."""
        return self.weights.state_dict()

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config: Optional[PrismaticConfig] = None,
                        device: Union[str, torch.device, None] = None, device_map: Any = None,
                        dims: Optional[VLADims] = None, torch_dtype: Any = None, dtype: Any = None, **kwargs: Any):
        """LOCAL HF export (`config.json` + `*.safetensors` [+ index], convert_openvla_weights_to_hf.py:235-249) →
        model on the GPU. Shards are streamed one at a time straight into the packed arena; nothing is fetched from the
        hub; files are read with safetensors / json only. Accepted and ignored for call-site compatibility:
        `trust_remote_code`, `low_cpu_mem_usage`, `attn_implementation`, `quantization_config=None`, …"""
        from ...models.load import load_hf_directory
        for k in (torch_dtype, dtype):
            if k not in (None, torch.bfloat16, "bfloat16", "auto"):
                raise NotImplementedError(f"only torch_dtype=torch.bfloat16 is available on the MI355X path (got {k})")
        if kwargs.get("quantization_config") is not None:
            raise NotImplementedError("bitsandbytes quantisation is a CUDA path; not available here")
        if device is None and isinstance(device_map, (str, int, torch.device)) and device_map not in ("auto", "balanced"):
            device = device_map
        return load_hf_directory(cls, pretrained_model_name_or_path, config=config, device=device, dims=dims)

    def save_pretrained(self, save_directory, *args, max_shard_size: Union[int, str] = 5 << 30, **kwargs) -> None:
        """`config.json` + sharded safetensors under HF names (reference callers: finetune.py:322-337)."""
        from ...models.load import save_pretrained as _save
        if isinstance(max_shard_size, str):
            num, unit = float(max_shard_size[:-2]), max_shard_size[-2:].upper()
            max_shard_size = int(num * {"KB": 1 << 10, "MB": 1 << 20, "GB": 1 << 30}[unit])
        _save(self, save_directory, max_shard_bytes=int(max_shard_size))

    def _lru(self, cache: "OrderedDict", key: tuple, build):
        """Engines are heavy (KV caches, activations, a captured graph): keep the most recently used few per model and
        drop the rest, so a server seeing many (batch, prompt length) pairs cannot run HBM dry."""
        eng = cache.get(key)
        if eng is None:
            eng = cache[key] = build()
            while len(cache) > self._ENGINE_CACHE:
                cache.popitem(last=False)
        else:
            cache.move_to_end(key)
        return eng

    def engine(self, batch: int, prompt_len: int, n_new: int = 7, padded: bool = False, cached: bool = False,
               sample: bool = False, score: bool = False, score_range: Optional[Tuple[int, int]] = None,
               vocab_range: Optional[Tuple[int, int]] = None, use_adapters: Optional[bool] = None,
               attn_taps: Optional[AttnTaps] = None, value: Optional[str] = None, beams: Optional[int] = None,
               group: Optional[int] = None) -> OpenVLAEngine:
        """`group` (G): the engine whose `batch` rows are `batch` / G prompts with one shared prefill each
        (`OpenVLAEngine(group=)`, behind `share_prefill=True`); part of the cache key only when given.
        `beams` (W): the beam-search engine of `batch` / W prompts (`OpenVLAEngine(beams=)`); part of the cache key only
        when given.
        `value` ("action" | "token", see `attach_value_head`): an engine whose plan also evaluates the attached value
        head; the level and the head's identity join the cache key only when given.
        `attn_taps` (attention_taps.AttnTaps): an engine whose plan records where the action tokens attend; part of the
        cache key only when given, so the engines of every other call are the ones they were.
        `use_adapters` (see `attach_adapters`): None = the adapted weights if adapters are attached, False = the base
        model, True = the adapted weights or an error. Part of the cache key; adapted engines are built over
        `lora.adapted_weights()`.
        `cached=True`: the engine behind a `forward(..., use_cache=True)` KV-cache handle — keyed apart from the engines
        `predict_action` / `generate` use, so an interleaved action prediction of the same shape does not invalidate the
        caller's cache (each kind has its own LRU slot; a second cached prefill of the same shape still does).
        `score=True` (with `score_range`) is a kind of its own again: the engines that score given tokens. `vocab_range`
        (sample=True / score=True: the restricted policy) is fixed per engine, so it is part of the key as well."""
        fp8 = bool(getattr(self, "fp8", False))       # `model.fp8 = True`: W8A8 e4m3 Llama prefill projections (extension)
        if vocab_range is not None:
            vocab_range = (int(vocab_range[0]), int(vocab_range[1]))
        adapted = self._resolve_adapters(use_adapters)
        if adapted and fp8 and not self._adapters.fp8_enabled:
            raise NotImplementedError("fp8=True with attached adapters: the derived e4m3 weight copies would go stale on every "
                                      "refresh of the adapted weights. Opt in with attach_adapters(lora, fp8=True) / "
                                      "load_adapter(dir, fp8=True) or lora.enable_fp8(): the refresh then requantises them on the device")
        weights = self._adapters.adapted_weights() if adapted else self.weights
        key = (batch, prompt_len, n_new, fp8, padded, cached, sample) + (("score", score_range) if score else ()) + \
            (("vocab", vocab_range) if vocab_range is not None else ()) + (("adapted",) if adapted else ()) + \
            ((("taps", attn_taps.key(self.dims.llm_layers)),) if attn_taps is not None else ()) + \
            ((("value", value, id(self._value_head)),) if value is not None else ()) + \
            ((("beams", int(beams)),) if beams is not None else ()) + ((("group", int(group)),) if group is not None else ())
        return self._lru(self._engines, key,
                         lambda: OpenVLAEngine(weights, batch, prompt_len, n_new=n_new, fp8=fp8 and not padded, padded=padded,
                                               sample=sample, score=score, score_range=score_range, vocab_range=vocab_range,
                                               attn_taps=attn_taps, value=value,
                                               value_head=self._value_head if value is not None else None, beams=beams,
                                               **({} if group is None else dict(group=group))))

    # ---- where the action tokens attend (attention_taps.py) ----
    @staticmethod
    def _attn_taps(return_attention: Optional[str], attention_layers) -> Optional[AttnTaps]:
        if return_attention is None:
            if attention_layers is not None:
                raise ValueError("attention_layers goes with return_attention=")
            return None
        if return_attention not in ("segments", "full", "both"):
            raise ValueError(f'return_attention must be None, "segments", "full" or "both", got {return_attention!r}')
        return AttnTaps(layers=None if attention_layers is None else tuple(int(l) for l in attention_layers),
                        full=return_attention != "segments", segments=return_attention != "full")

    @torch.no_grad()
    def attention_maps(self, input_ids: torch.LongTensor, pixel_values: Optional[torch.Tensor] = None,
                       attention_mask: Optional[torch.Tensor] = None, layers=None) -> tuple:
        """HF's `attentions` for the all-position forward of these inputs (multimodal, or language-only without
        pixel_values): a tuple with one entry per decoder layer, fp32 [B, H, S, S] (S = 256 + L, or L), None for a layer
        outside `layers` (None: all). Row i of an entry is query i's softmax over the keys it sees (causal, pads hidden);
        computed by bl_attention_probs_f32 from the layer's own q and cached keys, never rounded to bf16."""
        from ...forward_full import _all_rows_engine, forward_all_rows
        taps = AttnTaps(layers=None if layers is None else tuple(int(l) for l in layers), full=True, segments=False)
        forward_all_rows(self, input_ids, attention_mask, pixel_values, None, attn_taps=taps)
        eng = _all_rows_engine(self, input_ids.shape[0], input_ids.shape[1], pixel_values is None, taps)
        return tuple(None if m is None else m.clone() for m in eng.attention_maps())

    # ---- LoRA adapters: inference under merged weights beside the frozen base (training/lora.py) ----
    _adapters = None           # the attached training.lora.LoraAdapters

    def _resolve_adapters(self, use_adapters: Optional[bool]) -> bool:
        if use_adapters and self._adapters is None:
            raise ValueError("use_adapters=True, but no adapters are attached (attach_adapters / load_adapter)")
        return self._adapters is not None and use_adapters is not False

    def attach_adapters(self, lora, fp8: bool = False) -> "PrismaticForConditionalGeneration":
        """Run `engine` / `generate` / `predict_action` / `sample_actions` / `score_actions` under `lora` (a
        training.lora.LoraAdapters over THIS model's weights): their engines read `lora.adapted_weights()`, the adapters
        merged into a second set of packed GEMM weights (W' = bf16(W + bf16(s·B)·A), refreshed here and by `lora.refresh()` —
        or after every optimizer step by `TrainStep(..., lora=lora, refresh_adapted=True)`). `use_adapters=False` on those
        calls is the base policy, whose weights are never written. `forward()` (the all-position HF branches) reads the
        base weights.
        `fp8=True` is `lora.enable_fp8()`: the opt-in that lets `model.fp8 = True` (e4m3 prefill) run under the adapters —
        every refresh then requantises the adapted weights' e4m3 copies on the device. It must come before a
        `TrainStep(..., refresh_adapted=True)` over `lora` is built (LoraAdapters.enable_fp8)."""
        if lora.w is not self.weights:
            raise ValueError("attach_adapters: the adapters were built over another model's weights")
        if fp8:
            lora.enable_fp8()                # may raise: before anything attached is dropped
        if self._adapters is not None and self._adapters is not lora:
            self.detach_adapters()
        self._adapters = lora
        if self.weights.embed.is_cuda:       # a CPU-allocated model (layout tests) runs no kernel: its adapted weights stay copies
            lora.refresh()
        return self

    def detach_adapters(self) -> "PrismaticForConditionalGeneration":
        """Back to the base model; the engines built over the adapted weights are dropped."""
        self._adapters = None
        for key in [k for k in self._engines if "adapted" in k]:
            del self._engines[key]
        return self

    def load_adapter(self, adapter_dir, seed: int = 0, fp8: bool = False) -> "PrismaticForConditionalGeneration":
        """Attach the PEFT-named adapter that `training.finetune.save_checkpoint` writes (finetune.py:322-330):
        `adapter_model.safetensors` (base_model.model.<module>.lora_{A,B}.weight) + `adapter_config.json`, from which `r`,
        `lora_alpha` and `lora_dropout` are taken. A module this model has no GEMM group for, or a module of an adapted
        group that the file lacks, is a ValueError. `fp8`: as in `attach_adapters`."""
        import json
        from pathlib import Path
        from safetensors.torch import load_file
        from ...training.lora import LoraAdapters
        d = Path(adapter_dir)
        cfg_path, st_path = d / "adapter_config.json", d / "adapter_model.safetensors"
        if not cfg_path.is_file() or not st_path.is_file():
            raise FileNotFoundError(f"{d}: adapter_config.json and adapter_model.safetensors expected")
        cfg = json.loads(cfg_path.read_text())
        if cfg.get("peft_type", "LORA") != "LORA" or "r" not in cfg:
            raise ValueError(f"{cfg_path}: a PEFT LoRA config with `r` expected")
        r = int(cfg["r"])
        lora = LoraAdapters(self.weights, r=r, alpha=cfg.get("lora_alpha"), seed=seed, dropout=float(cfg.get("lora_dropout", 0.0)))
        sd = load_file(str(st_path))
        known = {f"base_model.model.{mod}.lora_{ab}.weight" for ad in lora.adapters for mod in ad.modules for ab in "AB"}
        unknown = sorted(k for k in sd if k not in known)
        if unknown:
            raise ValueError(f"{st_path}: {len(unknown)} tensors of modules this model has no adapter group for, e.g. {unknown[:3]}")
        missing = sorted(known - set(sd))
        if missing:
            raise ValueError(f"{st_path}: {len(missing)} adapter tensors are missing, e.g. {missing[:3]}")
        lora.load_state_dict(sd)
        return self.attach_adapters(lora, fp8=fp8)

    # ---- the critic at inference: V(s) from the rollout's own prefill (training/value_head.py, csrc/value.hip) ----
    _value_head = None         # the attached training.value_head.ValueHead (the object itself, not a copy)

    def attach_value_head(self, vh) -> "PrismaticForConditionalGeneration":
        """Let `generate` / `predict_action` / `sample_actions` / `score_actions` return the critic's V(s) (`return_values=`):
        `vh` is a training.value_head.ValueHead of dim `dims.llm_dim` on this model's device. The model keeps the object,
        and its engines read `vh.weight` / `vh.bias` in place: a learner that trains this head (TrainStep(value_head=vh)) is
        seen by the next call, with no rebuild. `use_adapters=` on those calls selects the trunk the value is computed over,
        as it does for the policy."""
        if vh.dim != self.dims.llm_dim:
            raise ValueError(f"attach_value_head: the head's dim {vh.dim} is not the model's llm_dim {self.dims.llm_dim}")
        if vh.weight.device != self.weights.embed.device:
            raise ValueError(f"attach_value_head: the head lives on {vh.weight.device}, the model on {self.weights.embed.device}")
        if self._value_head is not None and self._value_head is not vh:
            self.detach_value_head()
        self._value_head = vh
        return self

    def load_value_head(self, directory) -> "PrismaticForConditionalGeneration":
        """Attach the head that `ValueHead.save` wrote into `directory` (`value_head.safetensors`)."""
        from ...training.value_head import ValueHead
        return self.attach_value_head(ValueHead.load(directory, self.weights.embed.device))

    def detach_value_head(self) -> "PrismaticForConditionalGeneration":
        """Drop the head and the engines built over it."""
        self._value_head = None
        for key in [k for k in self._engines if any(isinstance(p, tuple) and p[:1] == ("value",) for p in k)]:
            del self._engines[key]
        return self

    def _value_level(self, return_values: Optional[str]) -> Optional[str]:
        if return_values is None:
            return None
        if return_values not in ("action", "token"):
            raise ValueError(f'return_values must be None, "action" or "token", got {return_values!r}')
        if self._value_head is None:
            raise ValueError("return_values= needs a value head (attach_value_head / load_value_head)")
        return return_values

    # ---- forward: the reference's three branches (modeling_prismatic.py:322-415) ----
    cache_new_tokens = 7       # tokens a `forward(..., use_cache=True)` KV cache is sized for (prefill token + 6 cached steps)

    @torch.no_grad()
    def forward(self, input_ids: Optional[torch.LongTensor] = None, attention_mask: Optional[torch.Tensor] = None,
                pixel_values: Optional[torch.FloatTensor] = None, labels: Optional[torch.LongTensor] = None,
                inputs_embeds: Optional[torch.FloatTensor] = None, past_key_values: Optional[Any] = None,
                use_cache: Optional[bool] = None, output_attentions: Optional[bool] = None,
                output_hidden_states: Optional[bool] = None, output_projector_features: Optional[bool] = None,
                return_dict: Optional[bool] = None) -> Union[Tuple, PrismaticCausalLMOutputWithPast]:
        """The reference's forward (modeling_prismatic.py:291-447), branch for branch:

          * cached generation — `input_ids [B, 1]` + `past_key_values` (:325-341; the batch-1 assert is lifted): one
            decode step on the KV cache the handle names → logits [B, 1, vocab], the same handle one token longer;
          * language-only forward — `pixel_values is None` (:343-359): fp32 logits [B, L, vocab] (+ loss); `inputs_embeds`
            [B, L, D] may replace `input_ids` here (extension; the reference's own `inputs_embeds` plumbing is dead code,
            SURVEY App. C.3);
          * multimodal forward (:362-415): fp32 logits [B, 256+L, vocab] and, with `labels`, the shifted mean
            cross-entropy over the valid tokens (HF CausalLM loss). With `use_cache=True` (and no labels) it is the FIRST
            STEP OF GENERATION: the engine's generation plan runs — bit for bit the launches `generate()` replays — and
            returns the last position's logits [B, 1, vocab] (what GenerationMixin consumes; `logits_to_keep=1` in
            current transformers) plus an opaque `past_key_values` handle bound to that engine's KV caches.

        `output_hidden_states=True` (all-position branches) returns HF's tuple: embeddings, every decoder layer's output,
        the last one after the final norm. `output_attentions` is not served here: the attention kernels never materialise
        the probability matrix (neither does the reference under flash-attn); `attention_maps` computes it on request. No gradients flow through this class."""
        if output_attentions:
            raise NotImplementedError("output_attentions: the fused attention kernels do not materialise attention weights; "
                                      "attention_maps(input_ids, pixel_values, attention_mask, layers) computes them on request")
        if input_ids is None and inputs_embeds is None:
            raise ValueError("Invalid PrismaticForConditionalGeneration `forward()` call: need input_ids (or inputs_embeds)")
        from ...forward_full import EngineKVCache, forward_all_rows, forward_cached_step, forward_prefill_cached
        hidden = proj = loss = None
        cache: Optional[EngineKVCache] = None
        if input_ids is not None and input_ids.shape[1] == 1:
            assert past_key_values is not None, "You must provide `past_key_values` during cached generation!"
            assert labels is None, "Unexpected key `labels` provided during cached generation!"
            logits = forward_cached_step(self, input_ids, past_key_values)
            cache = past_key_values
        elif pixel_values is None:
            assert past_key_values is None, "Unexpected key `past_key_values` provided during language-only forward!"
            loss, logits, _, hidden = forward_all_rows(self, input_ids, attention_mask, None, labels, inputs_embeds,
                                                      bool(output_hidden_states))
        else:
            if input_ids is None or input_ids.shape[0] != pixel_values.shape[0]:
                raise ValueError("Non-homogenous batch of (text, image) input -- forward() does not support mixed batches!")
            assert past_key_values is None, "Unexpected key `past_key_values` provided during language-only forward!"
            if use_cache and labels is None and not output_hidden_states and not output_projector_features:
                logits, cache = forward_prefill_cached(self, input_ids, attention_mask, pixel_values, self.cache_new_tokens)
            else:
                loss, logits, proj, hidden = forward_all_rows(self, input_ids, attention_mask, pixel_values, labels,
                                                             inputs_embeds, bool(output_hidden_states))
        out = PrismaticCausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=cache, hidden_states=hidden,
                                              projector_features=proj if output_projector_features else None)
        if return_dict is False:
            return out.to_tuple()
        return out

    def prepare_inputs_for_generation(self, input_ids: Optional[torch.Tensor] = None, past_key_values: Optional[Any] = None,
                                      inputs_embeds: Optional[torch.FloatTensor] = None,
                                      pixel_values: Optional[torch.FloatTensor] = None,
                                      attention_mask: Optional[torch.Tensor] = None, **kwargs: Any) -> Dict[str, Any]:
        """modeling_prismatic.py:450-485 (GenerationMixin hook): with a cache only the newest token is fed; pixel values,
        mask, cache and `use_cache` ride along. The batch-1 restriction of the reference (:460-463) is lifted, and its
        dead `"input_embeds"` key is spelled `inputs_embeds`."""
        if past_key_values is not None:
            input_ids = input_ids[:, -1:]
        if inputs_embeds is not None and past_key_values is None:
            model_inputs: Dict[str, Any] = {"inputs_embeds": inputs_embeds}
        else:
            model_inputs = {"input_ids": input_ids}
        model_inputs.update({"attention_mask": attention_mask, "pixel_values": None if past_key_values is not None else pixel_values,
                             "past_key_values": past_key_values, "use_cache": kwargs.get("use_cache")})
        return model_inputs

    # nn.Module.__call__ dispatches to forward()

    # ---- generation: greedy, or seeded sampling ----
    @torch.no_grad()
    def generate(self, input_ids: torch.LongTensor, max_new_tokens: int = 7, pixel_values: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, **kwargs: Any):
        """The keywords are those of `_generate`, which is this call before its return is formatted.
        `use_adapters`: see `engine` (None: the attached adapters if any; False: the base model).
        `return_values="action" | "token"` (a value head attached, `attach_value_head`) appends the critic's values, fp32 on
        the device: [B] = V(s) of the state the action is taken in (the row that predicts the first new token, the
        learner's level="action" value row), or [B, max_new_tokens] = the rows that predict every new token
        (level="token"). The returned elements are the fields of `EngineResult` that were asked for, in its order: ids, wt,
        range_wt, values, attention. The value op only reads the residual rows: ids, logits and weights are those of the
        call without it.
        `return_attention="segments" | "full" | "both"` appends an `attention_taps.ActionAttention` to whatever the call
        returns: for every new token, tapped layer (`attention_layers`, None = all) and head, the attention of the query that
        produced it — summed over bos | image | text | generated ("segments"), over every cache row ("full"), or both.
        `text_splits` [B, k] (indices into input_ids, BOS counted) cut the text into k + 1 pieces, e.g. task | description |
        "\nOut:". With `forced_ids` it is the attention under the given tokens. The taps only read: ids, logits and weights
        are those of the call without them.
        Greedy decoding, returns [B, L + max_new_tokens] like GenerationMixin (prompt ‖ new tokens). `use_cache` is
        accepted and ignored: the KV cache is always used (use_cache=False in the fork's demo re-runs the vision towers
        7 times, run_openvla_demo.py:43 — same result, 7× the work). A batch whose attention_mask has zeros is taken as
        RIGHT-padded prompts: pads are hidden from attention and every sequence continues from its own last token.
        `sampling=SamplingParams(temperature, top_k, top_p, seed)` draws the tokens instead (per-sequence settings and
        seeds; bridgelang_amd/sampling.py is the exact specification, and a sequence's tokens depend on its own seed only,
        not on the batch around it); `return_weights=True` then returns (ids, wt [B, max_new_tokens, 2] int64): the drawn
        token's integer weight and the kept total of every step, whose quotient is its probability (`sampling.logprob`).
        `forced_ids` [B, max_new_tokens] turns the call round: nothing is generated, the decode steps are conditioned on
        these tokens and the result is (prompt ‖ forced_ids, wt [B, max_new_tokens, 2]) — every forced token's kept weight
        and the kept total under `sampling` (None: the unwarped distribution, temperature 1), the pair the sampler reports
        when it draws that token (`sampling.score_rows`; weight 0 = outside the support). `score_range=(first, count)`
        appends range_wt int32 [B, max_new_tokens, count]: the kept weights of that token range at every step.
        `vocab_range=(first, count)` restricts the policy to that token range (`sampling.py`, `vocab=`): draws, scores and
        weights are under the softmax of those logits alone, a forced token outside it scores weight 0, and without
        `sampling=` the call is constrained greedy decoding (temperature 0 through the sampling engine).
        `num_beams=W` (2 … 16, at most the policy's token count) with `num_return_sequences=R <= W` (default 1) is beam search
        over the new tokens on the device (bridgelang_amd/beam.py defines it: fixed length, no early finish, so
        `length_penalty` / `early_stopping` cannot change the order and are ignored): ids [B·R, L + max_new_tokens],
        prompt-major and best first, as HF shapes them; `return_weights=True` adds wt [B·R, max_new_tokens, 2], every token's
        weight pair under the unwarped policy given the tokens before it. `vocab_range`, `use_adapters` and
        `return_values="action"` combine with it; `sampling=`, `do_sample`, `forced_ids`, `return_attention` and
        `return_values="token"` raise ValueError. `num_beams=1` is the call without it.
        `share_prefill=True` prefills every prompt once where the call asks several things about it: with `num_beams=W` the W
        beams, with `forced_ids` [B, K, n] the K candidates (rows come back prompt-major, [B·K, …]; `sampling` then holds one
        entry per row; B·K <= 16). Results are those of the replicated call, bit for bit. Padded prompts, `return_attention`,
        `return_values="token"` and `model.fp8` raise ValueError with it; a call with one row per prompt has nothing to share
        and runs as without it."""
        return present(*self._generate(input_ids, max_new_tokens, pixel_values, attention_mask, **kwargs))

    def _generate(self, input_ids: torch.LongTensor, max_new_tokens: int = 7, pixel_values: Optional[torch.Tensor] = None,
                  attention_mask: Optional[torch.Tensor] = None, do_sample: bool = False,
                  sampling: Optional[SamplingParams] = None, return_weights: bool = False,
                  forced_ids: Optional[torch.Tensor] = None, score_range: Optional[Tuple[int, int]] = None,
                  vocab_range: Optional[Tuple[int, int]] = None, use_adapters: Optional[bool] = None,
                  return_attention: Optional[str] = None, attention_layers=None, text_splits=None,
                  return_values: Optional[str] = None, num_beams: int = 1, num_return_sequences: Optional[int] = None,
                  share_prefill: bool = False, group: Optional[int] = None, **_: Any) -> EngineResult:
        """`generate` as a record: its argument checks, one engine run, and the run's `EngineResult` with `ids` = prompt ‖
        new tokens and `wt` only where `generate` returns it. What `predict_action` / `score_actions` read by field.
        Keywords it does not know (`use_cache`, `length_penalty`, `early_stopping`) are accepted and ignored.
        `group=G` (with share_prefill=True; what `sample_actions` passes): G rows per prompt, prompt-major, over one prefill
        of each prompt — `sampling` and a 2-D `forced_ids` then hold one entry per ROW."""
        W, R = self._beam_args(num_beams, num_return_sequences, vocab_range)
        if group is not None and not share_prefill:
            raise ValueError("group= goes with share_prefill=True")
        if forced_ids is not None and torch.as_tensor(forced_ids).dim() == 3:        # [B, K, n]: K candidates per prompt
            if not share_prefill or group is not None:
                raise ValueError("forced_ids [B, K, n] goes with share_prefill=True (it is the group: no group= beside it)")
            forced_ids = torch.as_tensor(forced_ids)
            group, forced_ids = int(forced_ids.shape[1]), forced_ids.reshape(-1, forced_ids.shape[2])
        if share_prefill:       # whatever the group engine rejects is refused here with its reason: no silent fall-back
            for on, why in ((attention_mask is not None and not bool(torch.as_tensor(attention_mask).bool().all()),
                             "padded prompts put every row at its own position; the shared decode kernel has one"),
                            (return_attention is not None, "return_attention: the taps read one cache per row"),
                            (return_values == "token", 'return_values="token" is not built for shared prefills ("action" is)'),
                            (bool(getattr(self, "fp8", False)), "model.fp8: the e4m3 prefill is not the path it is specified against")):
                if on:
                    raise ValueError(f"share_prefill=True: {why}")
        if W > 1:
            for on, why in ((sampling is not None or do_sample, "sampling= / do_sample draw tokens, beam search ranks them"),
                            (forced_ids is not None, "forced_ids scores given tokens, beam search chooses its own"),
                            (return_attention is not None, "return_attention: the taps are not reordered with the beams"),
                            (return_values == "token", 'return_values="token" follows one sequence per row ("action" is available)')):
                if on:
                    raise ValueError(f"num_beams={W}: {why}")
        if do_sample and sampling is None:
            raise NotImplementedError("do_sample=True draws from torch's global device RNG stream, which the HIP path does "
                                      "not reproduce: pass sampling=SamplingParams(temperature=, top_k=, top_p=, seed=) instead")
        if return_weights and sampling is None and W == 1:
            raise ValueError("return_weights goes with sampling= or num_beams=")
        if pixel_values is None:
            raise ValueError("generate() needs pixel_values")
        ids, pv = input_ids.to(self.device), pixel_values.to(self.device)
        taps = self._attn_taps(return_attention, attention_layers)
        if taps is None and text_splits is not None:
            raise ValueError("text_splits goes with return_attention=")
        value = self._value_level(return_values)
        forced = None if forced_ids is None else torch.as_tensor(forced_ids).to(self.device, torch.int64)
        if forced is None and score_range is not None:
            raise ValueError("score_range goes with forced_ids=")
        if W > 1:       # the best R of every prompt's W beams, prompt-major
            r = self._run_beams(ids, pv, max_new_tokens, attention_mask, W, R, vocab_range, use_adapters, value, share_prefill)
            return r._replace(ids=torch.cat([ids.repeat_interleave(R, dim=0), r.ids], dim=1), wt=r.wt if return_weights else None)
        r = self._run_engine(ids, pv, max_new_tokens, attention_mask, sampling, forced, score_range, vocab_range, use_adapters,
                             taps, text_splits, value, group)
        rows = ids if group is None else ids.repeat_interleave(group, dim=0)
        return r._replace(ids=torch.cat([rows, r.ids], dim=1), wt=r.wt if return_weights or forced is not None else None)

    @torch.no_grad()
    def _run_engine(self, ids: torch.Tensor, pv: torch.Tensor, n_new: int, attention_mask: Optional[torch.Tensor],
                    sampling: Optional[SamplingParams], forced: Optional[torch.Tensor], score_range, vocab_range,
                    use_adapters: Optional[bool], taps: Optional[AttnTaps], text_splits, value: Optional[str],
                    group: Optional[int] = None) -> EngineResult:
        """The one path of every generation call through an engine: choose it, fill its settings, forced ids, inputs and
        segments (after the inputs: `set_padded_inputs` resets them), run the plan. Returns copies: nothing handed out
        aliases an engine buffer. The model's engines are not captured, so `replay()` launches the plan eagerly.
        `group=G`: the engine of ids.shape[0] · G rows over one prefill per prompt (`OpenVLAEngine(group=)`)."""
        score = forced is not None
        padded = attention_mask is not None and not bool(attention_mask.bool().all())
        if sampling is None and score:
            sampling = SamplingParams()                              # the unwarped distribution (a score has no seed)
        elif sampling is None and vocab_range is not None:
            sampling = SamplingParams(temperature=0.0, seed=0)       # constrained greedy decoding
        eng = self.engine(ids.shape[0] * (group or 1), ids.shape[1], n_new, padded=padded, sample=sampling is not None and not score,
                          score=score, score_range=score_range, vocab_range=vocab_range, use_adapters=use_adapters, attn_taps=taps,
                          value=value, group=group)
        if sampling is not None:
            eng.set_sampling(sampling)
        if score:
            eng.set_forced_ids(forced)
        if padded:
            eng.set_padded_inputs(ids, pv, attention_mask)
        else:
            eng.set_inputs(ids, pv)
        if taps is not None:                # the segments of THIS call's prompts
            mask = attention_mask if padded else torch.ones(eng.B, eng.L, dtype=torch.int64)
            eng.set_segments(*prompt_segments(mask, eng.n_patches, eng.n_new, text_splits))
        eng.replay()
        return eng.result(torch.clone)

    def _beam_args(self, num_beams, num_return_sequences, vocab_range) -> Tuple[int, int]:
        """(W, R) of `num_beams` / `num_return_sequences`, checked: W an integer in 1 … MAX_BEAMS and at most the number of
        tokens the policy chooses from, 1 <= R <= W (None: 1)."""
        n_tokens = self.dims.vocab if vocab_range is None else int(vocab_range[1])
        if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)) or not 1 <= num_beams <= min(MAX_BEAMS, n_tokens):
            raise ValueError(f"num_beams must be an integer in 1 … {min(MAX_BEAMS, n_tokens)} (at most {MAX_BEAMS} beams, and no "
                             f"more than the {n_tokens} tokens of the policy), got {num_beams!r}")
        R = 1 if num_return_sequences is None else num_return_sequences
        if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= num_beams:
            raise ValueError(f"num_return_sequences must be an integer in 1 … num_beams = {num_beams}, got {num_return_sequences!r}")
        return int(num_beams), int(R)

    @torch.no_grad()
    def _run_beams(self, ids: torch.Tensor, pv: torch.Tensor, n_new: int, attention_mask: Optional[torch.Tensor], W: int, R: int,
                   vocab_range, use_adapters: Optional[bool], value: Optional[str], share_prefill: bool = False) -> EngineResult:
        """Beam search of W beams for every prompt, the best R of each returned prompt-major: ids [B·R, n_new], wt
        [B·R, n_new, 2], values [B·R] (V(s) is the prompt's: the same for its R rows). The prompts are split over engine
        runs of max(1, 16 // W) prompts — a prompt's beams are never split, and every run stays within the 16 rows where a
        sequence's result is its batch-1 result — so a prompt's beams do not depend on the prompts around it.
        `share_prefill=True`: the same runs on the group=W engine — every prompt is prefilled once, not W times."""
        B = ids.shape[0]
        padded = attention_mask is not None and not bool(attention_mask.bool().all())
        per_run, parts = max(1, 16 // W), []
        for e0 in range(0, B, per_run):
            c = min(per_run, B - e0)
            eng = self.engine(c * W, ids.shape[1], n_new, padded=padded, vocab_range=vocab_range, use_adapters=use_adapters,
                              value=value, beams=W, group=W if share_prefill else None)
            if padded:
                eng.set_padded_inputs(ids[e0:e0 + c], pv[e0:e0 + c], attention_mask[e0:e0 + c])
            else:
                eng.set_inputs(ids[e0:e0 + c], pv[e0:e0 + c])
            eng.replay()
            r = eng.result(torch.clone)
            if share_prefill and r.values is not None:      # one V(s) per prompt → per row, as the replicated engine hands it out
                r = r._replace(values=r.values.repeat_interleave(W))
            parts.append(r)
        best = lambda x: x.reshape((-1, W) + tuple(x.shape[1:]))[:, :R].reshape((-1,) + tuple(x.shape[1:]))
        return EngineResult(ids=torch.cat([best(p.ids) for p in parts]), wt=torch.cat([best(p.wt) for p in parts]),
                            values=None if value is None else torch.cat([best(p.values) for p in parts]))


def _numpy(t: Optional[torch.Tensor]) -> Optional[np.ndarray]:
    return None if t is None else t.cpu().numpy()


# ---- copies / candidates of a batch, several per engine run (`sample_actions`, `score_actions`) ----
def copy_runs(B: int, K: int) -> List[Tuple[int, int]]:
    """(first copy j0, copies c) of the engine runs that cover K copies of a batch of B: max(1, 16 // B) per run — batches up
    to 16 keep "a sequence's result is its batch-1 result"."""
    per_run = max(1, 16 // B)
    return [(j0, min(per_run, K - j0)) for j0 in range(0, K, per_run)]


def group_runs(B: int, K: int) -> List[Tuple[int, int, int, int]]:
    """(first prompt b0, prompts nb, first copy j0, copies c) of the engine runs that cover K copies of B prompts with ONE
    prefill per prompt and run (`share_prefill=True`): rows are prompt-major, row (b - b0)·c + (j - j0). K <= 16: a prompt's K
    rows are never split, max(1, 16 // K) prompts per run. K > 16: the copies are cut into chunks of at most 16, each run of
    them with its own prefill. No run exceeds 16 rows: "a sequence's result is its batch-1 result" holds in every one."""
    runs = []
    for j0 in range(0, K, 16):
        c = min(16, K - j0)
        per_run = max(1, 16 // c)
        runs += [(b0, min(per_run, B - b0), j0, c) for b0 in range(0, B, per_run)]
    return runs


def group_sampling(T, k, p, seed, b0: int, nb: int, j0: int, c: int) -> SamplingParams:
    """The resolved per-sequence settings [B] for prompts b0 … b0 + nb - 1 and copies j0 … j0 + c - 1, prompt-major [nb·c]:
    copy j draws with `derive_seed(seed, j)` whatever the chunking; seed=None (a score has none): 0."""
    rows = slice(b0, b0 + nb)
    return SamplingParams(temperature=np.repeat(T[rows], c), top_k=np.repeat(k[rows], c), top_p=np.repeat(p[rows], c),
                          seed=0 if seed is None else np.stack([derive_seed(seed[rows], j) for j in range(j0, j0 + c)], axis=1).reshape(-1))


def stack_groups(parts: Sequence, runs: Sequence[Tuple[int, int, int, int]], B: int, K: int):
    """Per-run arrays [nb·c, …] (prompt-major, `group_runs`; None: absent) → [B, K, …]."""
    if parts[0] is None:
        return None
    out = np.empty((B, K) + tuple(parts[0].shape[1:]), dtype=parts[0].dtype)
    for x, (b0, nb, j0, c) in zip(parts, runs):
        out[b0:b0 + nb, j0:j0 + c] = np.asarray(x).reshape((nb, c) + tuple(x.shape[1:]))
    return out


def tile_sampling(T, k, p, seed, j0: int, c: int) -> SamplingParams:
    """The resolved per-sequence settings [B] for copies j0 … j0 + c - 1, copy-major [c·B]: copy j draws with
    `derive_seed(seed, j)`; seed=None (a score has none): 0."""
    return SamplingParams(temperature=np.tile(T, c), top_k=np.tile(k, c), top_p=np.tile(p, c),
                          seed=0 if seed is None else np.concatenate([derive_seed(seed, j) for j in range(j0, j0 + c)]))


def tap_kwargs(return_attention, attention_layers, text_splits, B: int, c: int) -> dict:
    """The attention keywords of a run over c copies (`text_splits` [B, k] tiled copy-major); none without `return_attention`."""
    if return_attention is None:
        return {}
    return dict(return_attention=return_attention, attention_layers=attention_layers,
                text_splits=None if text_splits is None else torch.as_tensor(text_splits).reshape(B, -1).repeat(c, 1))


def stack_runs(parts: Sequence, B: int):
    """Per-run results [c·B, …] (copy-major; arrays or tensors, None: absent) → [B, copies, …]."""
    if parts[0] is None:
        return None
    split = [x.reshape((x.shape[0] // B, B) + tuple(x.shape[1:])) for x in parts]
    if isinstance(split[0], np.ndarray):
        return np.concatenate(split, axis=0).swapaxes(0, 1)
    return torch.cat(split, dim=0).transpose(0, 1).contiguous()


def stack_values(parts: Sequence, B: int, level: Optional[str]):
    """The critic's values of the runs: every copy of a sequence is in the same state, so level "action" is copy 0's [B];
    level "token" is every copy's [B, copies, n]."""
    if parts[0] is None:
        return None
    return parts[0][:B].copy() if level == "action" else stack_runs(parts, B)


def stack_attention(parts: Sequence[Optional[ActionAttention]], B: int) -> Optional[ActionAttention]:
    """The ActionAttention of the runs → one with tensors [B, copies, n_new, layers, H, ·]."""
    if parts[0] is None:
        return None
    return ActionAttention(probs=stack_runs([a.probs for a in parts], B), segments=stack_runs([a.segments for a in parts], B),
                           names=parts[0].names, layers=parts[0].layers)


class OpenVLAForActionPrediction(PrismaticForConditionalGeneration):
    config_class = OpenVLAConfig

    def __init__(self, config: OpenVLAConfig, device: Union[str, torch.device, None] = None,
                 dims: Optional[VLADims] = None) -> None:
        super().__init__(config, device, dims)
        self.norm_stats = config.norm_stats
        self.bins = np.linspace(-1, 1, config.n_action_bins)
        self.bin_centers = (self.bins[:-1] + self.bins[1:]) / 2.0
        # de-tokenisation vocabulary: the padded "multiple of 64" rows are not action tokens (reference :503-504)
        self.vocab_size = self.dims.vocab - config.pad_to_multiple_of

    def action_token_range(self) -> Tuple[int, int]:
        """(first, count) of the token ids that carry an action bin: vocab_size - n_action_bins … vocab_size - 1. The range
        of the restricted policy (`action_tokens_only=True`; `PolicyLossConfig.token_range`, `rl.policy_batch`)."""
        n_bins = int(self.config.n_action_bins)
        return int(self.vocab_size) - n_bins, n_bins

    def predict_action(self, input_ids: Optional[torch.LongTensor] = None, unnorm_key: Union[str, Sequence[Optional[str]], None] = None,
                       action_tokens_only: bool = False, use_adapters: Optional[bool] = None, **kwargs: Any) -> np.ndarray:
        """`use_adapters`: see `engine` (None: under the attached adapters if any; False: the base policy).
        ids → 7 greedy action tokens → bin centres → un-normalised 7-DoF action (reference :506-536). `unnorm_key` may
        be a list with one key per sequence (extension: a server batch that mixes datasets of one action dimension);
        the result is then always [B, n]. `action_tokens_only=True` decodes under the policy restricted to
        `action_token_range()`: with `sampling=` every draw is an action token, without it the call is constrained greedy
        decoding (the argmax over the action tokens). `return_attention=` / `attention_layers=` / `text_splits=` (see
        `generate`) return the `ActionAttention` of the action tokens as an extra last element; `text_splits` index the
        input_ids as given (the empty token this call appends joins the last text piece).
        `return_values="action" | "token"` (see `generate`, `attach_value_head`) returns the critic's values as one more
        element, fp32 ndarray [B] or [B, n]. Order: the action, then (tokens, wt) with `return_weights`, then the values, then
        the `ActionAttention`.
        `num_beams=W` (see `generate`) returns the action of the best of W beams — the most likely whole action beam search
        finds, where the greedy chain is only the most likely token at a time — shaped as today; `num_return_sequences=R > 1`
        returns the best R, [B, R, n] (`beam_actions` adds their tokens and log-probabilities)."""
        p = self._predict(input_ids, unnorm_key, action_tokens_only, use_adapters, **kwargs)
        return present(p.actions, None if p.wt is None else p.tokens, p.wt, p.values, p.attention)

    def _predict(self, input_ids: torch.LongTensor, unnorm_key, action_tokens_only: bool = False,
                 use_adapters: Optional[bool] = None, **kwargs: Any) -> SimpleNamespace:
        """`predict_action` as named parts: actions, tokens, wt, values (numpy) and attention; None: not asked for."""
        input_ids = input_ids.to(self.device)
        keys = list(unnorm_key) if isinstance(unnorm_key, (list, tuple)) else None
        if keys is not None:
            if len(keys) != input_ids.shape[0] or len({self.get_action_dim(k) for k in keys}) != 1:
                raise ValueError("predict_action: a list of unnorm_keys needs one key per sequence, all of one action dimension")
            unnorm_key = keys[0]
        input_ids, m = self._action_prompt(input_ids, kwargs.get("attention_mask"))
        if m is not None:
            kwargs["attention_mask"] = m
        n = self.get_action_dim(unnorm_key)
        if action_tokens_only:
            kwargs["vocab_range"] = self.action_token_range()
        r = self._generate(input_ids, max_new_tokens=n, use_adapters=use_adapters, **kwargs)
        tokens = r.ids[:, -n:].cpu().numpy()
        B, R = input_ids.shape[0], tokens.shape[0] // input_ids.shape[0]     # R > 1: num_return_sequences rows per prompt
        if keys is not None:
            actions = np.stack([np.asarray(self.actions_from_token_ids(tokens[i:i + 1], k)).reshape(-1) for i, k in enumerate(k for k in keys for _ in range(R))])
        else:
            actions = self.actions_from_token_ids(tokens, unnorm_key)
        wt, values = _numpy(r.wt), _numpy(r.values)
        if R > 1:       # [B, R, …], best first; V(s) is the prompt's
            actions, tokens = np.asarray(actions).reshape(B, R, n), tokens.reshape(B, R, n)
            if values is not None and kwargs.get("group") is None:      # a group engine's values are the prompts' already
                values = values[::R].copy()
            wt = None if wt is None else wt.reshape(B, R, n, 2)
        return SimpleNamespace(actions=actions, tokens=tokens, wt=wt, values=values, attention=r.attention)

    def _action_prompt(self, input_ids: torch.LongTensor, m: Optional[torch.Tensor]):
        """The prompt with the empty token 29871 behind each sequence's last token → (input_ids, attention_mask)."""
        if m is not None and not bool(m.bool().all()):
            # right-padded batch: the empty token goes behind each sequence's last REAL token (one more column)
            m = m.to(self.device).long()
            n = m.sum(dim=1)
            rows = torch.arange(input_ids.shape[0], device=self.device)
            need = input_ids[rows, n - 1] != 29871
            ids = torch.cat((input_ids, torch.full_like(input_ids[:, :1], self.pad_token_id)), dim=1)
            m = torch.cat((m, torch.zeros_like(m[:, :1])), dim=1)
            ids[rows[need], n[need]] = 29871
            m[rows[need], n[need]] = 1
            return ids, m
        input_ids = self.with_empty_token(input_ids)
        if m is not None and m.shape[1] != input_ids.shape[1]:
            m = m.to(self.device)
            m = torch.cat((m, torch.ones_like(m[:, :1])), dim=1)
        return input_ids, m

    def sample_actions(self, input_ids: torch.LongTensor, pixel_values: torch.Tensor,
                       unnorm_key: Union[str, Sequence[Optional[str]], None] = None, sampling: Optional[SamplingParams] = None,
                       num_samples: int = 1, attention_mask: Optional[torch.Tensor] = None,
                       action_tokens_only: bool = False,
                       use_adapters: Optional[bool] = None, return_attention: Optional[str] = None, attention_layers=None,
                       text_splits=None, return_values: Optional[str] = None,
                       share_prefill: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`share_prefill=True` prefills every prompt once per engine run instead of once per copy (`OpenVLAEngine(group=)`,
        runs by `group_runs`): the same arrays, bit for bit, for less work. Padded prompts, `return_attention`,
        `return_values="token"` and `model.fp8` raise ValueError with it: nothing falls back silently.
        `use_adapters`: see `engine` (None: under the attached adapters if any; False: the base policy).
        `return_values="action"` appends V(s) fp32 [B] — every copy of a sequence is in the same state, so one value per
        sequence, taken from copy 0; `"token"` appends [B, num_samples, n], the values along every copy's own tokens. Order:
        actions, tokens, logprobs, values, attention.
        `num_samples` sampled actions per sequence with their log-probabilities (RL rollouts, best-of-N, uncertainty):
        → (actions [B, num_samples, n], token_ids int64 [B, num_samples, n], logprobs fp64 [B, num_samples, n]). The batch
        is repeated `num_samples` times (several copies per engine run while the run stays within 16 sequences); copy j of a sequence with seed s draws with
        seed s + 0x9E3779B97F4A7C15·j mod 2^64 (`sampling.derive_seed`), so copy j equals that one call. logprobs[b, j, t] =
        log(w / total) of step t's weight pair: the token's log-probability under the warped (temperature / top-k /
        top-p) distribution. `action_tokens_only=True` draws from the policy restricted to `action_token_range()`: every
        token is an action token and its log-probability is the one under that restricted policy — what a learner with
        `PolicyLossConfig(token_range=model.action_token_range())` trains against.
        `return_attention=` (with `attention_layers=`, `text_splits=` [B, k]; see `generate`) appends the `ActionAttention` of
        every copy: tensors [B, num_samples, n, layers, H, ·]."""
        if sampling is None:
            sampling = SamplingParams()
        if num_samples < 1:
            raise ValueError("num_samples must be >= 1")
        B = input_ids.shape[0]
        T, k, p, seed = sampling.resolve(B)
        keys = list(unnorm_key) if isinstance(unnorm_key, (list, tuple)) else None
        level = self._value_level(return_values)
        if share_prefill:
            groups = group_runs(B, num_samples)
            runs = [self._predict(input_ids[b0:b0 + nb], keys[b0:b0 + nb] if keys is not None else unnorm_key, action_tokens_only,
                                  use_adapters, pixel_values=pixel_values[b0:b0 + nb],
                                  attention_mask=None if attention_mask is None else attention_mask[b0:b0 + nb],
                                  sampling=group_sampling(T, k, p, seed, b0, nb, j0, c), return_weights=True, return_values=level,
                                  return_attention=return_attention, share_prefill=True, group=c)
                    for b0, nb, j0, c in groups]
            flat = lambda x: np.asarray(x).reshape((-1,) + tuple(np.shape(x)[-1:]))
            first = [i for i, g in enumerate(groups) if g[2] == 0]       # V(s) is the prompt's: the runs of copy 0 cover every prompt
            return present(stack_groups([flat(r.actions) for r in runs], groups, B, num_samples),
                           stack_groups([flat(r.tokens) for r in runs], groups, B, num_samples),
                           stack_groups([logprob(r.wt).reshape(flat(r.tokens).shape) for r in runs], groups, B, num_samples),
                           None if level is None else np.concatenate([runs[i].values for i in first]))
        runs = [self._predict(input_ids.repeat(c, 1), keys * c if keys is not None else unnorm_key, action_tokens_only, use_adapters,
                              pixel_values=pixel_values.repeat(c, 1, 1, 1),
                              attention_mask=None if attention_mask is None else attention_mask.repeat(c, 1),
                              sampling=tile_sampling(T, k, p, seed, j0, c), return_weights=True, return_values=level,
                              **tap_kwargs(return_attention, attention_layers, text_splits, B, c))
                for j0, c in copy_runs(B, num_samples)]
        return present(stack_runs([np.asarray(r.actions).reshape(r.tokens.shape[0], -1) for r in runs], B),
                       stack_runs([r.tokens for r in runs], B), stack_runs([logprob(r.wt) for r in runs], B),
                       stack_values([r.values for r in runs], B, level), stack_attention([r.attention for r in runs], B))

    def beam_actions(self, input_ids: torch.LongTensor, pixel_values: torch.Tensor,
                     unnorm_key: Union[str, Sequence[Optional[str]], None] = None, num_beams: int = 4,
                     num_return_sequences: Optional[int] = None, attention_mask: Optional[torch.Tensor] = None,
                     action_tokens_only: bool = False, use_adapters: Optional[bool] = None,
                     return_values: Optional[str] = None, share_prefill: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`share_prefill=True`: every prompt is prefilled once, not once per beam (see `sample_actions`); same arrays.
        The `num_return_sequences` (None: all `num_beams`) most likely whole actions that beam search of `num_beams` beams
        finds for every prompt, best first, in the shapes of `sample_actions`: → (actions [B, R, n], token_ids int64
        [B, R, n], logprobs fp64 [B, R, n]). logprobs = `sampling.logprob` of the per-token weight pairs: every token's
        log-probability under the unwarped policy given the tokens before it (their sum is the action's joint
        log-probability), bit for bit what `score_actions(token_ids=those tokens)` returns. bridgelang_amd/beam.py defines the
        search: fixed length n, no early finish, HF's `num_beams=W, do_sample=False` search when `action_tokens_only=True`
        keeps EOS out of it. `return_values="action"` appends V(s) fp32 [B]; `use_adapters`: see `engine`. One beam is the
        greedy action with its log-probabilities."""
        if return_values == "token":
            raise ValueError('beam_actions: return_values="token" follows one sequence per row ("action" is available)')
        vocab_range = self.action_token_range() if action_tokens_only else None
        W, R = self._beam_args(num_beams, num_beams if num_return_sequences is None else num_return_sequences, vocab_range)
        level = self._value_level(return_values)
        keys = list(unnorm_key) if isinstance(unnorm_key, (list, tuple)) else None
        B = input_ids.shape[0]
        if keys is not None and (len(keys) != B or len({self.get_action_dim(k) for k in keys}) != 1):
            raise ValueError("beam_actions: a list of unnorm_keys needs one key per sequence, all of one action dimension")
        n = self.get_action_dim(keys[0] if keys is not None else unnorm_key)
        ids, m = self._action_prompt(input_ids.to(self.device), attention_mask)
        if share_prefill:
            if m is not None and not bool(m.bool().all()):
                raise ValueError("share_prefill=True: padded prompts put every row at its own position; the shared decode kernel has one")
            if bool(getattr(self, "fp8", False)):
                raise ValueError("share_prefill=True: model.fp8: the e4m3 prefill is not the path it is specified against")
        r = self._run_beams(ids, pixel_values.to(self.device), n, m, W, R, vocab_range, use_adapters, level, share_prefill)
        tokens = r.ids.cpu().numpy()
        row_keys = [unnorm_key] * (B * R) if keys is None else [k for k in keys for _ in range(R)]
        actions = np.stack([np.asarray(self.actions_from_token_ids(tokens[i:i + 1], k)).reshape(-1) for i, k in enumerate(row_keys)])
        return present(actions.reshape(B, R, n), tokens.reshape(B, R, n), logprob(_numpy(r.wt)).reshape(B, R, n),
                       None if level is None else _numpy(r.values)[::R].copy())

    def score_actions(self, input_ids: torch.LongTensor, pixel_values: torch.Tensor, token_ids=None, actions=None,
                      unnorm_key: Optional[str] = None, sampling: Optional[SamplingParams] = None,
                      attention_mask: Optional[torch.Tensor] = None, return_bins: bool = False,
                      action_tokens_only: bool = False, use_adapters: Optional[bool] = None,
                      return_attention: Optional[str] = None, attention_layers=None, text_splits=None,
                      return_values: Optional[str] = None, share_prefill: bool = False):
        """`share_prefill=True`: every prompt is prefilled once per engine run, not once per candidate (see `sample_actions`);
        the same arrays, bit for bit.
        `return_values="action"` appends V(s) fp32 [B] (the state is the same for every candidate: candidate 0's);
        `"token"` appends [B, K, n], the values along the given tokens. `return_attention=` (with `attention_layers=`,
        `text_splits=` [B, k]; see `generate`) appends the `ActionAttention` under the GIVEN actions, tensors [B, K, n, layers,
        H, ·]. Order: logprobs, then (wt, bin_wt) with `return_bins`, then the values, then the `ActionAttention`.
        `use_adapters`: see `engine` (None: under the attached adapters if any; False: the base policy — with adapters
        attached, an RL learner's reference policy).
        Log-probabilities of GIVEN actions under the policy `sample_actions` draws from (a PPO / GRPO learner's
        log π(a | s), a reranker's score of a planner's proposal): exactly one of `token_ids` (int64) and `actions`
        (tokenised by `token_ids_from_actions` with `unnorm_key`), shaped [B, n] or [B, K, n] with K candidates per
        sequence → logprobs fp64 [B, K, n] (K = 1 for [B, n]), -inf where a token lies outside the support that
        `sampling` (temperature / top-k / top-p per sequence; no seed) leaves. For tokens `sample_actions` drew under the
        same settings the values equal its logprobs bit for bit: the decode steps run the cached plan conditioned on the
        given tokens, so every step sees the logits the sampler saw. Candidates are batched like `sample_actions`' copies
        (16 // B per engine run). `return_bins=True` → (logprobs, wt int64 [B, K, n, 2], bin_wt int32 [B, K, n,
        n_action_bins]): the integer weight pairs and the kept weight of every action token, bin_wt[..., j] for token
        vocab_size - n_action_bins + j, so bin_wt / wt[..., 1:] are exact per-bin probabilities (`sampling.range_entropy`).
        `action_tokens_only=True` scores under the policy restricted to `action_token_range()`, as `sample_actions` draws
        with the same flag: a token outside the range scores -inf, and the bin weights then sum to the kept total exactly."""
        if (token_ids is None) == (actions is None):
            raise ValueError("score_actions: give exactly one of token_ids= and actions=")
        if token_ids is None:
            token_ids = self.token_ids_from_actions(actions, unnorm_key)
        tok = np.asarray(token_ids.detach().cpu().numpy() if hasattr(token_ids, "detach") else token_ids)
        B = input_ids.shape[0]
        if tok.ndim == 2:
            tok = tok[:, None, :]
        if tok.ndim != 3 or tok.shape[0] != B or tok.shape[1] < 1 or not np.issubdtype(tok.dtype, np.integer):
            raise ValueError(f"score_actions: integer token ids [B, n] or [B, K, n] with B = {B}, got {tok.dtype} {tok.shape}")
        tok = tok.astype(np.int64)
        K, n = tok.shape[1:]
        if tok.min() < 0 or tok.max() >= self.dims.vocab:
            raise ValueError(f"score_actions: token ids must lie in [0, {self.dims.vocab})")
        if sampling is None:
            sampling = SamplingParams()
        T, k, p, _ = replace(sampling, seed=0).resolve(B)
        n_bins = self.config.n_action_bins
        rng = (self.vocab_size - n_bins, n_bins) if return_bins else None
        ids, m = self._action_prompt(input_ids.to(self.device), attention_mask)      # the prompt as predict_action prepares it
        level = self._value_level(return_values)
        if share_prefill:
            groups = group_runs(B, K)
            runs = [self._generate(ids[b0:b0 + nb], n, pixel_values=pixel_values[b0:b0 + nb],
                                   attention_mask=None if m is None else m[b0:b0 + nb],
                                   sampling=group_sampling(T, k, p, None, b0, nb, j0, c),
                                   forced_ids=torch.from_numpy(np.ascontiguousarray(tok[b0:b0 + nb, j0:j0 + c])), score_range=rng,
                                   vocab_range=self.action_token_range() if action_tokens_only else None, use_adapters=use_adapters,
                                   return_values=level, return_attention=return_attention, share_prefill=True)
                    for b0, nb, j0, c in groups]
            wt = stack_groups([_numpy(r.wt) for r in runs], groups, B, K)
            first = [i for i, g in enumerate(groups) if g[2] == 0]
            return present(logprob(wt), wt if return_bins else None, stack_groups([_numpy(r.range_wt) for r in runs], groups, B, K),
                           None if level is None else np.concatenate([_numpy(runs[i].values) for i in first]))
        runs = []
        for j0, c in copy_runs(B, K):
            forced = torch.from_numpy(np.ascontiguousarray(tok[:, j0:j0 + c].transpose(1, 0, 2)).reshape(c * B, n))
            runs.append(self._generate(ids.repeat(c, 1), n, pixel_values=pixel_values.repeat(c, 1, 1, 1),
                                       attention_mask=None if m is None else m.repeat(c, 1), sampling=tile_sampling(T, k, p, None, j0, c),
                                       forced_ids=forced, score_range=rng,
                                       vocab_range=self.action_token_range() if action_tokens_only else None,
                                       use_adapters=use_adapters, return_values=level,
                                       **tap_kwargs(return_attention, attention_layers, text_splits, B, c)))
        wt = stack_runs([_numpy(r.wt) for r in runs], B)
        return present(logprob(wt), wt if return_bins else None, stack_runs([_numpy(r.range_wt) for r in runs], B),
                       stack_values([_numpy(r.values) for r in runs], B, level), stack_attention([r.attention for r in runs], B))

    def token_ids_from_actions(self, actions: np.ndarray, unnorm_key: Optional[str] = None) -> np.ndarray:
        """Un-normalised actions [..., n] → action token ids int64 [..., n]: the inverse of `actions_from_token_ids`, i.e.
        what the training pipeline makes of a demonstrated action. The dataset's BOUNDS_Q99 normalisation first
        (rlds/utils/data_utils.py:76-93): dimensions the statistics' `mask` selects go linearly from [q01, q99] to [-1, 1]
        — 2·(a - q01) / (q99 - q01 + 1e-8) - 1 — and are clipped to it, the others (the gripper) pass through. Then the
        action tokenizer (action_tokenizer.py:38-47): clip to [-1, 1], `np.digitize` against the bin edges, and
        token = vocab_size - bin. An action beyond q01 / q99 therefore lands in an end bin."""
        stats = self.get_action_stats(unnorm_key)
        a = np.asarray(actions, dtype=np.float64)
        lo, hi = np.asarray(stats["q01"], dtype=np.float64), np.asarray(stats["q99"], dtype=np.float64)
        mask = np.asarray(stats.get("mask", np.ones_like(lo, dtype=bool)), dtype=bool)
        if a.shape[-1] != lo.shape[0]:
            raise ValueError(f"token_ids_from_actions: actions of dimension {lo.shape[0]} expected, got shape {a.shape}")
        normalized = np.where(mask, np.clip(2.0 * (a - lo) / (hi - lo + 1e-8) - 1.0, -1.0, 1.0), a)
        bins = np.digitize(np.clip(normalized, float(self.bins[0]), float(self.bins[-1])), self.bins)
        return (self.vocab_size - bins).astype(np.int64)

    def with_empty_token(self, input_ids: torch.LongTensor) -> torch.LongTensor:
        """Append the special empty token 29871 the Llama tokenizer would have put after "Out:" (reference :510-515)."""
        if torch.all(input_ids[:, -1] == 29871):
            return input_ids
        tail = torch.full((input_ids.shape[0], 1), 29871, dtype=torch.long, device=input_ids.device)
        return torch.cat((input_ids, tail), dim=1)

    def actions_from_token_ids(self, token_ids: np.ndarray, unnorm_key: Optional[str] = None) -> np.ndarray:
        """Generated action token ids [B, n] → un-normalised actions (reference :520-536)."""
        discretized = np.clip(self.vocab_size - token_ids - 1, a_min=0, a_max=self.bin_centers.shape[0] - 1)
        normalized = self.bin_centers[discretized]
        stats = self.get_action_stats(unnorm_key)
        mask = stats.get("mask", np.ones_like(stats["q01"], dtype=bool))
        hi, lo = np.array(stats["q99"]), np.array(stats["q01"])
        actions = np.where(mask, 0.5 * (normalized + 1) * (hi - lo) + lo, normalized)
        return actions[0] if actions.shape[0] == 1 else actions

    @staticmethod
    def _check_unnorm_key(norm_stats: Dict[str, Dict[str, Any]], unnorm_key: Optional[str]) -> str:
        if unnorm_key is None:
            assert len(norm_stats) == 1, (
                f"Your model was trained on more than one dataset, please pass a `unnorm_key` from the following "
                f"options to choose the statistics used for un-normalizing actions: {norm_stats.keys()}")
            unnorm_key = next(iter(norm_stats.keys()))
        assert unnorm_key in norm_stats, (
            f"The `unnorm_key` you chose is not in the set of available dataset statistics, please choose from: "
            f"{norm_stats.keys()}")
        return unnorm_key

    def get_action_dim(self, unnorm_key: Optional[str] = None) -> int:
        return len(self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]["q01"])

    def get_action_stats(self, unnorm_key: Optional[str] = None) -> Dict[str, Any]:
        return self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]


def register_auto_classes() -> None:
    """What finetune.py:151-154 / deploy.py:66-69 do before `from_pretrained`: make `model_type == "openvla"` resolve to
    these classes through the HF Auto classes. transformers < 5 has `AutoModelForVision2Seq`; >= 5 renamed it to
    `AutoModelForImageTextToText` — whichever exist are registered. Idempotent."""
    import transformers
    from transformers import AutoConfig
    for model_type, cfg in (("prismatic", PrismaticConfig), ("openvla", OpenVLAConfig)):
        try:
            AutoConfig.register(model_type, cfg)
        except ValueError:
            pass                                     # already registered
    for name in ("AutoModelForVision2Seq", "AutoModelForImageTextToText"):
        auto = getattr(transformers, name, None)
        if auto is None:
            continue
        for cfg, cls in ((PrismaticConfig, PrismaticForConditionalGeneration), (OpenVLAConfig, OpenVLAForActionPrediction)):
            try:
                auto.register(cfg, cls)
            except ValueError:
                pass
