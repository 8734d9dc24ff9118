"""Which tensors train, and where their optimizer state lives: the stage table of `PrismaticVLM.freeze_backbones`
(prismatic/models/vlms/prismatic.py:129-241), the optimizer grouping of `FSDPStrategy.run_setup`
(prismatic/training/strategies/fsdp.py:195-236) and the flat parameter space behind `TrainStep` (DESIGN.md "Training
step"). Host-side bookkeeping over torch tensors: no kernels, nothing of the inference engine, usable on the CPU."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..weights import PackedGroup, VLAWeights, _block_view, _unpack
from .sharding import ShardComm, ShardLayout, bucket_key

# stage → (vision trainable, projector trainable, llm: "all" | "last" | "none")   — prismatic.py:129-241
STAGES: Dict[str, Tuple[bool, bool, str]] = {
    "align": (False, True, "none"),
    "finetune": (False, True, "all"), "vla-train": (False, True, "all"),
    "full-finetune": (True, True, "all"), "vla-full-train": (True, True, "all"),
    "last-layer-finetune": (False, False, "last"), "vla-last-layer-train": (False, False, "last"),
    "vla-sandwich-train": (True, True, "last"),
    "lora": (False, False, "none"),          # vla-scripts/finetune.py: base frozen, adapters train (training/lora.py)
}


def trainable_names(w: VLAWeights, stage: str) -> List[str]:
    """HF tensor names with requires_grad=True after `freeze_backbones(stage)`; "last" = embed_tokens, the final decoder
    layer and lm_head (llama2.py:101-102; the final norm is not in that tuple and stays frozen)."""
    if stage not in STAGES:
        raise ValueError(f"Stage `{stage}` is not supported")
    vision, proj, llm = STAGES[stage]
    last = f"language_model.model.layers.{w.dims.llm_layers - 1}."
    out = []
    for name in w.placements:
        if name.startswith("vision_backbone."):
            ok = vision
        elif name.startswith("projector."):
            ok = proj
        elif llm == "all":
            ok = True
        elif llm == "last":
            ok = name.startswith(last) or name in ("language_model.model.embed_tokens.weight", "language_model.lm_head.weight")
        else:
            ok = False
        if ok:
            out.append(name)
    return out


# buckets whose PARAMETERS are sharded under fsdp-full-shard: every FSDP unit of the reference — decoder layers, ViT blocks
# (+ patch embeddings), projector, and the root's token embeddings / lm_head (prismatic.py:285-306, dinosiglip_vit.py:136-140,
# base_llm.py:182-188, fsdp.py:160-168). Not sharded: the two buckets of small plain tensors.
def param_sharded_key(key: str) -> bool:
    return key.startswith(("llm.layer", "vision.", "projector", "llm.lm_head", "llm.embed"))


def pool_of(key: str) -> str:
    """Gather-slot pool of a parameter-sharded bucket: uniform decoder layers / the vision units / the three big singletons."""
    return "layers" if key.startswith("llm.layer") else "vision" if key.startswith("vision.") else "head"


def no_decay(name: str, shape: Tuple[int, ...]) -> bool:
    """fsdp.py:208: `param.ndim <= 1 or name.endswith(".bias")` → weight_decay 0."""
    return len(shape) <= 1 or name.endswith(".bias")


@dataclass
class Unit:
    """One optimizer unit: a packed GEMM weight group (logical [n, k] matrix) or a plain tensor."""
    key: str
    offset: int                 # into the flat (bucket-padded) parameter space
    numel: int
    group: Optional[PackedGroup]
    dst: Optional[torch.Tensor]        # plain: contiguous bf16 view of the live parameter
    decay: bool
    bucket: int
    names: Tuple[str, ...] = ()


class ParamStore:
    """Trainable tensors as one flat parameter space (sharding.ShardLayout): full fp32 gradients and a full bf16 staging
    copy on every rank, fp32 masters and AdamW moments for this rank's 1/world slice of every bucket only."""

    def __init__(self, w: VLAWeights, stage: str, world: int = 1, rank: int = 0,
                 extra: Optional[List[Tuple[str, torch.Tensor, bool, str]]] = None, only: Optional[Sequence[str]] = None,
                 shard_params: bool = False, defer_grads: bool = False):
        """`extra`: additional trainable bf16 tensors outside the model's own table — (name, flat live tensor, decayed,
        bucket key), e.g. LoRA adapters. `only`: restrict the stage's trainable set to these HF names (whole fused groups;
        diagnostics / tests: optimizer state for a handful of tensors instead of the model). `shard_params`: the buckets
        of every FSDP unit (param_sharded_key) keep NO full bf16 copy — each rank holds its 1/world slice (`own`), the unit
        is gathered around its use (FSDP FULL_SHARD, fsdp.py:84-87; TrainStep(shard_params=True))."""
        self.w, self.stage = w, stage
        specs = w._specs()
        names = set(trainable_names(w, stage))
        if only is not None:
            keep = set(only)
            for g in w.groups:
                if keep & set(g.members):
                    keep |= set(g.members)
            names &= keep
        self.names = names
        self.units: List[Unit] = []
        self.by_name: Dict[str, Unit] = {}
        self.layout = lay = ShardLayout(world, rank)

        def add(key: str, numel: int, group, dst, decay: bool, members) -> None:
            """One unit at the end of the bucket that is open."""
            u = Unit(key, 0, numel, group, dst, decay, len(lay.buckets) - 1, tuple(members))
            u.offset = lay.add(numel, len(self.units))
            self.units.append(u)
            for n in members:
                self.by_name[n] = u
        cur = None
        for gi, g in enumerate(w.groups):                       # GEMM weight groups (all decayed: ndim >= 2)
            tr = [n in names for n in g.members]
            if not any(tr):
                continue
            assert all(tr), f"group {g.members} is only partly trainable"
            key = bucket_key(g.members[0])
            if key != cur:
                lay.begin(key, True)
                cur = key
            add(f"group{gi}", g.n * g.k, g, None, True, g.members)
        EMBED = "language_model.model.embed_tokens.weight"
        # (bucket key, decayed, names): the token embeddings are half of the reference's root FSDP unit (fsdp.py:160-168) and get
        # a bucket of their own right behind the GEMM-weight buckets (parameter-sharded with them); the other plain tensors
        # (norm scales, biases, LayerScale, position / class tokens: 0.1 % of the model) share one bucket per weight-decay class
        plain_buckets = [("llm.embed", True, [EMBED])] if EMBED in names and w.placements[EMBED].group is None else []
        for decay in (True, False):
            plain_buckets.append(("plain.decay" if decay else "plain.nodecay", decay,
                                  [n for n, pl in w.placements.items() if pl.group is None and n in names and n != EMBED
                                   and (not no_decay(n, specs[n].shape)) == decay]))
        for bkey, decay, members in plain_buckets:
            todo = [(n, w.placements[n]) for n in members]
            if not todo:
                continue
            lay.begin(bkey, decay)
            for name, pl in todo:
                assert pl.ld == pl.cols or pl.rows == 1
                dst = pl.dst.view(-1)[pl.offset:pl.offset + pl.rows * pl.cols]
                add(name, dst.numel(), None, dst, decay, (name,))
        cur = None
        for name, dst, decay, bkey in (extra or []):
            if bkey != cur:
                lay.begin(bkey, decay)
                cur = bkey
            assert dst.is_contiguous() and dst.dtype == torch.bfloat16 and lay.buckets[-1].decay == decay
            add(name, dst.numel(), None, dst.view(-1), decay, (name,))
        lay.close()
        self.total = lay.total
        self.n_params = sum(u.numel for u in self.units)
        dev = w.embed.device
        # Parameter-sharded buckets (FSDP FULL_SHARD units, param_sharded_key) occupy a contiguous range [lo, hi) of the
        # flat space that is CUT OUT of the addressing of the replicated buffers — the bf16 staging copy of the updated
        # parameters and the flat fp32 gradient: for those buckets a rank keeps only its 1/world slice of the parameters
        # (`own`, bf16) and of the reduced gradient (`gshard`, fp32); the full gradient of ONE unit exists transiently in
        # one of its pool's two slots (`gslots`) between that unit's weight-gradient GEMMs and its reduce-scatter, as FSDP
        # frees a unit's full gradient after reduce-scatter (fsdp.py:160-168).
        self.shard_params = shard_params
        sh = [b for b in lay.buckets if shard_params and param_sharded_key(b.key)]
        self.sharded_keys = {b.key for b in sh}
        self._cut = (sh[0].offset, sh[-1].offset + sh[-1].numel) if sh else (lay.total, lay.total)
        assert sum(b.numel for b in sh) == self._cut[1] - self._cut[0], "parameter-sharded buckets must be contiguous"
        self._n_rep = n_rep = lay.total - (self._cut[1] - self._cut[0])
        self.stage_bf16 = torch.zeros(max(n_rep, 8), dtype=torch.bfloat16, device=dev)
        self.own_off, n_own = {}, 0
        # gradient slots: per pool two transient fp32 buffers sized for the pool's largest bucket; a bucket uses slot
        # (its index in the pool's forward order) % 2 — for the decoder layers that is layer % 2
        self.grad_slot_of: Dict[str, Tuple[str, int]] = {}
        self._slot_numel: Dict[str, int] = {}
        seen: Dict[str, int] = {}
        for b in sh:
            self.own_off[b.key] = n_own
            n_own += lay.shard_numel(b)
            pool = pool_of(b.key)
            self.grad_slot_of[b.key] = (pool, seen.get(pool, 0) % 2)
            seen[pool] = seen.get(pool, 0) + 1
            self._slot_numel[pool] = max(self._slot_numel.get(pool, 0), b.numel)
        self._n_own = n_own
        self.own = torch.zeros(max(n_own, 8), dtype=torch.bfloat16, device=dev) if sh else None
        self.grad = self.gshard = None
        self.gslots: Dict[str, List[torch.Tensor]] = {}
        self.use_grad_slots = True          # TrainStep clears it when no collective runs (world 1): the "slice" is then the whole
                                            # bucket and the weight-gradient GEMMs write the persistent buffer directly
        if not defer_grads:                 # TrainStep defers: it first gives the model's own unit allocations back
            self.alloc_grads()
        f = lambda: torch.zeros(max(lay.local_total, 8), dtype=torch.float32, device=dev)
        self.master, self.m, self.v = f(), f(), f()
        for bi, b in enumerate(lay.buckets):                    # masters ← this rank's slice of the live bf16 weights
            full = torch.zeros(b.numel, dtype=torch.float32, device=dev)
            for ui in b.members:
                u = self.units[ui]
                sl = full[u.offset - b.offset:u.offset - b.offset + u.numel]
                if u.group is not None:
                    sl.view(u.group.n, u.group.k).copy_(_unpack(u.group.packed))
                else:
                    sl.copy_(u.dst)
            lo, hi = lay.shard_range(b)
            lo_l = lay.local_offset(b)
            self.master[lo_l:lo_l + hi - lo].copy_(full[lo - b.offset:hi - b.offset])
            if b.key in self.sharded_keys:
                self.own_slice(b).copy_(full[lo - b.offset:hi - b.offset])
            del full
        self.blocks_per_bucket = 2048
        self.partial = torch.zeros(self.blocks_per_bucket * max(len(lay.buckets), 1), dtype=torch.float32, device=dev)
        self.norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)     # [total norm, clip coefficient]
        self.step_count = 0

    def alloc_grads(self) -> None:
        """The fp32 gradient buffers: flat for the replicated buckets; this rank's slices + two transient slots per pool
        for the parameter-sharded ones."""
        if self.grad is not None:
            return
        dev = self.w.embed.device
        self.grad = torch.zeros(max(self._n_rep, 8), dtype=torch.float32, device=dev)
        if self.sharded_keys:
            self.gshard = torch.zeros(max(self._n_own, 8), dtype=torch.float32, device=dev)
            if self.use_grad_slots:
                self.gslots = {pool: [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(2)]
                               for pool, n in self._slot_numel.items()}

    # ---- views ----
    def _replicated(self, buf: torch.Tensor, offset: int, numel: int) -> torch.Tensor:
        """View of flat range [offset, offset + numel) in a buffer that skips the parameter-sharded range."""
        lo, hi = self._cut
        assert offset + numel <= lo or offset >= hi, "parameter-sharded buckets have no replicated copy"
        o = offset if offset < lo else offset - (hi - lo)
        return buf[o:o + numel]

    def stage_view(self, offset: int, numel: int) -> torch.Tensor:
        """bf16 staging view of flat range [offset, offset + numel) (never inside the parameter-sharded range)."""
        return self._replicated(self.stage_bf16, offset, numel)

    def grad_range(self, offset: int, numel: int) -> torch.Tensor:
        """fp32 gradient of flat range [offset, offset + numel) of the replicated buckets."""
        return self._replicated(self.grad, offset, numel)

    def own_slice(self, b) -> torch.Tensor:
        """This rank's bf16 slice of a parameter-sharded bucket."""
        o = self.own_off[b.key]
        return self.own[o:o + self.layout.shard_numel(b)]

    def grad_slot(self, b) -> torch.Tensor:
        """The transient full-size fp32 gradient of parameter-sharded bucket b (decoder layer l uses slot l % 2 of the
        layer pool; the vision / head units alternate inside their pools)."""
        if not self.use_grad_slots:          # one rank, no collective: the rank's slice of the reduced gradient is the bucket itself
            assert self.layout.world == 1
            return self.reduced_grad(b)
        pool, parity = self.grad_slot_of[b.key]
        return self.gslots[pool][parity][:b.numel]

    def reduced_grad(self, b) -> torch.Tensor:
        """This rank's slice of bucket b's gradient once reduced: what the norm and AdamW read."""
        if b.key in self.sharded_keys:
            o = self.own_off[b.key]
            return self.gshard[o:o + self.layout.shard_numel(b)]
        lo, hi = self.layout.shard_range(b)
        return self.grad_range(lo, hi - lo)

    def _unit_grad(self, u: Unit) -> torch.Tensor:
        b = self.layout.buckets[u.bucket]
        if b.key in self.sharded_keys:
            return self.grad_slot(b)[u.offset - b.offset:u.offset - b.offset + u.numel]
        return self.grad_range(u.offset, u.numel)

    def grad_view(self, name_or_unit) -> torch.Tensor:
        """fp32 gradient of a unit: [n, k] for a group, flat for a plain tensor (for a parameter-sharded unit: the
        transient slot its weight-gradient GEMMs write — valid until the slot's next unit overwrites it)."""
        u = name_or_unit if isinstance(name_or_unit, Unit) else self.by_name[name_or_unit]
        sl = self._unit_grad(u)
        return sl.view(u.group.n, u.group.k) if u.group is not None else sl

    def _named(self, flat: Optional[torch.Tensor], name: str, unit_slice: Optional[torch.Tensor] = None) -> torch.Tensor:
        u = self.by_name[name]
        sl = unit_slice if unit_slice is not None else flat[u.offset:u.offset + u.numel]
        if name not in self.w.placements:                       # extra unit: flat
            return sl
        pl = self.w.placements[name]
        shape = self.w._specs()[name].shape
        if u.group is None:
            return sl.view(shape)
        return _block_view(sl, pl).reshape(shape)

    def named_grad(self, name: str) -> torch.Tensor:
        """Gradient under its HF name / shape (a copy for grouped tensors): the local, un-reduced gradient of a replicated
        bucket. Parameter-sharded units have no such thing once collectives run — their full gradient lives in a transient
        slot that the flush reduce-scatters in place and later units overwrite — so this raises for them; without
        collectives (one rank) the rank's "slice" is the whole bucket and the call is valid."""
        u = self.by_name[name]
        if self.layout.buckets[u.bucket].key in self.sharded_keys and self.use_grad_slots:
            raise RuntimeError(f"{name}: the full gradient of a parameter-sharded unit is transient (reduce-scattered in its slot, "
                               "overwritten two units later); read store.reduced_grad(bucket) — this rank's reduced slice — instead")
        return self._named(None, name, self._unit_grad(u))

    def full_master(self, comm: Optional[ShardComm] = None) -> torch.Tensor:
        """All fp32 masters in the flat layout (gathered over ranks when sharded) — checkpoints and tests."""
        return (comm or ShardComm(self.layout)).gather_full(self.master)

    def named_master(self, name: str, full: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._named(self.full_master() if full is None else full, name)

    def master_state_dict(self, comm: Optional[ShardComm] = None) -> Dict[str, torch.Tensor]:
        full = self.full_master(comm)
        return {n: self._named(full, n).clone() for n in self.by_name}

    def trainable(self, name: str) -> bool:
        return name in self.by_name

    def unit_of_packed(self, packed: torch.Tensor) -> Optional[Unit]:
        for u in self.units:
            if u.group is not None and u.group.packed.data_ptr() == packed.data_ptr():
                return u
        return None
