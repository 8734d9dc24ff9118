"""Parameter sharding (FSDP FULL_SHARD) of the training step: decoder layers ("layers" pool), ViT blocks + patch embeddings
("vision"), projector / token embeddings / lm_head ("head"). `UnitPools` owns the gather slots and their events, the
communication stream, and the ops a plan uses to gather, await, release and flush one unit (DESIGN.md "Parameter sharding")."""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional

import torch

from .. import ops, train_ops as T
from ..ops import Op
from ..weights import VLAWeights
from .param_store import ParamStore, Unit
from .sharding import ShardComm


class UnitPools:
    """One machinery for every FSDP unit of the reference (prismatic.py:285-306, dinosiglip_vit.py:136-140,
    fsdp.py:160-168): per pool TWO gather slots — the logical bf16 bucket + one buffer of forward layouts + one of dgrad
    layouts, each sized for the pool's largest unit and carved into per-unit views — the model's tensors are re-pointed
    at the views of slot (unit index % 2; decoder layer l: l % 2) and the pool's own allocation is freed. A unit is
    all-gathered (and packed) into its slot one unit ahead of its use, on the communication stream; its weight gradients
    go to one of two transient fp32 slots of the pool and are reduce-scattered into the rank's persistent slice right
    after the unit's last weight-gradient GEMM. The token embeddings are a plain [vocab, D] tensor: read in place from the
    gathered bucket. Under `fp8` a decoder layer's gather quantises instead of packing: the slot carries the e4m3
    forward / dgrad copies (+ scales, in the `Linears` record of the slot view) and no bf16 dgrad layouts."""

    def __init__(self, w: VLAWeights, store: ParamStore, comm: ShardComm, lin, recompute: bool, fp8: bool):
        """`lin`: the step's `Linears`, whose e4m3 entries and quantising ops the fp8 slots use."""
        self.w, self.store, self.comm = w, store, comm
        st, lay, dev = store, store.layout, w.embed.device
        by_group = {id(u.group): u for u in st.units if u.group is not None}
        by_key = {b.key: b for b in lay.buckets}
        self.units: Dict[str, dict] = {}       # bucket key → its pool, slot parity, bucket, slot views' Units and dgrad layouts, gather-time ops
        self.slots: Dict[str, List[dict]] = {}
        self.params_updated = torch.cuda.Event()       # end of the last optimizer_step: parameter gathers wait for it
        self.materialized = False
        self._planned: Optional[str] = None    # the unit inside `planning()`
        self.comm_stream: Optional[torch.cuda.Stream] = None       # set by `start`, after the plans are built: the glue ops read it when they run
        self.rs_scratch: Optional[torch.Tensor] = None
        if fp8:
            lin.fp8_scratch()
        for pool in ("layers", "vision", "head"):
            fields = w.unit_fields(pool)                                   # (unit key, path, group index | None, HF name | None)
            keys = list(dict.fromkeys(k for k, *_ in fields))
            live = [k for k in keys if k in st.sharded_keys]
            if not live:
                continue
            if len(live) != len(keys):
                raise ValueError(f"parameter sharding needs every unit of the {pool} pool trainable or none "
                                 f"({sorted(set(keys) - set(live))} frozen; the decoder layers: vla-full-train / vla-train)")
            fp8_pool = fp8 and pool == "layers"
            numel = lambda k: sum(w.groups[gi].n * w.groups[gi].k for kk, _, gi, _ in fields if kk == k and gi is not None)
            flat_max, pk_max = max(by_key[k].numel for k in keys), max(max(numel(k) for k in keys), 8)
            slots = [dict(flat=torch.zeros(flat_max, dtype=torch.bfloat16, device=dev),
                          fwd=torch.zeros(pk_max, dtype=torch.bfloat16, device=dev),
                          bwd=None if fp8_pool else torch.zeros(pk_max, dtype=torch.bfloat16, device=dev),
                          ready=torch.cuda.Event(), free=torch.cuda.Event(), grads_flushed=torch.cuda.Event()) for _ in range(2)]
            self.slots[pool] = slots
            views: Dict[tuple, torch.Tensor] = {}
            for k in keys:
                b = by_key[k]
                parity = st.grad_slot_of[k][1]
                slot, off = slots[parity], 0
                info = dict(pool=pool, parity=parity, bucket=b, by_ptr={}, T={}, fwd_ops=[], bwd_ops=[])
                for kk, path, gi, name in fields:
                    if kk != k:
                        continue
                    if gi is not None:
                        u = by_group[id(w.groups[gi])]
                        n, kd = u.group.n, u.group.k
                        fv = slot["fwd"][off:off + n * kd].view(n // 16, kd // 32, 64, 8)
                        rm = slot["flat"][u.offset - b.offset:u.offset - b.offset + u.numel].view(n, kd)
                        if fp8_pool:                                       # the units of one parity share the slot's e4m3 copies
                            q = lin.fp8_weight_ops(rm, fv)
                            info["fwd_ops"] += q[:2]
                            info["bwd_ops"] += q[2:]
                        else:
                            tv = slot["bwd"][off:off + n * kd].view(kd // 16, n // 32, 64, 8)
                            info["fwd_ops"].append(T.pack(rm, fv, run=False))
                            info["bwd_ops"].append(T.transpose_pack(rm, tv, n, run=False))
                            info["T"][fv.data_ptr()] = tv
                        off += n * kd
                        info["by_ptr"][fv.data_ptr()] = u
                        views[(k, path)] = fv
                    else:                                                  # token embeddings: used where the gather lands them
                        u = st.by_name[name]
                        obj, attr = w._attr_of(path)
                        views[(k, path)] = slot["flat"][u.offset - b.offset:u.offset - b.offset + u.numel].view(getattr(obj, attr).shape)
                        u.dst = None                                       # the optimizer writes the rank's slice, nothing is copied back
                if recompute and pool == "layers":                         # the backward pass replays the layer's forward
                    info["bwd_ops"] = info["bwd_ops"] + info["fwd_ops"]
                self.units[k] = info
            if w.pool_resident(pool):
                w.release_unit_weights(pool, views)
            else:                                  # re-planned step over an already sharded model
                w.repoint_unit_weights(pool, views)

    def start(self, comm_stream: torch.cuda.Stream, reduce_dtype: torch.dtype) -> None:
        """The communication stream the gathers and flushes are issued on, and the bf16 wire copy of one unit's gradients."""
        self.comm_stream = comm_stream
        if self.comm.active and reduce_dtype != torch.float32:
            self.rs_scratch = torch.zeros(max(self.store._slot_numel.values()), dtype=torch.bfloat16, device=self.w.embed.device)

    def slot(self, key: str) -> dict:
        info = self.units[key]
        return self.slots[info["pool"]][info["parity"]]

    def gather(self, key: str, backward: bool = False, both: bool = False) -> Op:
        """Issue unit `key`'s parameter gather + packing (forward layouts, dgrad layouts, or both) on the communication stream."""
        def fn():
            info, slot, side = self.units[key], self.slot(key), self.comm_stream
            side.wait_event(self.params_updated)              # AdamW (main stream) has written the rank's slice
            side.wait_event(slot["free"])                     # the unit that used this slot before is done with it
            with torch.cuda.stream(side):
                b = info["bucket"]
                self.comm.all_gather_into(slot["flat"][:b.numel], self.store.own_slice(b))
                if both or not backward:
                    ops.run_all(info["fwd_ops"])
                if both or backward:
                    ops.run_all(info["bwd_ops"])
                slot["ready"].record(side)
        return ops.glue("gather_unit_params", fn, ())

    def await_(self, key: str) -> Op:
        return ops.glue("await_unit_params", lambda: torch.cuda.current_stream().wait_event(self.slot(key)["ready"]), ())

    def release(self, key: str) -> Op:
        return ops.glue("release_unit_params", lambda: self.slot(key)["free"].record(torch.cuda.current_stream()), ())

    def await_grad(self, key: str) -> Op:
        return ops.glue("await_unit_grad_slot", lambda: torch.cuda.current_stream().wait_event(self.slot(key)["grads_flushed"]), ())

    def flush(self, key: str) -> Op:
        """After the unit's last weight gradient: reduce-scatter its transient fp32 slot, keep this rank's slice."""
        def fn():
            st, lay, side = self.store, self.store.layout, self.comm_stream
            if not st.use_grad_slots:
                return
            b = self.units[key]["bucket"]
            gs = st.grad_slot(b)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            side.wait_event(ev)
            with torch.cuda.stream(side):
                scratch = self.rs_scratch[:b.numel] if self.rs_scratch is not None else None
                self.comm.reduce_scatter_bucket(gs, b, scratch)
                n = lay.shard_numel(b)
                T.copy_f32(gs[lay.rank * n:(lay.rank + 1) * n], st.reduced_grad(b))
                self.slot(key)["grads_flushed"].record(side)
        return ops.glue("flush_unit_grads", fn, ())

    @contextlib.contextmanager
    def planning(self, key: str):
        """While the backward ops of unit `key` are planned: the two units of a pool that share a gather slot share its
        views too, so one pointer means two weights, and `unit_of` / `transposed` answer for the unit named here."""
        assert self._planned is None and key in self.units
        self._planned = key
        try:
            yield
        finally:
            self._planned = None

    def unit_of(self, packed: torch.Tensor) -> Optional[Unit]:
        """The optimizer unit behind a slot view of the unit being planned; None for any other tensor."""
        return self.units[self._planned]["by_ptr"].get(packed.data_ptr()) if self._planned is not None else None

    def transposed(self, packed: torch.Tensor) -> Optional[torch.Tensor]:
        """The dgrad layout behind a slot view of the unit being planned; None for a weight that lives in no slot."""
        key = packed.data_ptr()
        if self._planned is not None and key in self.units[self._planned]["T"]:
            return self.units[self._planned]["T"][key]
        assert not any(key in info["T"] for info in self.units.values()), "slot weights are addressed while their unit is planned"
        return None

    def seq(self, seq: List[str], j: int, backward: bool, body: List[Op]) -> List[Op]:
        """Ops of unit seq[j] wrapped in its parameter / gradient-slot protocol: wait for its gather, start the next unit's
        gather (after this unit's release when both share a slot), and in the backward pass wait for the gradient slot and
        flush it afterwards. Units that are not parameter-sharded pass through."""
        key = seq[j]
        if key not in self.units:
            return body
        nxt = seq[j + 1] if j + 1 < len(seq) and seq[j + 1] in self.units else None
        same = nxt is not None and self.slot(nxt) is self.slot(key)
        pre: List[Op] = []
        if j == 0:
            pre.append(self.gather(key, backward))
        pre.append(self.await_(key))
        if nxt is not None and not same:
            pre.append(self.gather(nxt, backward))
        if backward:
            pre.append(self.await_grad(key))
        post = [self.release(key)]
        if backward:
            post.append(self.flush(key))
        if nxt is not None and same:
            post.append(self.gather(nxt, backward))
        return pre + body + post

    def materialize_params(self) -> None:
        """Bring every parameter-sharded unit back into the model's own allocation (gather each unit, pack) — for inference,
        `state_dict()` / `save_pretrained` after parameter-sharded training. The step's plans address the slots, so the
        step object cannot train afterwards."""
        if self.materialized:
            return
        w, st = self.w, self.store
        by_group = {id(u.group): u for u in st.units if u.group is not None}
        for pool, slots in self.slots.items():
            w.restore_unit_weights(pool)
            cur = None
            for key, path, gi, name in w.unit_fields(pool):
                info = self.units[key]
                b, slot = info["bucket"], slots[info["parity"]]
                if key != cur:
                    torch.cuda.synchronize()                # a slot is re-used by the next unit of its parity
                    self.comm.all_gather_into(slot["flat"][:b.numel], st.own_slice(b))
                    cur = key
                obj, attr = w._attr_of(path)
                u = by_group[id(w.groups[gi])] if gi is not None else st.by_name[name]
                rm = slot["flat"][u.offset - b.offset:u.offset - b.offset + u.numel]
                if gi is not None:
                    T.pack(rm.view(u.group.n, u.group.k), getattr(obj, attr))
                else:
                    getattr(obj, attr).view(-1).copy_(rm)
        torch.cuda.synchronize()
        self.materialized = True
