"""What do the op plans launch? One JSON line per op of the inference engines, the staggered pipelines and the training
step (every stage, loss and option that changes a plan) on synthetic reduced-width weights: the kernel's name, every scalar
argument and every field of its descriptors (device tables included), each device pointer as (owner, byte offset into the
owner's allocation). An owner is named "a<ordinal>:<bytes>": the ordinal of the allocation's first appearance while a
configuration's lists are walked in order, and its size — so the names do not depend on which object or attribute holds the
allocation, only on which launches share it. A pointer that nothing reachable from the engine / pipeline / step holds is an
error. For the training step the (position, bucket) list of the per-bucket reduce-scatter is written too, and for sharded
parameters each unit's gather-time layout ops (the glue ops of the plans carry no tensors).
Two runs print the same lines exactly when the plans are the same launches on the same buffers:
   python tools/plan_fingerprint.py --out before.jsonl      (at one commit)
   python tools/plan_fingerprint.py --out after.jsonl       (at another; then diff the two files)
Run it before and after any change that is meant to leave the plans alone. Needs a GPU (tensors only; no plan is run)."""
import argparse, bisect, ctypes as C, dataclasses, json, sys
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bridgelang_amd import _lib, weights as W
from bridgelang_amd.engine import OpenVLAEngine
from bridgelang_amd.ops import Op
from bridgelang_amd.pipeline import StaggeredDecodePipeline

TABLES = {"bl_batched_ops": _lib.BatchOpDesc, "bl_lora_merge_batched_bf16": _lib.LoraMergeDesc,
          "bl_quantize_weight_fp8_packed_batched": _lib.WeightQuantDesc}      # ops whose first argument is a device table


def held_tensors(obj, path, seen):
    """(attribute path, tensor) for every device tensor reachable from obj — through containers and the project's own
    objects, not through Ops (a plan's tensors must be held by whoever owns the plan). Deterministic order."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            yield path, obj
        return
    if id(obj) in seen or isinstance(obj, (Op, str, bytes, int, float, type(None))):
        return
    seen.add(id(obj))
    if isinstance(obj, dict):
        for i, (k, v) in enumerate(obj.items()):
            yield from held_tensors(v, f"{path}[{k!r}]" if isinstance(k, str) else f"{path}[#{i}]", seen)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from held_tensors(v, f"{path}[{i}]", seen)
    elif type(obj).__module__.startswith("bridgelang_amd"):
        for k in sorted(set(getattr(obj, "__dict__", {})) | set(getattr(type(obj), "__slots__", ()))):
            yield from held_tensors(getattr(obj, k, None), f"{path}.{k}", seen)


class Owners:
    """Allocation intervals [base, end). `find` names one "a<ordinal of first use>:<bytes>" (or, with `named`, by the
    first path that reaches it: an op's own tensors)."""

    def __init__(self, pairs, named=False):
        spans = {}
        for path, t in pairs:
            st = t.untyped_storage()
            if st.nbytes():
                spans.setdefault(st.data_ptr(), (st.data_ptr() + st.nbytes(), path if named else None))
        self.bases = sorted(spans)
        self.spans = spans
        self.n_used = 0

    def find(self, p):
        i = bisect.bisect_right(self.bases, p) - 1
        if i >= 0 and p < self.spans[self.bases[i]][0]:
            base = self.bases[i]
            end, name = self.spans[base]
            if name is None:
                name = f"a{self.n_used}:{end - base}"
                self.spans[base] = (end, name)
                self.n_used += 1
            return [name, p - base]
        return None


def describe(op, owners):
    """The JSON record of one op."""
    own = Owners(((f"keep[{i}]", t) for i, k in enumerate(op.keep) for _, t in held_tensors(k, "", set())), named=True)

    def ptr(p):
        if not p:
            return None
        r = owners.find(p) or own.find(p)       # a device table or index vector made for this op alone is the op's own
        if r is None:
            raise LookupError(f"{op.name}: pointer {p:#x} lies in no tensor the plan's owner holds")
        return r

    def struct(s):
        return {n: ptr(getattr(s, n)) if t is C.c_void_p else getattr(s, n) for n, t in s._fields_}

    def arg(a, t):
        if isinstance(a, C.Array):
            return [ptr(v) if a._type_ is C.c_void_p else v for v in a]
        if hasattr(a, "_obj"):                  # byref(descriptor)
            return struct(a._obj)
        return ptr(a) if t is C.c_void_p else a

    argtypes = getattr(op.fn, "argtypes", None)
    if argtypes is None:                        # host-side glue: its name and the tensors it touches
        return {"name": op.name, "keep": [ptr(t.data_ptr()) for _, t in held_tensors(list(op.keep), "", set())]}
    assert len(op.args) == len(argtypes) - 1, op.name
    rec = {"name": op.name, "args": [arg(a, t) for a, t in zip(op.args, argtypes)]}
    if op.name in TABLES:
        n = op.args[2] if op.name == "bl_batched_ops" else op.args[1]
        raw = bytes(op.keep[0].cpu().numpy())
        rec["table"] = [struct(d) for d in (TABLES[op.name] * n).from_buffer_copy(raw)]
        if op.name == "bl_batched_ops":
            rec["block_start"] = op.keep[1].tolist()
    return rec


def configurations(dev):
    """(name, owner object, {list name: ops}) one at a time."""
    tiny = W.tiny_dims()
    new = lambda dims=tiny: W.allocate(dims, dev).fill_synthetic(seed=0)

    def engine(name, w, B=2, **kw):
        e = OpenVLAEngine(w, B, 8, 3, **kw)
        lists = {"dino_ops": e.dino_ops, "siglip_ops": e.siglip_ops, "projector_ops": e.projector_ops, "prefill_ops": e.prefill_ops}
        lists.update({f"decode_ops[{t}]": p for t, p in enumerate(e.decode_ops)})
        return name, e, lists, e.layer_ends

    def pipeline(name, w, B=2, n_new=3, **kw):
        p = StaggeredDecodePipeline(w, B, 8, n_new, **kw)
        return name, p, {f"merged_ops[{k}]": m for k, m in enumerate(p.merged_ops)}, None

    w = new()
    rng = dict(vocab_range=(31744, 256))
    for name, kw in (("default", {}), ("all_rows", dict(all_rows=True)), ("use_mask", dict(use_mask=True)), ("padded", dict(padded=True)),
                     ("fp8", dict(fp8=True)), ("text_only", dict(text_only=True)), ("sample", dict(sample=True, **rng)),
                     ("score", dict(score=True, score_range=(31800, 16), **rng)), ("splitk", dict(splitk=True))):
        yield engine(f"engine {name}", w, **kw)
    yield engine("engine B=17", w, B=17)
    yield engine("engine B=17 fp8", w, B=17, fp8=True)
    w64 = new(dataclasses.replace(tiny, llm_heads=8))
    yield engine("engine head_dim 64", w64)
    yield engine("engine one layer", new(W.tiny_dims(llm_layers=1)))
    from bridgelang_amd.training.lora import LoraAdapters
    yield engine("engine adapted fp8", LoraAdapters(new(), r=8).enable_fp8().adapted_weights(), fp8=True)
    for name, kw in (("default", {}), ("split_vision", dict(split_vision=True)), ("padded", dict(padded=True)), ("fp8", dict(fp8=True)),
                     ("sample", dict(sample=True)), ("score", dict(score=True, score_range=(31800, 16))), ("n_new=10", dict(n_new=10)),
                     ("B=17", dict(B=17)), ("B=8 n_new=18", dict(B=8, n_new=18))):
        yield pipeline(f"pipeline {name}", w, **kw)
    yield pipeline("pipeline head_dim 64", w64)
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.value_loss import ValueLossConfig

    def step(name, stage, w=None, **kw):
        """Fresh weights per step: a parameter-sharded step frees the model's own allocations."""
        ts = TrainStep(w or new(), stage, 2, 8, **kw)
        lists = {"vision_forward_ops": ts.vision_forward_ops, "forward_ops": ts.forward_ops, "backward_ops": ts.backward_ops,
                 "repack_ops": ts.repack_ops}
        units = ts.pools.units if ts.pools is not None else {}      # parameter-sharded units: {bucket key: its gather-time layout ops}
        for key, info in units.items():
            lists[f"unit[{key}].fwd_ops"], lists[f"unit[{key}].bwd_ops"] = info["fwd_ops"], info["bwd_ops"]
        towers = {"vfwd_tower": [len(p) for p in ts._vfwd_tower], "bwd_tower_at": getattr(ts, "_bwd_tower_at", None)}
        return f"train step {name}", ts, lists, {"ready": ts._ready, **towers}

    yield step("fp8", "vla-train", fp8=True)
    yield step("fp8 fp8_wgrad", "vla-train", fp8=True, fp8_wgrad=True)
    yield step("vla-train", "vla-train")
    yield step("vla-full-train", "vla-full-train")
    yield step("vla-full-train recompute", "vla-full-train", recompute=True)
    yield step("vla-full-train shard_params", "vla-full-train", shard_params=True)
    yield step("vla-train fp8 shard_params", "vla-train", fp8=True, shard_params=True)
    yield step("vla-last-layer-train", "vla-last-layer-train")
    yield step("align", "align")
    for name, kw in (("lora r=8", {}), ("lora r=8 dropout=0.1", dict(dropout=0.1))):
        ad = LoraAdapters(new(), r=8, **kw)
        yield step(name, "lora", w=ad.w, lora=ad)
    ad = LoraAdapters(new(), r=8).enable_fp8()
    yield step("lora refresh_adapted fp8", "lora", w=ad.w, lora=ad, refresh_adapted=True)
    yield step("vla-train loss=policy", "vla-train", loss="policy", value=ValueLossConfig(),
               policy=PolicyLossConfig(token_range=(31744, 256), ratio_level="action"))
    yield step("vla-train loss=preference", "vla-train", loss="preference")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    n_ops = 0
    with open(a.out, "w") as f:
        for cfg, owner, lists, marks in configurations(torch.device("cuda:0")):
            owners = Owners(held_tensors(owner, "", set()))
            if marks is not None:               # positions inside the lists: layer ends / bucket-ready markers / tower splits
                f.write(json.dumps({"cfg": cfg, **(marks if isinstance(marks, dict) else {"layer_ends": marks})}) + "\n")
            for lname, plan in lists.items():
                for i, op in enumerate(plan):
                    f.write(json.dumps({"cfg": cfg, "list": lname, "i": i, **describe(op, owners)}) + "\n")
                n_ops += len(plan)
            print(f"{cfg}: {sum(len(p) for p in lists.values())} ops", flush=True)
    print(f"{n_ops} ops written to {a.out}")


if __name__ == "__main__":
    main()
