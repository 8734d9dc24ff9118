"""The batched requantisation of the adapted decoder weights (bl_quantize_weight_fp8_packed_batched: the four GEMM groups of all
32 decoder layers, 128 entries, in one launch) at 7B, against a plain device copy (bl_copy_bytes) of the same bytes READ,
alternating in one process, best of several rounds; and the whole refresh of `LoraAdapters.enable_fp8()` (merge + quantise)
against the merge alone. `--step` adds the LoRA training step (B = 16) with refresh_adapted=True, fp8 copies off and on,
alternating.  python tools/bench_weight_fp8.py [--rounds 5] [--iters 3] [--step] [--out profiles/bench_weight_fp8.json]"""
import argparse, json, sys, torch
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bridgelang_amd import ops, train_ops as T, weights as W
from bridgelang_amd.training.lora import RP, LoraAdapters

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--step", action="store_true", help="also time TrainStep('lora', refresh_adapted=True) with fp8 copies off / on")
ap.add_argument("--step-iters", type=int, default=5)
ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "bench_weight_fp8.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
w = W.allocate(W.openvla_7b_dims(), dev).fill_synthetic(seed=0)


def adapters() -> LoraAdapters:
    lora = LoraAdapters(w, r=args.rank)
    g = torch.Generator(device=dev).manual_seed(0)
    for ad in lora.adapters:                               # trained-looking adapters: B non-zero inside its block structure
        for j in range(len(ad.modules)):
            rows = ad.member_rows(j).to(dev)
            blk = torch.zeros(len(rows), RP, device=dev)
            blk[:, :args.rank] = torch.randn(len(rows), args.rank, device=dev, generator=g) * 0.01
            ad.B[rows, j * RP:(j + 1) * RP] = blk.to(torch.bfloat16)
    return lora


lora = adapters().enable_fp8()
refresh = lora._plan()                                     # not handed out: the plan of refresh()
assert [op.name for op in refresh] == ["bl_lora_merge_batched_bf16", "bl_quantize_weight_fp8_packed_batched"]
merge, quant = refresh[:1], refresh[1:]
read_bytes = sum(getattr(lw, n).numel() * 2 for lw in lora.adapted_weights().layers for n in ("qkv_w", "o_w", "gu_w", "down_w"))
src = torch.empty(read_bytes // 2, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
scratch = torch.empty_like(src)
copy = [T.copy_f32(src, scratch, run=False)]


def timed(plan, iters) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.run_all(plan)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


ops.run_all(refresh + copy)
torch.cuda.synchronize()
t = {"quant": [], "copy": [], "merge": [], "refresh": []}
for _ in range(args.rounds):
    t["quant"].append(timed(quant, args.iters))
    t["copy"].append(timed(copy, args.iters))
    t["merge"].append(timed(merge, args.iters))
    t["refresh"].append(timed(refresh, args.iters))
best = {k: min(v) for k, v in t.items()}
res = {"what": "bl_quantize_weight_fp8_packed_batched vs bl_copy_bytes of the same bytes read; merge + quantise vs merge; 7B",
       "rank": args.rank, "entries": 4 * len(lora._fp8), "bytes_read": read_bytes, "bytes_written": read_bytes // 2,
       "rounds": args.rounds, "iters": args.iters,
       "quant_ms": round(best["quant"], 3), "copy_ms": round(best["copy"], 3), "quant_over_copy": round(best["quant"] / best["copy"], 3),
       "quant_TBps": round(1.5 * read_bytes / best["quant"] / 1e9, 3), "copy_TBps": round(2 * read_bytes / best["copy"] / 1e9, 3),
       "merge_ms": round(best["merge"], 3), "refresh_ms": round(best["refresh"], 3),
       "refresh_minus_merge_ms": round(best["refresh"] - best["merge"], 3),
       **{f"{k}_ms_all": [round(x, 3) for x in v] for k, v in t.items()}}

if args.step:
    from bridgelang_amd.training.step import TrainStep
    B, L = 16, 40
    g = torch.Generator().manual_seed(100)
    ids = torch.randint(3, 31000, (B, L), generator=g)
    ids[:, 0] = 1
    ids[:, -8:-1] = torch.randint(31744, 32000, (B, 7), generator=g)
    ids[:, -1] = 2
    labels = torch.full((B, L), -100)
    labels[:, -8:] = ids[:, -8:]
    pv = (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16)
    steps = {}
    for name, lo in (("bf16", LoraAdapters(w, r=args.rank)), ("fp8", LoraAdapters(w, r=args.rank).enable_fp8())):
        ts = TrainStep(w, "lora", B, L, max_grad_norm=float("inf"), weight_decay=0.01, lora=lo, refresh_adapted=True)
        ts.set_batch(ids, None, pv, labels)
        for _ in range(2):
            ts.step(5e-4, graph=True)
        steps[name] = ts
    torch.cuda.synchronize()
    st = {"bf16": [], "fp8": []}
    for _ in range(2):
        for name, ts in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.step_iters):
                ts.step(5e-4, graph=True)
            e1.record()
            torch.cuda.synchronize()
            st[name].append(round(e0.elapsed_time(e1) / args.step_iters, 3))
    res.update({"lora_step_B16_refresh_bf16_ms": st["bf16"], "lora_step_B16_refresh_fp8_ms": st["fp8"]})

print(json.dumps(res))
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
