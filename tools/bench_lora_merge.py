"""The batched LoRA refresh (bl_lora_merge_batched_bf16: every adapted group of the model in one launch) at 7B, rank 32,
against a plain device copy of the same bytes read and written (bl_copy_bytes), alternating in one process, best of several
rounds.  python tools/bench_lora_merge.py [--rounds 5] [--iters 3] [--out profiles/bench_lora_merge.json]"""
import argparse, json, sys, torch
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bridgelang_amd import ops, train_ops as T, weights as W
from bridgelang_amd.training.lora import RP, LoraAdapters

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "bench_lora_merge.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
w = W.allocate(W.openvla_7b_dims(), dev).fill_synthetic(seed=0)
lora = LoraAdapters(w, r=args.rank)
g = torch.Generator(device=dev).manual_seed(0)
for ad in lora.adapters:                                   # trained-looking adapters: B non-zero inside its block structure
    m = len(ad.modules)
    for j in range(m):
        rows = ad.member_rows(j).to(dev)
        blk = torch.zeros(len(rows), RP, device=dev)
        blk[:, :args.rank] = torch.randn(len(rows), args.rank, device=dev, generator=g) * 0.01
        ad.B[rows, j * RP:(j + 1) * RP] = blk.to(torch.bfloat16)
view = lora.adapted_weights()
merge = lora.refresh_ops()
nbytes = sum(ad.group.n * ad.group.k * 2 for ad in lora.adapters)
assert view.adapted_arena.nbytes >= nbytes
src = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
scratch = torch.empty_like(src)                            # the copy's destination: the merge's results are left alone
copy = [T.copy_f32(src, scratch, run=False)]


def timed(plan) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        ops.run_all(plan)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


ops.run_all(merge + copy)
torch.cuda.synchronize()
t_merge, t_copy = [], []
for _ in range(args.rounds):
    t_merge.append(timed(merge))
    t_copy.append(timed(copy))
bm, bc = min(t_merge), min(t_copy)
res = {"what": "bl_lora_merge_batched_bf16 vs bl_copy_bytes of the same bytes, 7B, all adapted groups",
       "rank": args.rank, "groups": len(lora.adapters), "bytes_read_and_written_each": nbytes, "rounds": args.rounds, "iters": args.iters,
       "merge_ms": round(bm, 3), "copy_ms": round(bc, 3), "merge_over_copy": round(bm / bc, 3),
       "merge_TBps": round(2 * nbytes / bm / 1e9, 3), "copy_TBps": round(2 * nbytes / bc / 1e9, 3),
       "merge_ms_all": [round(t, 3) for t in t_merge], "copy_ms_all": [round(t, 3) for t in t_copy]}
print(json.dumps(res))
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
