#!/usr/bin/env python
"""What the shared-prompt training step saves: `TrainStep(shared_prompt=G)` against the replicated step of the same
sequences; one JSON line. A record: the one condition is stated at the end.

  step     7B, stage "lora" (r = 32), loss="policy", P prompts × G samples, L = 40 (32 prompt ids + 7 action ids + EOS, the
           benchmark's batch with every prompt repeated G times and the action ids redrawn per sample), graph replay. The
           shared step (P·(288 + G·8) token rows, P images) and the replicated step (P·G·296 rows, P·G images) are built in
           ONE process on the same weights and alternate `--rounds` times, `--steps` timed steps per window after a warm-up
           step each. The two losses of the first forward are printed side by side (same sequences, two row layouts).
  parent   with --parent ROOT (a checkout of the parent commit with its library built): the replicated step alone, timed the
           same way in a child process that imports the package from ROOT, before and after the alternation — the default
           path on the parent's code, to show that it did not move. tools/ab_lib.sh alternates libraries for the GEMM shapes;
           a training step needs the parent's Python too, hence the checkout.

    python tools/bench_shared_prompt.py --parent /path/to/parent > profiles/bench_shared_prompt.json

Condition: min(shared) < min(parent replicated) − (the largest spread between the windows of any one arm).
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def grouped_inputs(P, G, L, seed=100):
    """The benchmark's batch shape (tools/bench_policy_step.py::bench_inputs) for P prompts × G samples: the G sequences of a
    prompt share ids [0, L − 8) and the image; their 7 action ids differ."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 31000, (P, L), generator=g)
    ids[:, 0] = 1
    ids = ids.repeat_interleave(G, 0)
    ids[:, -8:-1] = torch.randint(31744, 32000, (P * G, 7), generator=g)
    ids[:, -1] = 2
    labels = torch.full((P * G, L), -100)
    labels[:, -8:] = ids[:, -8:]
    pv = (torch.rand(P, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16)
    return ids, labels, pv, g


def build(args, dev, w, shared):
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    P, G, L = args.prompts, args.group, 40
    B = P * G
    ids, labels, pv, g = grouped_inputs(P, G, L)
    on = labels != -100
    kw = dict(lora=LoraAdapters(w, r=32), max_grad_norm=float("inf"), weight_decay=0.01, loss="policy", policy=PolicyLossConfig())
    if shared:
        ts = TrainStep(w, "lora", B, L, shared_prompt=G, branch_len=8, **kw)
        ts.set_batch(ids, None, pv, labels)
    else:
        ts = TrainStep(w, "lora", B, L, **kw)
        ts.set_batch(ids, None, pv.repeat_interleave(G, 0), labels)
    ts.set_policy_batch(torch.where(on, torch.randn(B, L, generator=g), torch.zeros(B, L)),
                        torch.where(on, torch.full((B, L), -10.4), torch.zeros(B, L)))
    return ts


def window(ts, steps):
    ts.step(5e-4, graph=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, _ = ts.step(5e-4, graph=True)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    return round((time.perf_counter() - t0) / steps * 1e3, 3)


def replicated_only(args):
    """The child of --parent: the replicated step of the package under args.root, alone."""
    sys.path.insert(0, args.root)
    from bridgelang_amd import weights as W
    dev = torch.device("cuda:0")
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    ts = build(args, dev, w, shared=False)
    print(json.dumps({"root": args.root, "token_rows": ts.T, "ms_per_step": [window(ts, args.steps) for _ in range(args.rounds)]}))


def parent_times(args, label):
    print(f"bench_shared_prompt: parent's replicated step ({label})", file=sys.stderr, flush=True)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--replicated-only", "--root", str(Path(args.parent).resolve()),
           "--steps", str(args.steps), "--rounds", str(args.rounds), "--prompts", str(args.prompts), "--group", str(args.group),
           "--model", args.model]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
    if done.returncode != 0:
        raise RuntimeError(f"parent ({label}): {done.stderr[-800:]}")
    return json.loads(done.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--parent", help="checkout of the parent commit (library built): its replicated step is timed too")
    ap.add_argument("--replicated-only", action="store_true", help="what the child of --parent runs")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    if args.replicated_only:
        replicated_only(args)
        return
    line = {"tool": "tools/bench_shared_prompt.py", "data": "synthetic", "stage": "lora", "rank": 32, "loss": "policy", "hip_graph": True,
            "prompts": args.prompts, "group": args.group, "L": 40, "steps": args.steps, "rounds": args.rounds}
    parent = []
    if args.parent:                          # before this process holds device memory of its own
        parent += parent_times(args, "before")
    sys.path.insert(0, str(ROOT))
    from bridgelang_amd import weights as W
    dev = torch.device("cuda:0")
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    sh = build(args, dev, w, shared=True)
    rep = build(args, dev, w, shared=False)
    line.update(model=dims.name, device=torch.cuda.get_device_name(0), token_rows={"shared": sh.T, "replicated": rep.T},
                images={"shared": sh.B, "replicated": rep.B}, row_ratio=round(rep.T / sh.T, 3),
                first_loss={"shared": round(sh.forward().item(), 6), "replicated": round(rep.forward().item(), 6)},
                device_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
    t = {"shared": [], "replicated": []}
    for _ in range(args.rounds):
        t["shared"].append(window(sh, args.steps))
        t["replicated"].append(window(rep, args.steps))
    del sh, rep, w
    torch.cuda.empty_cache()
    if args.parent:
        parent += parent_times(args, "after")
    arms = dict(t, **({"parent_replicated": parent} if parent else {}))
    spread = max(max(v) - min(v) for v in arms.values())
    base = min(parent) if parent else min(t["replicated"])
    line.update(ms_per_step=arms, spread_ms=round(spread, 3), replicated_over_shared=round(min(t["replicated"]) / min(t["shared"]), 3),
                baseline="parent_replicated" if parent else "replicated",
                shared_faster_than_baseline_by_more_than_the_spread=bool(min(t["shared"]) < base - spread))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
