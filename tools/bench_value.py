#!/usr/bin/env python
"""What a critic costs the policy-gradient step: the same step with and without the value head; one JSON line, also written
to profiles/bench_value.json. A record, nothing is gated.

  step      `TrainStep.step` at the benchmark's LoRA configuration (bench.py --mode train --stage lora: r = 32, B = 16,
            S = 296, graph replay): loss="policy" without a head and with `value=ValueLossConfig()` (one value per sequence,
            clipped) on one set of weights and adapters, each with its own ParamStore, `--steps` timed steps after one
            warm-up step, timed alternately `--rounds` times (the order swaps every round). Returns are synthetic; the old values are the step's own
            `values()` moved a little.
  kernels   the two value ops alone at that shape (B·S rows of 4096 bf16, one value row per sequence and, for comparison,
            8 per sequence), HIP events around `--reps` launches each (launch overhead included).

    python tools/bench_value.py
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from bench_policy_step import bench_inputs       # noqa: E402  (the benchmark's training batch)


def step_times(args, dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    lora = LoraAdapters(w, r=32)
    B, L = args.batch, 32 + 8
    ids, labels, pv, g = bench_inputs(B, L)
    kw = dict(lora=lora, max_grad_norm=float("inf"), weight_decay=0.01, loss="policy", policy=PolicyLossConfig())
    plain = TrainStep(w, "lora", B, L, **kw)
    crit = TrainStep(w, "lora", B, L, value=ValueLossConfig(), **kw)
    on = labels != -100
    for ts in (plain, crit):
        ts.set_batch(ids, None, pv, labels)
        ts.set_policy_batch(torch.zeros(B, L), torch.zeros(B, L))
    crit.set_value_batch(torch.zeros(B), torch.zeros(B))
    crit.forward()
    lp, v = crit.token_logprobs().cpu(), crit.values().cpu()
    noise = lambda: torch.where(on, 0.1 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    A = torch.where(on, torch.randn(B, L, generator=g), torch.zeros(B, L))
    for ts in (plain, crit):
        ts.set_policy_batch(A, lp + noise())
    crit.set_value_batch(v + torch.randn(B, generator=g), v + 0.1 * torch.randn(B, generator=g))
    runs = {"policy": [], "policy_value": []}
    order = [("policy", plain), ("policy_value", crit)]
    for rnd in range(args.rounds):
        for name, ts in (order if rnd % 2 == 0 else order[::-1]):      # neither is always the one that runs second
            ts.step(5e-4, graph=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss, _ = ts.step(5e-4, graph=True)
            torch.cuda.synchronize()
            runs[name].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
            assert np.isfinite(loss.item()), name
    spread = {k: round(max(v) - min(v), 3) for k, v in runs.items()}
    return {"model": dims.name, "stage": "lora", "rank": 32, "batch": B, "seq_len": plain.S, "steps": args.steps, "rounds": args.rounds,
            "hip_graph": True, **{f"{k}_ms_per_step": v for k, v in runs.items()}, "spread_ms": spread,
            "value_over_policy": round(min(runs["policy_value"]) / min(runs["policy"]), 4),
            "value_stats_last_step": {k: round(v.item(), 6) for k, v in crit.value_stats().items()}}


def op_times(args, dev):
    """Event-timed launches of the value head's forward and backward entry points on synthetic rows at the training shape."""
    from bridgelang_amd import train_ops as T
    from bridgelang_amd.training.value_loss import ValueLossConfig
    S, D, B = 296, 4096, args.batch
    rows = B * S
    g = torch.Generator().manual_seed(1)
    hn = torch.randn(rows, D, device=dev).to(torch.bfloat16)
    w = (torch.randn(D, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    b = torch.zeros(1, dtype=torch.bfloat16, device=dev)
    tgt = torch.full((B, S), -100, dtype=torch.int64)
    tgt[:, -9:-1] = torch.randint(31744, 32000, (B, 8), generator=g)
    tgt = tgt.view(-1).to(dev)
    Rt, vo = torch.randn(rows, generator=g).to(dev), (0.1 * torch.randn(rows, generator=g)).to(dev)
    vrows, stats, pstats = torch.zeros(rows, 4, device=dev), torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    dw, db, dh = torch.zeros(D, device=dev), torch.zeros(1, device=dev), torch.zeros(rows, D, dtype=torch.bfloat16, device=dev)
    out = {}
    for level in ("action", "token"):
        cfg = ValueLossConfig(level=level)
        idx = torch.zeros(T.value_index_slots(rows, level, S), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        plan = {"bl_value_head_f32": T.value_head(hn, tgt, w, b, Rt, vo, cfg, idx, cnt, vrows, stats, policy_stats=pstats, group_rows=S,
                                                  run=False),
                "bl_value_head_backward_f32": T.value_head_backward(hn, w, vrows, idx, cnt, dw, db, dh, cfg, group_rows=S, run=False)}
        for name, op in plan.items():
            for _ in range(3):
                op.run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                op.run()
            e1.record()
            torch.cuda.synchronize()
            out[f"{name}[{level}]"] = round(e0.elapsed_time(e1) / args.reps * 1e3, 2)
        out[f"value_rows[{level}]"] = int(cnt.item())
    return {"rows": rows, "dim": D, "reps": args.reps, "us_per_call_events": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--kernels-only", action="store_true", help="only the two value ops")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_value.json"), help="where the JSON line is written as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_value.py", "data": "synthetic", "device": torch.cuda.get_device_name(0)}
    line["value_ops"] = op_times(args, dev)
    if not args.kernels_only:
        torch.cuda.empty_cache()
        line["step"] = step_times(args, dev)
    text = json.dumps(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
