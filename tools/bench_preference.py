#!/usr/bin/env python
"""What a preference-pair step costs beside the cross-entropy and the policy-gradient step; one JSON line. A record,
nothing is gated.

  step      `TrainStep.step` at the benchmark's LoRA configuration (bench.py --mode train --stage lora: r = 32, B = 16,
            S = 296, graph replay): loss="ce", loss="policy" and loss="preference" on one set of weights, one set of
            adapters and one ParamStore, `--steps` timed steps after one warm-up step, timed alternately `--rounds` times.
            The preference batch is 8 pairs (sequence 2k chosen, 2k + 1 rejected) with the step's own `token_logprobs()`,
            moved a little, as the reference.
  kernels   the forward loss op alone at that shape (B·S rows of 32 064 logits, 8 labelled rows per sequence), HIP events
            around `--reps` launches each (launch overhead included).

    python tools/bench_preference.py > profiles/bench_preference.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bench_policy_step import bench_inputs       # noqa: E402  (the benchmark's training batch)


def step_times(args, dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    lora = LoraAdapters(w, r=32)
    B, L = args.batch, 32 + 8
    ids, labels, pv, g = bench_inputs(B, L)
    kw = dict(lora=lora, max_grad_norm=float("inf"), weight_decay=0.01)
    ce = TrainStep(w, "lora", B, L, **kw)
    pol = TrainStep(w, "lora", B, L, store=ce.store, loss="policy", policy=PolicyLossConfig(), **kw)
    pref = TrainStep(w, "lora", B, L, store=ce.store, loss="preference", preference=PreferenceLossConfig(beta=0.1, sft_coef=0.1), **kw)
    for ts in (ce, pol, pref):
        ts.set_batch(ids, None, pv, labels)
    on = labels != -100
    pref.forward()
    lp = pref.token_logprobs().cpu()
    noise = lambda: torch.where(on, 0.1 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    pol.set_policy_batch(torch.where(on, torch.randn(B, L, generator=g), torch.zeros(B, L)), lp + noise())
    pref.set_preference_batch([(b // 2 + 1) * (1 if b % 2 == 0 else -1) for b in range(B)], lp + noise())
    runs = {"ce": [], "policy": [], "preference": []}
    for _ in range(args.rounds):
        for name, ts in (("ce", ce), ("policy", pol), ("preference", pref)):
            ts.step(5e-4, graph=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss, _ = ts.step(5e-4, graph=True)
            torch.cuda.synchronize()
            runs[name].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
            assert np.isfinite(loss.item()), name
    return {"model": dims.name, "stage": "lora", "rank": 32, "batch": B, "pairs": B // 2, "seq_len": ce.S, "steps": args.steps,
            "hip_graph": True, **{f"{k}_ms_per_step": v for k, v in runs.items()},
            "preference_over_ce": round(min(runs["preference"]) / min(runs["ce"]), 4),
            "preference_over_policy": round(min(runs["preference"]) / min(runs["policy"]), 4),
            "preference_stats_last_step": {k: round(v.item(), 6) for k, v in pref.preference_stats().items()}}


def op_times(args, dev):
    """Event-timed launches of the three forward loss ops on synthetic logits at the training shape."""
    from bridgelang_amd import ops, train_ops as T
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    S, V, B = 296, 32064, args.batch
    rows = B * S
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, device=dev) * 2).to(torch.bfloat16).float()
    tgt = torch.full((B, S), -100, dtype=torch.int64)
    tgt[:, -9:-1] = torch.randint(31744, 32000, (B, 8), generator=g)
    tgt = tgt.view(-1).to(dev)
    f = lambda: torch.randn(rows, generator=g).mul_(0.1).to(dev)
    A, q, ref = f(), f() - 10.0, f() - 10.0
    pair = torch.tensor([(b // 2 + 1) * (1 if b % 2 == 0 else -1) for b in range(B)], dtype=torch.int32, device=dev)
    n_pairs = torch.tensor([B // 2], dtype=torch.int32, device=dev)
    row_loss, mc = torch.zeros(rows, device=dev), torch.zeros(2, device=dev)
    row_stats, stats = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    pair_stats, seq_stats = torch.zeros(B // 2, 4, device=dev), torch.zeros(B, 4, device=dev)
    plan = {"bl_cross_entropy_f32": ops.cross_entropy(logits, tgt, row_loss, mc, run=False),
            "bl_policy_loss_f32": T.policy_loss(logits, tgt, A, q, None, row_stats, stats, PolicyLossConfig(), run=False),
            "bl_preference_loss_f32": T.preference_loss(logits, tgt, pair, ref, row_stats, stats, pair_stats, seq_stats,
                                                        PreferenceLossConfig(), group_rows=S, n_pairs=n_pairs, run=False)}
    out = {}
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
        out[name] = round(e0.elapsed_time(e1) / args.reps * 1e3, 2)
    return {"rows": rows, "n": V, "valid_rows": int((tgt != -100).sum()), "pairs": B // 2, "reps": args.reps, "us_per_call_events": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--kernels-only", action="store_true", help="only the forward loss ops")
    args = ap.parse_args()
    if args.batch < 2 or args.batch % 2:
        ap.error("--batch: an even number of sequences (chosen, rejected)")
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_preference.py", "data": "synthetic", "device": torch.cuda.get_device_name(0)}
    line["loss_ops"] = op_times(args, dev)
    if not args.kernels_only:
        torch.cuda.empty_cache()
        line["step"] = step_times(args, dev)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
