#!/usr/bin/env python
"""What the policy-gradient loss costs beside cross-entropy in the training step, and how far the training forward's log π
is from the decode path's; one JSON line. A record, nothing is gated.

  step      `TrainStep.step` at the benchmark's training configuration (bench.py --mode train: full fine-tune, B = 32,
            S = 296, graph replay), loss="ce" against loss="policy" on one set of weights and one ParamStore, `--steps`
            timed steps after one warm-up step, the two timed alternately `--rounds` times.
  kernels   the loss-boundary ops alone at that shape (B·S rows of 32 064 logits, 8 labelled rows per sample), HIP events
            around `--reps` launches each (launch overhead included; `--kernels-only` runs just these, for a
            `rocprofv3 --kernel-trace --stats` pass that gives the kernels' own durations).
  mismatch  on the tiny model: |log ratio| between `score_actions` (decode path; equal to `sample_actions`' values bit for
            bit) and `token_logprobs()` (training forward) of the same sampled tokens: what a learner sees as ratio ≠ 1
            before any update.

    python tools/bench_policy_step.py > profiles/bench_policy_step.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def bench_inputs(B, L, seed=100):
    """The benchmark's training batch (bench.py::train_line): 32 prompt ids + 7 action ids + EOS, one 224 px frame."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 31000, (B, L), generator=g)
    ids[:, 0] = 1
    ids[:, -8:-1] = torch.randint(31744, 32000, (B, 7), generator=g)
    ids[:, -1] = 2
    labels = torch.full((B, L), -100)
    labels[:, -8:] = ids[:, -8:]
    pv = (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16)
    return ids, labels, pv, g


def step_times(args, dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    B, L = args.batch, 32 + 8
    ids, labels, pv, g = bench_inputs(B, L)
    ce = TrainStep(w, args.stage, B, L)
    pol = TrainStep(w, args.stage, B, L, store=ce.store, loss="policy", policy=PolicyLossConfig(entropy_coef=0.01, kl_coef=0.05))
    ce.set_batch(ids, None, pv, labels)
    pol.set_batch(ids, None, pv, labels)
    on = labels != -100
    A = torch.where(on, torch.randn(B, L, generator=g), torch.zeros(B, L))
    pol.set_policy_batch(A, torch.zeros(B, L), torch.zeros(B, L))
    pol.forward()
    lp = pol.token_logprobs().cpu()                      # behaviour / reference policy: this model, moved a little
    pol.set_policy_batch(A, lp + 0.1 * torch.randn(B, L, generator=g), lp + 0.1 * torch.randn(B, L, generator=g))
    runs = {"ce": [], "policy": []}
    for _ in range(args.rounds):
        for name, ts in (("ce", ce), ("policy", pol)):
            ts.step(2e-5, graph=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss, _ = ts.step(2e-5, graph=True)
            torch.cuda.synchronize()
            runs[name].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
            assert np.isfinite(loss.item()), name
    out = {"model": dims.name, "stage": args.stage, "batch": B, "seq_len": ce.S, "steps": args.steps, "hip_graph": True,
           **{f"{k}_ms_per_step": v for k, v in runs.items()},
           "policy_over_ce": round(min(runs["policy"]) / min(runs["ce"]), 4),
           "policy_stats_last_step": {k: round(v.item(), 6) for k, v in pol.policy_stats().items()}}
    return out


def op_times(args, dev):
    """Event-timed launches of the four loss-boundary ops on synthetic logits at the training shape."""
    from bridgelang_amd import ops, train_ops as T
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    S, V = 296, 32064
    rows = args.batch * S
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, device=dev) * 2).to(torch.bfloat16).float()
    tgt = torch.full((args.batch, S), -100, dtype=torch.int64)
    tgt[:, -9:-1] = torch.randint(31744, 32000, (args.batch, 8), generator=g)
    tgt = tgt.view(-1).to(dev)
    f = lambda: torch.randn(rows, generator=g).mul_(0.1).to(dev)
    A, q, ref = f(), f() - 10.0, f() - 10.0
    row_loss, mc = torch.zeros(rows, device=dev), torch.zeros(2, device=dev)
    row_stats, stats = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    dl = torch.zeros(rows, V, dtype=torch.bfloat16, device=dev)
    cfg = PolicyLossConfig(entropy_coef=0.01, kl_coef=0.05)
    plan = {"bl_cross_entropy_f32": ops.cross_entropy(logits, tgt, row_loss, mc, run=False),
            "bl_cross_entropy_backward_f32": T.cross_entropy_backward(logits, tgt, mc, dl, run=False),
            "bl_policy_loss_f32": T.policy_loss(logits, tgt, A, q, ref, row_stats, stats, cfg, run=False),
            "bl_policy_loss_backward_f32": T.policy_loss_backward(logits, tgt, row_stats, stats, dl, cfg, run=False)}
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
    return {"rows": rows, "n": V, "valid_rows": int((tgt != -100).sum()), "reps": args.reps, "us_per_call_events": out}


def mismatch(dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    from bridgelang_amd.sampling import SamplingParams
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import policy_batch
    from bridgelang_amd.training.step import TrainStep
    stats = {"robot": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    model = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=W.tiny_dims()).init_synthetic(seed=0)
    Bp, K, Lp, n, temp = 4, 4, 32, 7, 1.0
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, 31743, (Bp, Lp), generator=g)
    ids[:, 0], ids[:, -1] = 1, 29871
    pv = (torch.rand(Bp, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16)
    sp = SamplingParams(temperature=temp, seed=list(range(Bp)))
    _, tokens, lp = model.sample_actions(ids.to(dev), pv.to(dev), "robot", sp, num_samples=K)
    scored = model.score_actions(ids.to(dev), pv.to(dev), token_ids=tokens, sampling=sp)
    batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(Bp * K, n), scored.reshape(Bp * K, n), torch.zeros(Bp * K))
    ts = TrainStep(model.weights, "vla-train", Bp * K, batch["input_ids"].shape[1], loss="policy", policy=PolicyLossConfig(temperature=temp))
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv.repeat_interleave(K, 0), batch["labels"])
    ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
    ts.forward()
    on = batch["labels"] != -100
    d = (ts.token_logprobs().cpu().double()[on] - batch["old_logprobs"].double()[on]).abs()
    return {"model": "openvla-tiny", "tokens": int(on.sum()), "temperature": temp, "score_equals_sample_bitwise": bool(np.array_equal(scored, lp)),
            "abs_log_ratio_mean": float(d.mean()), "abs_log_ratio_max": float(d.max()), "mean_ratio": round(ts.policy_stats()["ratio"].item(), 6)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--stage", default="vla-full-train", choices=["vla-full-train", "vla-train"])
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--kernels-only", action="store_true", help="only the loss-boundary ops (for a kernel-trace pass)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_policy_step.py", "data": "synthetic", "device": torch.cuda.get_device_name(0)}
    line["loss_ops"] = op_times(args, dev)
    if not args.kernels_only:
        torch.cuda.empty_cache()
        line["decode_vs_training"] = mismatch(dev)
        torch.cuda.empty_cache()
        line["step"] = step_times(args, dev)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
