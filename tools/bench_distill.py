#!/usr/bin/env python
"""What a distillation step costs beside the policy-gradient step; one JSON line. A record, nothing is gated or tuned.

  kernels   the two new entry points and the policy loss's ranged pair at the training shape (B·S rows of 32 064 logits, 7
            labelled rows per sequence, the 256 action bins). Kernel times come from a kernel trace taken in a run of its
            own: with --trace this tool starts `rocprofv3 --kernel-trace --stats -- python tools/bench_distill.py
            --kernels-only` as a fresh child BEFORE it touches the GPU itself and reads the per-kernel statistics back. The
            same launches are also timed with HIP events (launch overhead included), in this process, profiler off.
  step      `TrainStep.step` at the benchmark's LoRA configuration (r = 32, S = 296, graph replay) with `--batch`
            sequences over the action-token range: loss="policy", loss="distill" (each kind), then loss="policy" again, each
            in a fresh child process (two 7B step objects of 32 sequences do not fit one device), `--rounds` windows of
            `--steps` timed steps after a warm-up step each.

    python tools/bench_distill.py --trace > profiles/bench_distill.json
"""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from bench_policy_step import bench_inputs       # noqa: E402  (the benchmark's training batch)

ACTIONS = (31744, 256)
KINDS = ("forward_kl", "reverse_kl", "jsd")


def action_labels(labels):
    """The benchmark's labels without the EOS position: the loss is over the action-token range."""
    return torch.where((labels >= ACTIONS[0]) & (labels < sum(ACTIONS)), labels, torch.full_like(labels, -100))


def teacher(B, L, g):
    return torch.softmax(2.0 * torch.randn(B, L, ACTIONS[1], generator=g), dim=-1)


def one_step(args, dev, name):
    """One loss's step in this process: `--rounds` windows of `--steps` timed steps after a warm-up step each."""
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    lora = LoraAdapters(w, r=32)
    B, L = args.batch, 32 + 8
    ids, labels, pv, g = bench_inputs(B, L)
    labels = action_labels(labels)
    on = labels != -100
    kw = dict(lora=lora, max_grad_norm=float("inf"), weight_decay=0.01)
    if name == "policy":
        ts = TrainStep(w, "lora", B, L, loss="policy", policy=PolicyLossConfig(token_range=ACTIONS), **kw)
        ts.set_batch(ids, None, pv, labels)
        ts.set_policy_batch(torch.where(on, torch.randn(B, L, generator=g), torch.zeros(B, L)),
                            torch.where(on, torch.full((B, L), -5.5), torch.zeros(B, L)))
    else:
        ts = TrainStep(w, "lora", B, L, loss="distill", distill=DistillLossConfig(kind=name, sft_coef=0.1, token_range=ACTIONS), **kw)
        ts.set_batch(ids, None, pv, labels)
        ts.set_distill_batch(teacher(B, L, g))
    ms = []
    for _ in range(args.rounds):
        ts.step(5e-4, graph=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, _ = ts.step(5e-4, graph=True)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
        assert np.isfinite(loss.item()), name
    stats = ts.policy_stats() if name == "policy" else ts.distill_stats()
    return {"model": dims.name, "seq_len": ts.S, "ms_per_step": ms, "stats_last_step": {k: round(v.item(), 6) for k, v in stats.items()}}


def step_times(args):
    """Each loss in a fresh child process, one after the other: two 7B step objects of 32 sequences do not fit one device, so
    the losses cannot alternate inside one process. The policy step is timed first and last, which shows the drift of the box
    over the whole measurement."""
    out, shape = {}, {}
    for label, name in (("policy", "policy"),) + tuple((k, k) for k in KINDS) + (("policy_again", "policy"),):
        print(f"bench_distill: timing {label}", file=sys.stderr, flush=True)
        done = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--one-step", name, "--steps", str(args.steps), "--rounds", str(args.rounds),
                               "--batch", str(args.batch), "--model", args.model], capture_output=True, text=True, timeout=900)
        if done.returncode != 0:
            raise RuntimeError(f"{label}: {done.stderr[-600:]}")
        r = json.loads(done.stdout.strip().splitlines()[-1])
        shape = {"model": r["model"], "seq_len": r["seq_len"]}
        out[f"{label}_ms_per_step"] = r["ms_per_step"]
        if name != "policy":
            out.setdefault("distill_stats_last_step", {})[name] = r["stats_last_step"]
    best = min(out["policy_ms_per_step"] + out["policy_again_ms_per_step"])
    return {**shape, "stage": "lora", "rank": 32, "batch": args.batch, "steps": args.steps, "hip_graph": True, "token_range": list(ACTIONS),
            "one_process_per_loss": True, **out, **{f"{k}_over_policy": round(min(out[f"{k}_ms_per_step"]) / best, 4) for k in KINDS}}


def loss_ops(args, dev):
    """The prepared launches at the training shape → {label: Op}."""
    from bridgelang_amd import train_ops as T
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    S, V, B = 296, 32064, args.batch
    rows = B * S
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, device=dev) * 2).to(torch.bfloat16).float()
    tgt = torch.full((B, S), -100, dtype=torch.int64)
    tgt[:, -9:-2] = torch.randint(ACTIONS[0], sum(ACTIONS), (B, 7), generator=g)
    tgt = tgt.view(-1).to(dev)
    A, q = torch.randn(rows, generator=g).to(dev), torch.full((rows,), -5.5, device=dev)
    teach = torch.softmax(2.0 * torch.randn(rows, ACTIONS[1], generator=g), dim=-1).to(dev)
    row_stats, stats = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    d_stats, d_st = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    dlogits = torch.zeros(rows, V, dtype=torch.bfloat16, device=dev)
    pcfg = PolicyLossConfig(token_range=ACTIONS)
    plan = {"bl_policy_loss_range_f32": T.policy_loss(logits, tgt, A, q, None, row_stats, stats, pcfg, run=False),
            "bl_policy_loss_backward_range_f32": T.policy_loss_backward(logits, tgt, row_stats, stats, dlogits, pcfg, run=False)}
    for kind in KINDS:
        cfg = DistillLossConfig(kind=kind, sft_coef=0.1, token_range=ACTIONS)
        plan[f"bl_distill_loss_f32[{kind}]"] = T.distill_loss(logits, tgt, teach, d_stats, d_st, cfg, run=False)
        plan[f"bl_distill_loss_backward_f32[{kind}]"] = T.distill_loss_backward(logits, tgt, teach, d_stats, d_st, dlogits, cfg, run=False)
    return plan, {"rows": rows, "n": V, "valid_rows": int((tgt != -100).sum()), "token_range": list(ACTIONS), "reps": args.reps}


def op_times(args, dev):
    plan, shape = loss_ops(args, dev)
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
    return {**shape, "us_per_call_events": out}


def kernel_trace(args):
    """A run of its own under the profiler (a fresh child; this process has not touched the GPU yet) → {kernel: statistics}.
    The child launches each op `reps` + 3 times in the order of `loss_ops`; forward_kl, reverse_kl and jsd share their kernels,
    so a kernel's line is over the three kinds."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()),
               "--kernels-only", "--reps", str(args.reps), "--batch", str(args.batch)]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if done.returncode != 0 or not files:
            return {"not_measured": f"rocprofv3 exit {done.returncode}, {len(files)} statistics file(s): {done.stderr[-300:]}"}
        out = {}
        for row in csv.DictReader(files[0].open()):
            name = row.get("Name", "")
            if "distill_" in name or "policy_" in name:
                short = name.split("(")[0].split("::")[-1].replace("void ", "")
                out[short] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        return out or {"not_measured": f"no distill / policy kernel in {files[0].name}"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--kernels-only", action="store_true", help="only the loss ops (what the traced child runs)")
    ap.add_argument("--trace", action="store_true", help="first take the kernel trace in a child process under rocprofv3")
    ap.add_argument("--one-step", choices=("policy",) + KINDS, help="time this loss's step alone (what a child of the step part runs)")
    args = ap.parse_args()
    if args.one_step:
        print(json.dumps(one_step(args, torch.device("cuda:0"), args.one_step)))
        return
    line = {"tool": "tools/bench_distill.py", "data": "synthetic"}
    if args.trace:
        line["kernel_trace"] = kernel_trace(args)
    if not args.kernels_only:                # before this process holds device memory of its own
        line["step"] = step_times(args)
    dev = torch.device("cuda:0")
    line["device"] = torch.cuda.get_device_name(0)
    line["loss_ops"] = op_times(args, dev)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
