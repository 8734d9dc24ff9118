#!/usr/bin/env python
"""What seeded sampling costs (7B synthetic weights unless --model openvla-tiny); one JSON line. A record, nothing is gated.

  leg a  per-launch time of bl_sample_f32 (T = 1, k = 50, p = 0.95, a seed per row) against bl_argmax_f32 on the same
         bf16-rounded randn·3 logits [rows, 32064], rows = 16 and 96: `--launches` back-to-back launches between two events.
  leg b  the `bench.py --pipeline 7` step: StaggeredDecodePipeline at B = 16, L = 32, captured graphs, `--steps` timed steps,
         greedy against sample=True with every sequence at that configuration (and sample=True with every sequence at
         temperature 0: the early-out path). Both pipelines live in one process and are timed alternately, `--rounds` times.
  leg c  the restricted policy (token range 31744 + 256, the action bins) against the full-row entry points ON THE SAME
         LOGITS, timed alternately `--rounds` times: bl_sample_range_f32 / bl_score_range_f32 beside bl_sample_f32 /
         bl_score_f32 (temperature only, rows = 16 and 96), and bl_policy_loss_range_f32 / its backward beside
         bl_policy_loss_f32 / its backward on [2304, 32064] logits (8 sequences of 288 positions) with every row labelled
         and with 7 labelled rows per sequence (the training shape: the rest of dlogits is the zero fill).

    python tools/bench_sample.py > profiles/bench_sample.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

B, L, V = 16, 32, 32064


def leg_a(dev, launches):
    from bridgelang_amd import ops
    out = {}
    for rows in (16, 96):
        g = torch.Generator().manual_seed(rows)
        logits = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16).float().to(dev)
        ids, wt = torch.zeros(rows, dtype=torch.int64, device=dev), torch.zeros(rows, 2, dtype=torch.int64, device=dev)
        T, k = torch.ones(rows, device=dev), torch.full((rows,), 50, dtype=torch.int32, device=dev)
        p, seed = torch.full((rows,), 0.95, device=dev), torch.arange(rows, dtype=torch.int64, device=dev)
        plans = {"bl_argmax_f32": ops.argmax(logits, ids, run=False),
                 "bl_sample_f32": ops.sample(logits, T, k, p, seed, 0, ids, wt, run=False),
                 "bl_sample_f32_top_p_only": ops.sample(logits, T, torch.zeros_like(k), p, seed, 0, ids, wt, run=False),
                 "bl_sample_f32_temperature_0": ops.sample(logits, torch.zeros_like(T), k, p, seed, 0, ids, wt, run=False)}
        res = {}
        for name, op in plans.items():
            for _ in range(10):
                op.run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                op.run()
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(e0.elapsed_time(e1) / launches * 1e3, 2)
        out[f"rows_{rows}_us_per_launch"] = res
    return out


def _time(op, launches):
    for _ in range(10):
        op.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        op.run()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / launches * 1e3, 2)


def _alternate(plans, launches, rounds):
    """Every plan `rounds` times, interleaved → {name: [µs per launch, one per round]}."""
    res = {name: [] for name in plans}
    for _ in range(rounds):
        for name, op in plans.items():
            res[name].append(_time(op, launches))
    return res


def leg_c(dev, launches, rounds):
    from bridgelang_amd import ops, train_ops
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    rng = (V - 320, 256)
    out = {"token_range": list(rng)}
    for rows in (16, 96):
        g = torch.Generator().manual_seed(rows)
        logits = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16).float().to(dev)
        ids, wt = torch.zeros(rows, dtype=torch.int64, device=dev), torch.zeros(rows, 2, dtype=torch.int64, device=dev)
        tok = torch.full((rows,), rng[0] + 5, dtype=torch.int64, device=dev)
        T, k = torch.ones(rows, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        p, seed = torch.ones(rows, device=dev), torch.arange(rows, dtype=torch.int64, device=dev)
        bins = torch.zeros(rows, rng[1], dtype=torch.int32, device=dev)
        plans = {"bl_sample_f32": ops.sample(logits, T, k, p, seed, 0, ids, wt, run=False),
                 "bl_sample_range_f32": ops.sample(logits, T, k, p, seed, 0, ids, wt, run=False, vocab=rng),
                 "bl_score_f32_with_bins": ops.score(logits, T, k, p, tok, wt, rng[0], bins, run=False),
                 "bl_score_range_f32_with_bins": ops.score(logits, T, k, p, tok, wt, rng[0], bins, run=False, vocab=rng)}
        out[f"sample_rows_{rows}_us_per_launch"] = _alternate(plans, launches, rounds)
    seqs, S = 8, 288
    rows = seqs * S
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(rows, V, generator=g) * 2).to(torch.bfloat16).float().to(dev)
    A, q = torch.randn(rows, generator=g).to(dev), torch.full((rows,), -5.0, device=dev)
    row_stats, stats = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev)
    dl = torch.zeros(rows, V, dtype=torch.bfloat16, device=dev)
    every = rng[0] + torch.randint(0, rng[1], (rows,), generator=g)
    few = torch.full((seqs, S), -100, dtype=torch.int64)
    few[:, S - 9:S - 2] = every.view(seqs, S)[:, S - 9:S - 2]
    for name, tgt in (("every_row_labelled", every.to(dev)), ("7_rows_per_sequence_labelled", few.view(-1).to(dev))):
        plans = {}
        for tag, cfg in (("", PolicyLossConfig(entropy_coef=0.01)), ("_range", PolicyLossConfig(entropy_coef=0.01, token_range=rng))):
            plans[f"bl_policy_loss{tag}_f32"] = train_ops.policy_loss(logits, tgt, A, q, None, row_stats, stats, cfg, run=False)
            plans[f"bl_policy_loss_backward{tag}_f32"] = train_ops.policy_loss_backward(logits, tgt, row_stats, stats, dl, cfg, run=False)
        for op in plans.values():                               # the backward plans read what a forward of their own kind saved
            op.run()
        out[f"policy_{name}_us_per_launch"] = dict(rows=rows, **_alternate(plans, max(20, launches // 4), rounds))
    return out


def leg_b(w, dev, steps, rounds):
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    from bridgelang_amd.sampling import SamplingParams
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, 31743, (B, L), generator=g)
    ids[:, 0], ids[:, -1] = 1, 29871
    ids, pv = ids.to(dev), (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    pipes = {"greedy": StaggeredDecodePipeline(w, B, L), "sampled": StaggeredDecodePipeline(w, B, L, sample=True)}
    for name, pipe in pipes.items():
        for e in pipe.engines:
            e.set_inputs(ids, pv)
        pipe.capture()
    settings = {"greedy": None, "sampled": SamplingParams(1.0, 50, 0.95, seed=list(range(B))),
                "sampled_temperature_0": SamplingParams(temperature=0.0)}
    runs = {k: [] for k in settings}
    for _ in range(rounds):
        for name, sp in settings.items():
            pipe = pipes["greedy" if sp is None else "sampled"]
            if sp is not None:
                for e in pipe.engines:
                    e.set_sampling(sp)
            for _ in range(pipe.slots):
                pipe.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                pipe.step()
            torch.cuda.synchronize()
            runs[name].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
    out = {f"{k}_ms_per_step": v for k, v in runs.items()}
    out["sampled_over_greedy"] = round(min(runs["sampled"]) / min(runs["greedy"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--legs", default="abc", choices=["a", "b", "c", "ab", "ac", "bc", "abc"])
    args = ap.parse_args()
    from bridgelang_amd import weights as W
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_sample.py", "data": "synthetic", "device": torch.cuda.get_device_name(0),
            "sampled_configuration": {"temperature": 1.0, "top_k": 50, "top_p": 0.95}}
    if "a" in args.legs:
        line["leg_a_kernel"] = dict(launches=args.launches, n=V, **leg_a(dev, args.launches))
    if "c" in args.legs:
        line["leg_c_token_range"] = dict(launches=args.launches, rounds=args.rounds, n=V, **leg_c(dev, args.launches, args.rounds))
    if "b" in args.legs:
        dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
        w = W.allocate(dims, dev).fill_synthetic(seed=0)
        line["leg_b_pipeline_step"] = dict(model=dims.name, batch=B, prompt_len=L, steps=args.steps, **leg_b(w, dev, args.steps, args.rounds))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
