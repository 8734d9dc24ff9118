#!/usr/bin/env python
"""What scoring given actions costs beside sampling them (7B synthetic weights unless --model openvla-tiny); one JSON
line. A record, nothing is gated: the score plan is the sampling plan with bl_score_f32 where that has bl_sample_f32.

  `sample_actions` against `score_actions` (token_ids = the sampled tokens; with and without return_bins) on one model
  object at B = 16 (`--batch`), L = 32, T = 1, k = 50, p = 0.95: wall time per call, host work included, `--calls` calls
  after two warm-up calls, the legs timed alternately `--rounds` times. A greedy `predict_action` rides along: at --batch 1
  it is the latency of one action, where the per-call host work of the front end shows most.

    python tools/bench_score.py > profiles/bench_score.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

L = 32


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    B = args.batch
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    from bridgelang_amd.sampling import SamplingParams
    dev = torch.device("cuda:0")
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    stats = {"robot": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    model = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=dims).init_synthetic(seed=0)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, 31743, (B, L), generator=g)
    ids[:, 0], ids[:, -1] = 1, 29871
    ids, pv = ids.to(dev), (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    sp = SamplingParams(1.0, 50, 0.95, seed=list(range(B)))
    tokens = model.sample_actions(ids, pv, "robot", sp)[1]
    legs = {"predict_action": lambda: model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key="robot"),
            "sample_actions": lambda: model.sample_actions(ids, pv, "robot", sp),
            "score_actions": lambda: model.score_actions(ids, pv, token_ids=tokens, sampling=sp),
            "score_actions_return_bins": lambda: model.score_actions(ids, pv, token_ids=tokens, sampling=sp, return_bins=True)}
    runs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, call in legs.items():
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            runs[name].append(round((time.perf_counter() - t0) / args.calls * 1e3, 3))
    line = {"tool": "tools/bench_score.py", "data": "synthetic", "device": torch.cuda.get_device_name(0), "model": dims.name,
            "batch": B, "prompt_len": L, "calls": args.calls, "configuration": {"temperature": 1.0, "top_k": 50, "top_p": 0.95},
            **{f"{k}_ms_per_call": v for k, v in runs.items()},
            "score_over_sample": round(min(runs["score_actions"]) / min(runs["sample_actions"]), 4)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
