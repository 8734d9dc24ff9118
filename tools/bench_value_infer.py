#!/usr/bin/env python
"""What the critic costs at inference (7B synthetic weights unless --model openvla-tiny): the action-sequence step
`predict_action` replays, without a value head, with value="action" (one bl_value_predict_f32 per action) and with
value="token" (one per generated token). One JSON line, also written to profiles/bench_value_infer.json. A record, nothing
is gated.

  step    OpenVLAEngine, L = 32 (S = 288), 7 tokens, one captured graph per configuration, at B = 1 and B = 16. The three
          engines of a batch size live in one process over one set of weights and are timed alternately, `--rounds` times,
          `--steps` replays each; the order is reversed every round, so none is always the one that runs after another.
          Reported: every round's ms per action batch and the per-configuration range.
  kernel  bl_value_predict_f32 alone on B rows of 4096 bf16 at the prefill's row stride, HIP events around `--launches`
          launches (launch overhead included).

What it replaces: without the op, V(s) of a rollout batch is a learner forward over the rebuilt training batch (DESIGN §6f's
`forward()` + `values()`, about 120 ms per 32 states at 7B).

    python tools/bench_value_infer.py
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

L = 32
CONFIGS = (("no_head", None), ("action", "action"), ("token", "token"))


def step_times(w, vh, dev, steps, rounds, batches):
    from bridgelang_amd.engine import OpenVLAEngine
    out = {}
    for B in batches:
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(3, 31743, (B, L), generator=g)
        ids[:, 0], ids[:, -1] = 1, 29871
        ids, pv = ids.to(dev), (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        engines = {name: OpenVLAEngine(w, B, L, **({} if level is None else dict(value=level, value_head=vh))) for name, level in CONFIGS}
        for e in engines.values():
            e.set_inputs(ids, pv)
            e.capture()
        torch.cuda.synchronize()
        off = engines["no_head"]
        same = all(torch.equal(e.gen_ids, off.gen_ids) and torch.equal(e.logits, off.logits) for e in engines.values())
        launches = {k: sum(op.name == "bl_value_predict_f32" for op in e.all_ops()) for k, e in engines.items()}
        runs = {k: [] for k in engines}
        order = list(engines.items())
        for rnd in range(rounds):
            for k, e in (order if rnd % 2 == 0 else order[::-1]):
                for _ in range(3):
                    e.replay()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    e.replay()
                torch.cuda.synchronize()
                runs[k].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
        best = {k: min(v) for k, v in runs.items()}
        out[f"batch_{B}"] = dict(ms_per_action_batch=runs, range_ms={k: [min(v), max(v)] for k, v in runs.items()},
                                 value_launches_per_action_batch=launches, ids_and_logits_equal_with_head=same,
                                 action_extra_ms=round(best["action"] - best["no_head"], 3),
                                 token_extra_ms=round(best["token"] - best["no_head"], 3),
                                 values_action=[round(float(v), 5) for v in engines["action"].value_result()[:2]])
        del engines
        torch.cuda.empty_cache()
    return out


def kernel_times(w, vh, dev, launches, batches):
    from bridgelang_amd import train_ops as T
    D, S = w.dims.llm_dim, w.dims.n_patches + L
    out = {}
    for B in batches:
        x = torch.randn(B, S, D, device=dev).to(torch.bfloat16)
        vals = torch.zeros(B, dtype=torch.float32, device=dev)
        op = T.value_predict(x[:, S - 1, :], w.norm, w.dims.rms_eps, vh.weight, vh.bias, vals, run=False)
        for _ in range(10):
            op.run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            op.run()
        e1.record()
        torch.cuda.synchronize()
        out[f"rows_{B}"] = round(e0.elapsed_time(e1) / launches * 1e3, 2)
    return {"dim": D, "row_stride": S * D, "launches": launches, "us_per_launch_events": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_value_infer.json"), help="where the JSON line is written as well")
    args = ap.parse_args()
    from bridgelang_amd import weights as W
    from bridgelang_amd.training.value_head import ValueHead
    dev = torch.device("cuda:0")
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    w = W.allocate(dims, dev).fill_synthetic(seed=0)
    vh = ValueHead(dims.llm_dim, dev, init_std=0.02, seed=0)
    batches = [int(b) for b in args.batches.split(",")]
    line = {"tool": "tools/bench_value_infer.py", "data": "synthetic", "device": torch.cuda.get_device_name(0), "model": dims.name,
            "prompt_len": L, "steps": args.steps, "rounds": args.rounds, "hip_graph": True,
            "kernel": kernel_times(w, vh, dev, args.launches, batches),
            "step": step_times(w, vh, dev, args.steps, args.rounds, batches),
            "replaces": "a learner forward over the rebuilt rollout batch, then values() (DESIGN 6f)"}
    text = json.dumps(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
