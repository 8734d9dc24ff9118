#!/usr/bin/env python
"""What beam search costs (7B synthetic weights unless --model openvla-tiny); one JSON line. A record, nothing is gated.

  leg a  per-launch time of the two kernels alone, `--launches` back-to-back launches between two events:
         bl_beam_step_f32 at W = 4 and W = 16 over one prompt's rows of 32 064 logits, the full vocabulary and the 256
         action tokens; bl_beam_reorder_kv_bf16 at W = 4 and W = 16 over the 64 caches of the 7B model (32 heads,
         head_dim 128, cache_len 320) moving 1 and 5 generated rows (the first and the last reorder of an action), with
         the bytes it moves and the GB/s that makes.
  leg b  the action-sequence step (OpenVLAEngine, L = 32 -> S = 288, 7 tokens, one captured graph) of ONE prompt with
         beams = 4 and beams = 16 beside the greedy engine at 4 and 16 rows, the same rows without a beam op. The engines
         of a row count live in one process and are timed alternately, `--rounds` times, `--steps` replays each.

    python tools/bench_beam.py > profiles/bench_beam.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

L, V = 32, 32064
ACTION_RANGE = (31744, 256)


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
    return e0.elapsed_time(e1) / launches * 1e3


def leg_a(dev, launches, rounds):
    from bridgelang_amd import ops
    from bridgelang_amd.beam import start_scores
    plans, moved = {}, {}
    for W in (4, 16):
        g = torch.Generator().manual_seed(W)
        logits = (torch.randn(W, V, generator=g) * 3).to(torch.bfloat16).float().to(dev)
        scores = (-torch.rand(W, generator=g) * 8).to(dev)
        out = (torch.zeros(W, dtype=torch.int64, device=dev), torch.zeros(W, dtype=torch.int32, device=dev),
               torch.zeros(W, 2, dtype=torch.int64, device=dev), torch.zeros(W, device=dev))
        plans[f"beam_step_W{W}_full_vocab"] = ops.beam_step(logits, W, scores, *out, run=False)
        plans[f"beam_step_W{W}_action_tokens"] = ops.beam_step(logits, W, scores, *out, run=False, vocab=ACTION_RANGE)
        plans[f"beam_step_W{W}_full_vocab_step0"] = ops.beam_step(logits[:1].expand(W, V).contiguous(), W,
                                                                  torch.from_numpy(start_scores(W)).to(dev), *out, run=False)
        caches = [torch.zeros(W, 32, 320, 128, dtype=torch.bfloat16, device=dev) for _ in range(64)]
        table = ops.cache_table(caches)
        parents = torch.randint(0, W, (W,), generator=g).to(torch.int32).to(dev)
        for n_rows in (1, 5):
            name = f"beam_reorder_kv_W{W}_64caches_{n_rows}rows"
            plans[name] = ops.beam_reorder_kv(table, caches, W, parents, 288, n_rows, run=False)
            moved[name] = plans[name].bytes
    res = {k: [] for k in plans}
    for _ in range(rounds):
        for k, op in plans.items():
            res[k].append(round(_time(op, launches), 2))
    return dict(us_per_launch=res, reorder_bytes_read_and_written=moved,
                reorder_gb_per_s={k: round(b / (min(res[k]) * 1e-6) / 1e9, 1) for k, b in moved.items()})


def leg_b(w, dev, steps, rounds, widths):
    from bridgelang_amd.engine import OpenVLAEngine
    out = {}
    for W in widths:
        g = torch.Generator().manual_seed(W)
        ids = torch.randint(3, 31743, (1, L), generator=g)
        ids[:, 0], ids[:, -1] = 1, 29871
        ids, pv = ids.to(dev), (torch.rand(1, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        engines = {"greedy_rows": OpenVLAEngine(w, W, L), "beams": OpenVLAEngine(w, W, L, beams=W),
                   "beams_action_tokens": OpenVLAEngine(w, W, L, beams=W, vocab_range=ACTION_RANGE)}
        engines["greedy_rows"].set_inputs(ids.repeat(W, 1), pv.repeat(W, 1, 1, 1))
        for k, e in engines.items():
            if k != "greedy_rows":
                e.set_inputs(ids, pv)
            e.capture()
        torch.cuda.synchronize()
        runs = {k: [] for k in engines}
        for _ in range(rounds):
            for k, e in engines.items():
                for _ in range(3):
                    e.replay()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    e.replay()
                torch.cuda.synchronize()
                runs[k].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
        best = {k: min(v) for k, v in runs.items()}
        top = engines["beams"].result().ids[0]
        out[f"one_prompt_{W}_beams"] = dict(ms_per_action=runs, rows=W, beam_steps_per_action=7, reorders_per_action=5,
                                            best_beam_is_the_greedy_chain=bool(torch.equal(top, engines["greedy_rows"].gen_ids[:, 0])),
                                            beams_over_greedy_rows=round(best["beams"] / best["greedy_rows"], 4),
                                            beams_extra_ms=round(best["beams"] - best["greedy_rows"], 3),
                                            action_tokens_over_greedy_rows=round(best["beams_action_tokens"] / best["greedy_rows"], 4),
                                            action_tokens_extra_ms=round(best["beams_action_tokens"] - best["greedy_rows"], 3))
        del engines
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--widths", default="4,16")
    ap.add_argument("--legs", default="ab", choices=["a", "b", "ab"])
    args = ap.parse_args()
    from bridgelang_amd import weights as W
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_beam.py", "data": "synthetic", "device": torch.cuda.get_device_name(0)}
    if "a" in args.legs:
        line["leg_a_kernels"] = dict(launches=args.launches, rounds=args.rounds, **leg_a(dev, args.launches, args.rounds))
    if "b" in args.legs:
        dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
        w = W.allocate(dims, dev).fill_synthetic(seed=0)
        line["leg_b_action"] = dict(model=dims.name, prompt_len=L, steps=args.steps, rounds=args.rounds,
                                    **leg_b(w, dev, args.steps, args.rounds, [int(b) for b in args.widths.split(",")]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
