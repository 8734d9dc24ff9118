#!/usr/bin/env python
"""Mixed-length serving through the staggered decode pipeline, measured (7B synthetic weights, B = 16); one JSON line.

  leg a  the cost of the padded plan itself: StaggeredDecodePipeline(padded=True) at L = 32 with all-ones masks against
         the un-padded pipeline at L = 32, same process, same inputs, captured graphs, `--steps` timed steps each.
  leg b  one fixed trace of `--requests` requests whose prompt lengths (empty token included) are uniform in 18…32,
         all queued at once, served by OpenVLAServer(pipeline_batch=16) twice: with pad_to=32 (ONE padded pipeline) and
         with pad_to=None (per-length bucketing: batches close at every change of length, a pipeline per length, at most
         `max_pipelines` = 2 kept — the server as it was before pad_to). Seconds from the first request queued to the last
         answer; each server first answers one untimed full-length batch, so the padded pipeline's one-off build and capture
         is outside its timed region (the bucketed server keeps building pipelines inside it: that is its behaviour).

    python tools/bench_serve_mixed.py > profiles/bench_serve_mixed.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

B, L, LO = 16, 32, 18


def make_inputs(n_rows, length, seed, dev=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 31743, (n_rows, length), generator=g)
    ids[:, 0] = 1
    pv = (torch.rand(n_rows, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16)
    return (ids, pv) if dev is None else (ids.to(dev), pv.to(dev))


def time_pipeline(pipe, steps):
    pipe.capture()
    for _ in range(max(3, pipe.slots)):      # also fills the pipeline
        pipe.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"ms_per_step": round(dt / steps * 1e3, 3), "action_seqs_per_s": round(B * steps / dt, 2)}


def leg_a(w, dev, steps):
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    ids, pv = make_inputs(B, L, 0, dev)
    ids[:, -1] = 29871
    out = {}
    for name, padded in (("unpadded", False), ("padded_all_ones", True)):
        pipe = StaggeredDecodePipeline(w, B, L, padded=padded)
        for e in pipe.engines:
            if padded:
                e.set_padded_inputs(ids, pv, torch.ones_like(ids))
            else:
                e.set_inputs(ids, pv)
        out[name] = time_pipeline(pipe, steps)
        del pipe
        torch.cuda.empty_cache()
    out["padded_over_unpadded_ms"] = round(out["padded_all_ones"]["ms_per_step"] / out["unpadded"]["ms_per_step"], 4)
    return out


def serve_trace(vla, lengths, pad_to):
    """Queue the whole trace at once (requests carry ids WITHOUT the empty token, as the processor hands them over)."""
    from bridgelang_amd import serve
    server = serve.OpenVLAServer(vla, None, pipeline_batch=B, max_wait_ms=2.0, pad_to=pad_to)

    def run(lens, seed):
        reqs = []
        for i, n in enumerate(lens):
            ids, pv = make_inputs(1, n - 1, seed + i)
            reqs.append(serve._Request(ids, pv, "synthetic"))
        t0 = time.perf_counter()
        for r in reqs:
            server._q.put(r)
        for r in reqs:
            r.future.result(timeout=3000)
        return time.perf_counter() - t0

    try:
        run([L] * B, 10_000)                  # untimed: builds and captures the first pipeline
        built0, n0 = server.pipelines_built, len(server.batch_sizes)
        dt = run(lengths, 20_000)
        sizes = server.batch_sizes[n0:]
        return {"seconds": round(dt, 3), "action_seqs_per_s": round(len(lengths) / dt, 2), "gpu_batches": len(sizes),
                "mean_batch": round(sum(sizes) / len(sizes), 2),
                "batches_mixing_lengths": sum(len(set(b)) > 1 for b in server.batch_lengths[n0:]),
                "pipelines_built_in_timed_region": server.pipelines_built - built0}
    finally:
        server.close()
        del server
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--legs", default="ab", choices=["a", "b", "ab"])
    args = ap.parse_args()
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    dev = torch.device("cuda:0")
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
    stats = {"synthetic": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    vla = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=dims).init_synthetic(seed=0)
    line = {"tool": "tools/bench_serve_mixed.py", "model": dims.name, "batch": B, "pad_to": L, "data": "synthetic",
            "device": torch.cuda.get_device_name(0)}
    note = lambda msg: print(f"[bench_serve_mixed] {msg}", file=sys.stderr, flush=True)
    if "a" in args.legs:
        note("leg a: padded vs un-padded pipeline")
        line["leg_a_padded_plan_cost"] = dict(steps=args.steps, prompt_len=L, **leg_a(vla.weights, dev, args.steps))
    if "b" in args.legs:
        g = torch.Generator().manual_seed(2024)
        lengths = torch.randint(LO, L + 1, (args.requests,), generator=g).tolist()
        note("leg b: the trace through the padded pipeline")
        padded = serve_trace(vla, lengths, L)
        note("leg b: the trace through per-length bucketing")
        line["leg_b_mixed_trace"] = {"requests": args.requests, "lengths": lengths, "padded_pipeline": padded,
                                     "per_length_bucketing": serve_trace(vla, lengths, None)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
