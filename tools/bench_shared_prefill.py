#!/usr/bin/env python
"""What one shared prefill per prompt gains (7B synthetic weights unless --model openvla-tiny); one JSON line. A record,
nothing is gated — but the tool writes NO record if a group engine's ids, weight pairs or logits differ from its replicated
twin's.

  leg a  per-launch time of the kernels alone, `--launches` back-to-back launches between two events, 32 heads, 16 rows
         of ONE prompt, prefix 288, pos = 290 (two generated rows present): bl_attention_decode_rope_shared_gq_bf16 at
         gq = 2, 4, 8 and bl_attention_decode_rope_bf16 on 16 replicated caches. The table DESIGN §6k chooses gq from.
  leg b  the action-sequence step (OpenVLAEngine, sample=True, L = 32 -> S = 288, 7 tokens, one captured graph) for
         (prompts, rows per prompt) in --cases: the group= engine beside today's engine of the same rows fed
         repeat_interleave'd inputs. Both live in one process and are timed alternately, `--rounds` times, `--steps`
         replays each; every round is reported, so the spread shows.

    python tools/bench_shared_prefill.py > profiles/bench_shared_prefill.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

L = 32
H, HD = 32, 128


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


def leg_a(dev, launches, rounds, rows=16, prefix=288, n_gen=2):
    from bridgelang_amd import ops
    from bridgelang_amd.engine import rope_tables
    cos, sin = rope_tables(HD, 2048, 10000.0, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(torch.bfloat16)
    pos, D = prefix + n_gen, H * HD
    qkv = rnd(rows, 3 * D)
    kp, vp = rnd(1, H, 320, HD), rnd(1, H, 320, HD)
    kg, vg = rnd(rows, H, 6, HD), rnd(rows, H, 6, HD)
    kr, vr = kp.repeat(rows, 1, 1, 1), vp.repeat(rows, 1, 1, 1)
    kr[:, :, prefix:pos], vr[:, :, prefix:pos] = kg[:, :, :n_gen], vg[:, :, :n_gen]
    o, o_ref = torch.zeros(rows, D, dtype=torch.bfloat16, device=dev), torch.zeros(rows, D, dtype=torch.bfloat16, device=dev)
    plans = {"decode_rope_replicated_caches": ops.attention_decode_rope(qkv, kr, vr, o_ref, cos, sin, B=rows, H=H, head_dim=HD, pos=pos, run=False)}
    for gq in (2, 4, 8):
        plans[f"decode_rope_shared_gq{gq}"] = ops.attention_decode_rope_shared(qkv, kp, vp, kg, vg, o, cos, sin, group=rows, H=H, head_dim=HD,
                                                                               prefix_len=prefix, pos=pos, gq=gq, run=False)
    plans["decode_rope_replicated_caches"].run()
    for k, op in plans.items():
        if k != "decode_rope_replicated_caches":
            op.run()
            torch.cuda.synchronize()
            if not torch.equal(o.view(torch.int16), o_ref.view(torch.int16)):
                raise SystemExit(f"{k}: output differs from the replicated kernel's: no record written")
    res = {k: [] for k in plans}
    for _ in range(rounds):
        for k, op in plans.items():
            res[k].append(round(_time(op, launches), 2))
    kv_bytes = dict(replicated=4.0 * rows * H * (pos + 1) * HD, shared=4.0 * H * (prefix + rows * (n_gen + 1)) * HD)
    return dict(rows=rows, heads=H, prefix_len=prefix, pos=pos, us_per_launch=res, kv_bytes_read=kv_bytes)


def leg_b(w, dev, steps, rounds, cases):
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.sampling import SamplingParams
    out = {}
    for P, G in cases:
        R = P * G
        g = torch.Generator().manual_seed(100 * P + G)
        ids = torch.randint(3, 31743, (P, L), generator=g)
        ids[:, 0], ids[:, -1] = 1, 29871
        ids, pv = ids.to(dev), (torch.rand(P, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        params = SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=np.arange(R, dtype=np.int64) * 7919 + 1)
        engines = {"group": OpenVLAEngine(w, R, L, sample=True, group=G), "replicated": OpenVLAEngine(w, R, L, sample=True)}
        engines["group"].set_inputs(ids, pv)
        engines["replicated"].set_inputs(ids.repeat_interleave(G, dim=0), pv.repeat_interleave(G, dim=0))
        for e in engines.values():
            e.set_sampling(params)
            e.capture()
            e.replay()
        torch.cuda.synchronize()
        a, b = engines["group"], engines["replicated"]
        if not (torch.equal(a.gen_ids, b.gen_ids) and torch.equal(a.gen_wt, b.gen_wt)
                and torch.equal(a.logits.view(torch.int32), b.logits.view(torch.int32))):
            raise SystemExit(f"(P, G) = ({P}, {G}): the group engine's ids, weight pairs or logits differ from the replicated "
                             f"engine's: no record written")
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
        out[f"{P}_prompts_x_{G}_rows"] = dict(ms_per_run=runs, rows=R, equal_ids_weights_logits=True,
                                              group_over_replicated=round(best["group"] / best["replicated"], 4),
                                              saved_ms=round(best["replicated"] - best["group"], 3),
                                              group_slower_than_replicated=bool(best["group"] > best["replicated"]))
        del engines, a, b
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--cases", default="1x4,1x8,1x16,2x8,4x4")
    ap.add_argument("--legs", default="ab", choices=["a", "b", "ab"])
    args = ap.parse_args()
    from bridgelang_amd import weights as W
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_shared_prefill.py", "data": "synthetic", "device": torch.cuda.get_device_name(0)}
    if "a" in args.legs:
        line["leg_a_kernels"] = dict(launches=args.launches, rounds=args.rounds, **leg_a(dev, args.launches, args.rounds))
    if "b" in args.legs:
        dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
        w = W.allocate(dims, dev).fill_synthetic(seed=0)
        cases = [tuple(int(x) for x in c.split("x")) for c in args.cases.split(",")]
        line["leg_b_engines"] = dict(model=dims.name, prompt_len=L, steps=args.steps, rounds=args.rounds,
                                     **leg_b(w, dev, args.steps, args.rounds, cases))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
