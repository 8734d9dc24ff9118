#!/usr/bin/env python
"""What the attention taps cost (7B synthetic weights unless --model openvla-tiny); one JSON line. A record, nothing is gated.

  leg a  per-launch time of bl_attention_probs_f32 alone, probs + 4 segments, un-rotated q from fused qkv rows, at
         (B, H, Sq, Skv) = (16, 32, 1, 295) — one generation tap — and (1, 32, 288, 288) causal — one attention_maps layer:
         `--launches` back-to-back launches between two events, with the K bytes it reads and the GB/s that makes.
  leg b  the action-sequence step `predict_action` replays (OpenVLAEngine, L = 32 → S = 288, 7 tokens, one captured graph) at
         B = 1 and B = 16 with taps off, AttnTaps(segments) and AttnTaps(full + segments) on all 32 layers. The three engines
         of a batch size live in one process and are timed alternately, `--rounds` times, `--steps` replays each.

    python tools/bench_attention_taps.py > profiles/bench_attention_taps.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

L, HD = 32, 128


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
    from bridgelang_amd.engine import rope_tables
    cos, sin = rope_tables(HD, 512, 10000.0, dev)
    out = {}
    for name, (B, H, Sq, Skv, causal) in (("generation_tap_16x32x1x295", (16, 32, 1, 295, False)),
                                          ("attention_maps_layer_1x32x288x288", (1, 32, 288, 288, True))):
        g = torch.Generator().manual_seed(Skv)
        D, cache_len = H * HD, 320
        qkv = torch.randn(B * Sq, 3 * D, generator=g).to(torch.bfloat16).to(dev)
        kc = torch.randn(B, H, cache_len, HD, generator=g).to(torch.bfloat16).to(dev)
        probs = torch.zeros(B, H, Sq, cache_len, dtype=torch.float32, device=dev)
        seg = torch.zeros(B, H, Sq, 4, dtype=torch.float32, device=dev)
        bounds = torch.tensor([[0, 1, 257, Skv - 6, Skv]] * B, dtype=torch.int32, device=dev)
        kw = dict(B=B, H=H, Sq=Sq, Skv=Skv, head_dim=HD, q_strides=(Sq * 3 * D, HD, 3 * D),
                  k_strides=(H * cache_len * HD, cache_len * HD, HD), causal=causal, cos=cos, sin=sin, pos0=Skv - Sq, run=False)
        plans = {"probs_and_segments": ops.attention_probs(qkv, kc, probs=probs, seg=seg, seg_bounds=bounds, **kw),
                 "segments_only": ops.attention_probs(qkv, kc, seg=seg, seg_bounds=bounds, **kw)}
        res = {k: [] for k in plans}
        for _ in range(rounds):
            for k, op in plans.items():
                res[k].append(round(_time(op, launches), 2))
        k_bytes = B * H * Skv * HD * 2 * ((Sq + 15) // 16)      # every 16-row query tile streams the head's K once
        out[name] = dict(us_per_launch=res, k_bytes_read=k_bytes, probs_bytes_written=B * H * Sq * cache_len * 4,
                         k_gb_per_s_segments_only=round(k_bytes / (min(res["segments_only"]) * 1e-6) / 1e9, 1))
    return out


def leg_b(w, dev, steps, rounds, batches):
    from bridgelang_amd.attention_taps import AttnTaps
    from bridgelang_amd.engine import OpenVLAEngine
    out = {}
    for B in batches:
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(3, 31743, (B, L), generator=g)
        ids[:, 0], ids[:, -1] = 1, 29871
        ids, pv = ids.to(dev), (torch.rand(B, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        engines = {"taps_off": OpenVLAEngine(w, B, L), "segments": OpenVLAEngine(w, B, L, attn_taps=AttnTaps()),
                   "both": OpenVLAEngine(w, B, L, attn_taps=AttnTaps(full=True, segments=True))}
        for e in engines.values():
            e.set_inputs(ids, pv)
            e.capture()
        torch.cuda.synchronize()
        same = all(torch.equal(e.gen_ids, engines["taps_off"].gen_ids) and torch.equal(e.logits, engines["taps_off"].logits)
                   for e in engines.values())
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
        out[f"batch_{B}"] = dict(ms_per_action_batch=runs, ids_and_logits_equal_with_taps=same,
                                 tap_launches_per_action_batch=w.dims.llm_layers * 7,
                                 segments_over_off=round(best["segments"] / best["taps_off"], 4),
                                 both_over_off=round(best["both"] / best["taps_off"], 4),
                                 segments_extra_ms=round(best["segments"] - best["taps_off"], 3),
                                 both_extra_ms=round(best["both"] - best["taps_off"], 3))
        del engines
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--model", default="openvla-7b", choices=["openvla-7b", "openvla-tiny"])
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--legs", default="ab", choices=["a", "b", "ab"])
    args = ap.parse_args()
    from bridgelang_amd import weights as W
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_attention_taps.py", "data": "synthetic", "device": torch.cuda.get_device_name(0)}
    if "a" in args.legs:
        line["leg_a_kernel"] = dict(launches=args.launches, rounds=args.rounds, **leg_a(dev, args.launches, args.rounds))
    if "b" in args.legs:
        dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[args.model]()
        w = W.allocate(dims, dev).fill_synthetic(seed=0)
        line["leg_b_action_batch"] = dict(model=dims.name, prompt_len=L, steps=args.steps, rounds=args.rounds,
                                          **leg_b(w, dev, args.steps, args.rounds, [int(b) for b in args.batches.split(",")]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
