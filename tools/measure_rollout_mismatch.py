#!/usr/bin/env python
"""How far the policy that draws the tokens is from the policy the learner differentiates, and what the rollout correction
(PolicyLossConfig.rollout_is_cap, bl_policy_loss_is_f32) costs at the loss boundary; one JSON line. A record, nothing is
gated and nothing is tuned against it.

  mismatch  per model (`--models`): one rollout batch from `sample_actions(action_tokens_only=True)` at temperature 1 under
            LoRA adapters at their initial values (B = 0: the base model), once through the bf16 prefill and once through the
            e4m3 prefill (`attach_adapters(lora, fp8=True)`, `model.fp8`), each fed to ONE self-proximal forward of the bf16
            learner (`TrainStep(stage="lora")`, before any update): `rollout_stats()` and |λ| = |log π_learner − log μ| over
            the sampled tokens. The truncation and the mask are set wide (cap 2, mask (1/4, 4)) so the fractions count
            outliers only.
  loss_ops  the forward loss op alone at the 7B training shape (32·296 rows of 32 064 logits, 8 labelled rows per sample):
            the uncorrected op of each level, ranged and unranged, against bl_policy_loss_is_f32 on the same buffers, HIP
            events around `--reps` launches each (launch overhead included), in one process.

    python tools/measure_rollout_mismatch.py > profiles/rollout_mismatch.json

That one invocation writes the whole record (both models, then the loss ops). `device` is the name the runtime reports for
the card, `arch` its gfx target.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def op_times(args, dev):
    from bridgelang_amd import train_ops as T
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    B, S, V = 32, 296, 32064
    rows = B * S
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, device=dev) * 2).to(torch.bfloat16).float()
    tgt = torch.full((B, S), -100, dtype=torch.int64)
    tgt[:, -9:-1] = torch.randint(31744, 32000, (B, 8), generator=g)
    tgt = tgt.view(-1).to(dev)
    f = lambda: torch.randn(rows, generator=g).mul_(0.1).to(dev)
    A, q, mu, ref = f(), f() - 10.0, f() - 10.0, f() - 10.0
    row_stats, stats, group_stats = torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(B, 4, device=dev)
    is_rows, is_stats = torch.zeros(rows, 2, device=dev), torch.zeros(8, device=dev)
    out = {}
    for level in ("token", "action"):
        for rng in (None, (31744, 256)):
            base = dict(entropy_coef=0.01, kl_coef=0.05, ratio_level=level, token_range=rng)
            plain = T.policy_loss(logits, tgt, A, q, ref, row_stats, stats, PolicyLossConfig(**base), run=False, group_rows=S,
                                  group_stats=group_stats)
            cfg = PolicyLossConfig(rollout_is_cap=2.0, rollout_is_mask=(0.25, 4.0), **base)
            fixed = {"given": T.policy_loss(logits, tgt, A, q, ref, row_stats, stats, cfg, run=False, group_rows=S, group_stats=group_stats,
                                            behaviour_logprob=mu, is_rows=is_rows, is_stats=is_stats),
                     "self": T.policy_loss(logits, tgt, A, None, ref, row_stats, stats, cfg, run=False, group_rows=S,
                                           group_stats=group_stats, behaviour_logprob=mu, is_rows=is_rows, is_stats=is_stats)}
            times = {}
            for name, op in ((plain.name, plain), *((f"{o.name}[{k}]", o) for k, o in fixed.items())):
                for _ in range(3):
                    op.run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    op.run()
                e1.record()
                torch.cuda.synchronize()
                times[name] = round(e0.elapsed_time(e1) / args.reps * 1e3, 2)
            out[f"{level}{'' if rng is None else ' ranged'}"] = times
    return {"rows": rows, "n": V, "valid_rows": int((tgt != -100).sum()), "reps": args.reps, "us_per_call_events": out}


def mismatch(name, dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    from bridgelang_amd.sampling import SamplingParams
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import policy_batch
    from bridgelang_amd.training.step import TrainStep
    dims = {"openvla-7b": W.openvla_7b_dims, "openvla-tiny": W.tiny_dims}[name]()
    stats = {"robot": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    model = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=dims).init_synthetic(seed=0)
    Bp, K, Lp, n = 4, 4, 32, 7
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, 31743, (Bp, Lp), generator=g)
    ids[:, 0], ids[:, -1] = 1, 29871
    pv = (torch.rand(Bp, 6, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16)
    sp = SamplingParams(temperature=1.0, seed=list(range(Bp)))
    rng = model.action_token_range()
    lora = LoraAdapters(model.weights, r=8)
    model.attach_adapters(lora, fp8=True)
    cfg = PolicyLossConfig(temperature=1.0, token_range=rng, rollout_is_cap=2.0, rollout_is_mask=(0.25, 4.0))
    ts, out = None, {"model": dims.name, "tokens": Bp * K * n, "temperature": 1.0, "learner": "bf16 training forward, LoRA stage, no update"}
    try:
        for engine, fp8 in (("bf16", False), ("e4m3", True)):
            model.fp8 = fp8
            _, tokens, lp = model.sample_actions(ids.to(dev), pv.to(dev), "robot", sp, num_samples=K, action_tokens_only=True)
            b = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(Bp * K, n), lp.reshape(Bp * K, n), torch.zeros(Bp * K),
                             token_range=rng, rollout_is=True)
            if ts is None:
                ts = TrainStep(model.weights, "lora", Bp * K, b["input_ids"].shape[1], lora=lora, loss="policy", policy=cfg)
            ts.set_batch(b["input_ids"], b["attention_mask"], pv.repeat_interleave(K, 0), b["labels"])
            ts.set_policy_batch(b["advantages"], None, behaviour_logprobs=b["behaviour_logprobs"])
            ts.forward()
            lam = ts.is_rows[ts.targets != -100, 0].double().abs()
            out[f"{engine}_rollout"] = {**{k: float(v.item()) for k, v in ts.rollout_stats().items()},
                                        "abs_log_rho_mean": float(lam.mean()), "abs_log_rho_max": float(lam.max())}
    finally:
        model.fp8 = False
        model.detach_adapters()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--models", default="openvla-tiny,openvla-7b", help="comma-separated: openvla-tiny, openvla-7b; empty: none")
    ap.add_argument("--no-ops", action="store_true", help="skip the loss-op timing")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "tools/measure_rollout_mismatch.py", "data": "synthetic", "device": torch.cuda.get_device_name(0),
            "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "mismatch": []}
    for name in filter(None, args.models.split(",")):
        line["mismatch"].append(mismatch(name, dev))
        torch.cuda.empty_cache()
    if not args.no_ops:
        line["loss_ops"] = op_times(args, dev)
    assert all(np.isfinite(v) for m in line["mismatch"] for k, r in m.items() if k.endswith("_rollout") for v in r.values())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
