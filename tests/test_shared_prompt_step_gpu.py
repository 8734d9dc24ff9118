"""TrainStep(shared_prompt=G, branch_len=nb): a prompt's G sequences trained over ONE forward of the prompt.

The oracle runs the REPLICATED six sequences (P = 2 prompts of different lengths × G = 3) through `oracle_logits`, and the
shared step is held to the bounds of tests/test_policy_step_gpu.py against torch.autograd over it: loss within 2e-3 × the mean
|row loss|, the statistics within the same bound (floor 1), every trainable tensor's gradient at cosine > 0.99 and max error
<= 0.06 × its scale — for loss="policy" at token level and at ratio_level="action", and for loss="ce", at stage vla-train, and
once under LoRA. The action-level case uses ratio_norm="mean": the action's log-ratio is then a mean of token log-ratios and
carries one token's bf16-sized difference between the device's and the oracle's log π, so the file's bound applies as it
stands (under "sum" the differences of the n tokens add up, which tests/test_action_ratio_step_gpu.py allows for).
Then: readers come back in the caller's shapes and order, recompute / graph replay / a second eager run give the same bits,
the default plans hold none of the new entry points, the unsupported combinations raise, and a rollout round trip.
"""
import numpy as np
import pytest
import torch

from test_action_ratio_step_gpu import oracle_logits, restated_action_loss, rows_of
from test_policy_step_gpu import restated_loss
from test_train_step_gpu import cos

from conftest import rand_bf16

pytestmark = pytest.mark.gpu

NP, G, L, NB = 2, 3, 20, 8
B = NP * G
TEMP = 0.9
NEW = ("bl_attention_tree_lse_bf16", "bl_attention_tree_backward_bf16", "bl_rope_pos_bf16", "bl_rope_pos_backward_bf16")


def make_group_batch(seed=0):
    """P prompts of 11 and 8 tokens, each with G continuations of 7 action tokens + EOS, labelled on those 8 (the collator's
    form); right-padded to L. pixel values one per PROMPT."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, L), 32000)
    mask = torch.zeros(B, L, dtype=torch.bool)
    labels = torch.full((B, L), -100)
    for p, lp in enumerate((11, 8)):
        prompt = torch.randint(3, 31000, (lp,), generator=g)
        prompt[0] = 1
        for k in range(G):
            b, n = p * G + k, lp + 8
            ids[b, :lp] = prompt
            ids[b, lp:n - 1] = torch.randint(31744, 32000, (7,), generator=g)
            ids[b, n - 1] = 2
            mask[b, :n] = True
            labels[b, lp:n] = ids[b, lp:n]
    pv = rand_bf16((NP, 6, 224, 224), seed + 1)
    return ids, mask, labels, pv


@pytest.fixture(scope="module")
def world(dev):
    """The tiny model, the grouped batch, the oracle's logits over the replicated sequences (graph kept: one backward per
    loss) and its own log π of the labelled tokens at TEMP, label-aligned."""
    from bridgelang_amd.training.step import trainable_names
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    ids, mask, labels, pv = make_group_batch()
    names = trainable_names(w, "vla-train")
    for n in names:
        sd[n].requires_grad_(True)
    logits = oracle_logits(sd, dims, ids, mask, pv.repeat_interleave(G, 0))          # [B, S − 1, V]
    tg = rows_of(labels, -100)
    with torch.no_grad():
        lsm = torch.log_softmax(logits.double() / TEMP, dim=-1)
        lp_rows = torch.where(tg != -100, lsm.gather(2, tg.clamp(min=0)[..., None])[..., 0], torch.zeros(()).double())
        lp = torch.zeros(B, L, dtype=torch.float64)
        lp[:, 1:] = lp_rows[:, 256:]
    return dict(dims=dims, w=w, sd=sd, names=names, batch=(ids, mask, labels, pv), logits=logits, tg=tg, lp=lp)


def policy_inputs(world, level):
    ids, mask, labels, pv = world["batch"]
    on, lp = labels != -100, world["lp"]
    g = torch.Generator().manual_seed(9)
    A = torch.where(on, torch.randn(B, L, generator=g) + 0.5, torch.zeros(B, L))
    if level == "token":     # log-ratios ±0.5 (clipped on one side each), ±0.05 and 0 (inside), as the token-level file draws them
        shift = torch.tensor([0.5, -0.05, 0.05, -0.5, 0.0])[torch.arange(B * L) % 5].view(B, L)
    else:                    # per ACTION (mean norm): +0.6 / −0.6 clipped, ±0.02 inside
        shift = torch.tensor([0.6, -0.02, -0.6, 0.02, 0.6, -0.6])[:, None].expand(B, L)
    q = torch.where(on, (lp - shift).float(), torch.zeros(B, L))
    ref = torch.where(on, lp.float() + 0.2 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    return A, q, ref


def check_grads(named_got, names, want_grads):
    worst = 1.0
    for n, ref_g in zip(names, want_grads):
        got = named_got(n)
        s = ref_g.abs().max().item()
        assert s > 0, n
        c = cos(got, ref_g)
        worst = min(worst, c)
        err = (got - ref_g).abs().max().item()
        assert c > 0.99 and err <= 0.06 * s, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {s:.3g}"
    print(f"worst gradient cosine {worst:.5f}")


@pytest.mark.parametrize("kind", ["policy-token", "policy-action", "ce"])
def test_shared_step_matches_autograd_over_replicated_sequences(dev, world, kind):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, sd, names = world["dims"], world["w"], world["sd"], world["names"]
    ids, mask, labels, pv = world["batch"]
    logits, tg, on = world["logits"], world["tg"], labels != -100
    params = [sd[n] for n in names]
    if kind == "ce":
        rows = torch.nn.functional.cross_entropy(logits.reshape(-1, dims.vocab).double(), tg.reshape(-1), ignore_index=-100, reduction="none")
        row = rows[tg.reshape(-1) != -100]
        want = row.mean()
        ts = TrainStep(w, "vla-train", B, L + 2, shared_prompt=G, branch_len=NB)
        ts.set_batch(ids, mask, pv, labels)
    else:
        level = kind.split("-")[1]
        cfg = PolicyLossConfig(temperature=TEMP, clip_low=0.2, clip_high=0.2, entropy_coef=0.01, kl_coef=0.05,
                               **(dict(ratio_level="action", ratio_norm="mean") if level == "action" else {}))
        A, q, ref = policy_inputs(world, level)
        if level == "token":
            want, row, ratio, _, stats = restated_loss(logits.reshape(-1, dims.vocab), tg.reshape(-1), rows_of(A, 0.0).reshape(-1),
                                                       rows_of(q, 0.0).reshape(-1), rows_of(ref, 0.0).reshape(-1), cfg)
        else:
            want, row, s, _, stats = restated_action_loss(logits, tg, rows_of(A, 0.0), rows_of(q, 0.0), rows_of(ref, 0.0), cfg)
            ratio = torch.exp(s)
        ratio = ratio.detach()       # every ratio at least 0.03 away from the clip boundaries: the clip fraction compares exactly
        assert ((ratio - 0.8).abs().min() > 0.03) and ((ratio - 1.2).abs().min() > 0.03) and 0 < stats["clip_frac"] < 1
        ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=cfg, shared_prompt=G, branch_len=NB)
        ts.set_batch(ids, mask, pv, labels)
        ts.set_policy_batch(A, q, ref)
    want_grads = torch.autograd.grad(want, params, retain_graph=True)
    assert ts.B == NP and ts.T == NP * ts.shared.S and ts.shared.P0 % NB == 0
    loss = ts.forward()
    ts.backward()
    scale = row.detach().abs().mean().item()
    print(f"[{kind}] loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |row_loss| {scale:.4f}); "
          f"{ts.T} token rows against {B * (L + 2 + 256)} replicated")
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    if kind != "ce":
        got_stats = {k: v.item() for k, v in ts.policy_stats().items()}
        print("stats", got_stats, "oracle", {k: float(v.detach()) for k, v in stats.items()})
        assert got_stats["n_valid"] == int(on.sum()) and got_stats["loss"] == loss.item()
        assert got_stats["clip_frac"] == pytest.approx(float(stats["clip_frac"]), abs=1e-6)
        for k in ("pg", "entropy", "kl", "approx_kl", "ratio"):
            assert abs(got_stats[k] - float(stats[k])) <= 2e-3 * max(abs(float(stats[k])), 1.0), k
        tl = ts.token_logprobs().cpu()                      # [B, l] in the caller's order
        assert tuple(tl.shape) == (B, L) and (tl[~on] == 0).all() and (tl[on] < 0).all()
        dlp = (tl[on].double() - world["lp"][on]).abs().max().item()
        print(f"max |token_logprobs − oracle| = {dlp:.3g}")
        assert dlp < 0.05                                   # a misplaced row would be off by whole nats
        if kind == "policy-action":
            act = {k: v.cpu() for k, v in ts.action_stats().items()}
            assert all(tuple(v.shape) == (B,) for v in act.values()) and torch.equal(act["n"], on.sum(1).float())
            assert (act["log_ratio"].double() - s.detach()).abs().max().item() < 0.02      # per sequence, in the caller's order
    check_grads(lambda n: ts.store.named_grad(n).float().cpu(), names, want_grads)


def test_shared_step_under_lora(dev, world):
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate
    from test_lora_gpu import effective_sd, random_adapters
    dims = world["dims"]
    ids, mask, labels, pv = world["batch"]
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.detach().float().cpu() for k, v in w.state_dict().items()}
    lora = LoraAdapters(w, r=32)
    ad_sd = random_adapters(lora, seed=7)
    lora.load_state_dict(ad_sd)
    mods = [m for ad in lora.adapters for m in ad.modules]
    params = {k: v.clone().requires_grad_(True) for k, v in ad_sd.items()}
    logits = oracle_logits(effective_sd(sd, params, lora.scaling, mods), dims, ids, mask, pv.repeat_interleave(G, 0))
    tg, on = rows_of(labels, -100), labels != -100
    cfg = PolicyLossConfig(temperature=TEMP, clip_low=0.2, clip_high=0.2, entropy_coef=0.01)
    with torch.no_grad():
        lsm = torch.log_softmax(logits.double() / TEMP, dim=-1)
        lp = torch.zeros(B, L, dtype=torch.float64)
        lp[:, 1:] = torch.where(tg != -100, lsm.gather(2, tg.clamp(min=0)[..., None])[..., 0], torch.zeros(()).double())[:, 256:]
    A, q, _ = policy_inputs(dict(world, lp=lp), "token")
    zero = torch.zeros(B * (L + 255))
    want, row, ratio, _, stats = restated_loss(logits.reshape(-1, dims.vocab), tg.reshape(-1), rows_of(A, 0.0).reshape(-1),
                                               rows_of(q, 0.0).reshape(-1), zero, cfg)
    ratio = ratio.detach()
    assert ((ratio - 0.8).abs().min() > 0.03) and ((ratio - 1.2).abs().min() > 0.03) and 0 < stats["clip_frac"] < 1
    want.backward()
    ts = TrainStep(w, "lora", B, L + 2, lora=lora, loss="policy", policy=cfg, shared_prompt=G, branch_len=NB, max_grad_norm=float("inf"))
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, q)
    loss = ts.forward()
    ts.backward()
    scale = row.detach().abs().mean().item()
    print(f"[lora] loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |row_loss| {scale:.4f})")
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    assert ts.policy_stats()["clip_frac"].item() == pytest.approx(float(stats["clip_frac"]), abs=1e-6)
    masters = {u.key: ts.store.grad[u.offset:u.offset + u.numel] for u in ts.store.units}
    got = lora.state_dict(masters)
    check_grads(lambda k: got[k].float().cpu(), list(params), [p.grad for p in params.values()])


def _bits(ts):
    return dict(stats=ts.stats.clone(), dlogits=ts.dlogits.clone(), grad=ts.store.grad.clone(), lp=ts.token_logprobs().clone())


def test_recompute_graph_replay_and_second_run_give_the_same_bits(dev, world):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    w = world["w"]
    ids, mask, labels, pv = world["batch"]
    A, q, ref = policy_inputs(world, "token")
    cfg = PolicyLossConfig(temperature=TEMP, entropy_coef=0.01, kl_coef=0.05)
    runs = {}
    for recompute in (False, True):
        ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=cfg, shared_prompt=G, branch_len=NB, recompute=recompute)
        ts.set_batch(ids, mask, pv, labels)
        ts.set_policy_batch(A, q, ref)
        ts.forward()
        ts.backward()
        runs[recompute] = _bits(ts)
        assert float(ts.store.grad.abs().sum()) > 0
        if recompute:
            continue
        ts.store.grad.zero_()
        ts.forward()
        ts.backward()
        again = _bits(ts)
        for _ in range(2):                                   # the capture, then a replay
            ts.stats.zero_()
            ts.dlogits.zero_()
            ts.store.grad.zero_()
            ts.forward(graph=True)
            ts.backward(graph=True)
            replay = _bits(ts)
            for k in again:
                assert torch.equal(runs[False][k], again[k]), f"{k}: two eager runs differ"
                assert torch.equal(runs[False][k], replay[k]), f"{k}: graph replay differs from eager"
    for k in runs[False]:
        assert torch.equal(runs[False][k], runs[True][k]), f"{k}: recompute=True differs"


def test_default_plans_hold_none_of_the_new_entry_points_and_limits_raise(dev, world):
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    w = world["w"]
    ids, mask, labels, pv = world["batch"]
    plain = TrainStep(w, "vla-train", B, L + 2, loss="policy")
    fo, bo = [op.name for op in plain.forward_ops], [op.name for op in plain.backward_ops]
    assert not any(n in NEW for n in fo + bo) and plain.shared is None and not hasattr(plain, "pos_rows")
    sh = TrainStep(w, "vla-train", B, L + 2, loss="policy", shared_prompt=G, branch_len=NB)
    fs, bs = [op.name for op in sh.forward_ops], [op.name for op in sh.backward_ops]
    swap = {"bl_rope_bf16": "bl_rope_pos_bf16", "bl_attention_lse_bf16": "bl_attention_tree_lse_bf16",
            "bl_rope_backward_bf16": "bl_rope_pos_backward_bf16", "bl_attention_backward_bf16": "bl_attention_tree_backward_bf16"}
    assert fs == [swap.get(n, n) for n in fo] and bs == [swap.get(n, n) for n in bo]      # the same plans over another row layout
    nl = world["dims"].llm_layers
    assert fs.count(NEW[0]) == nl and fs.count(NEW[2]) == nl and bs.count(NEW[1]) == nl and bs.count(NEW[3]) == nl
    for kw in (dict(loss="preference", preference=PreferenceLossConfig()), dict(loss="distill", distill=DistillLossConfig()),
               dict(loss="policy", value=ValueLossConfig()), dict(fp8=True), dict(world=2, rank=0), dict(shared_prompt=G),
               dict(branch_len=NB)):
        args = dict(shared_prompt=G, branch_len=NB)
        if "shared_prompt" in kw or "branch_len" in kw:
            args = {}
        with pytest.raises(ValueError, match="shared_prompt"):
            TrainStep(w, "vla-train", B, L + 2, **args, **kw)
    with pytest.raises(ValueError, match="multiple"):
        TrainStep(w, "vla-train", B - 1, L + 2, shared_prompt=G, branch_len=NB)
    # a batch the layout refuses leaves the static inputs as they were
    sh.set_batch(ids, mask, pv, labels)
    before = (sh.input_ids.clone(), sh.key_mask.clone(), sh.targets.clone(), sh.pos_rows.clone())
    bad = ids.clone()
    bad[1, 3] += 1                                          # a prompt token differs inside group 0
    with pytest.raises(ValueError, match="differ"):
        sh.set_batch(bad, mask, pv, labels)
    with pytest.raises(ValueError):
        sh.set_batch(ids[:B - 1], mask[:B - 1], pv, labels[:B - 1])
    for a, b in zip(before, (sh.input_ids, sh.key_mask, sh.targets, sh.pos_rows)):
        assert torch.equal(a, b)


def test_rollout_round_trip(dev):
    """sample_actions(num_samples=3, share_prefill=True) → group_advantages → policy_batch → three shared steps: the prompt is
    paid for once on both sides; the loss is finite and falls."""
    from bridgelang_amd import sampling as S
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import group_advantages, policy_batch
    from bridgelang_amd.training.step import TrainStep
    from test_engine_gpu import make_inputs
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    model = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=W.tiny_dims()).init_synthetic(seed=11)
    Bp, K, n, temp = 2, 3, 7, 1.3
    ids, pv = make_inputs(model.dims, Bp, 10, seed=31)
    actions, tokens, lp = model.sample_actions(ids.to(dev), pv.to(dev), "bridge_orig", S.SamplingParams(temperature=temp, seed=[5, 6]),
                                               num_samples=K, share_prefill=True)
    adv = group_advantages(-np.abs(actions - 0.1).sum(-1))
    assert float(adv.abs().max()) > 0
    batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(Bp * K, n), lp.reshape(Bp * K, n), adv.reshape(-1))
    l = batch["input_ids"].shape[1]
    ts = TrainStep(model.weights, "vla-train", Bp * K, l, loss="policy", policy=PolicyLossConfig(temperature=temp),
                   shared_prompt=K, branch_len=n)
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv, batch["labels"])      # one image per prompt
    ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
    losses = []
    for i in range(3):
        loss, norm = ts.step(2e-4)
        losses.append(loss.item())
        if i == 0:
            first = {k: v.item() for k, v in ts.policy_stats().items()}
            print("rollout vs shared training forward:", first)
            # the sampler's π is the learner's up to bf16 noise between two kernel paths; a misplaced row is off by whole nats
            assert first["n_valid"] == Bp * K * n and abs(first["ratio"] - 1.0) < 0.25
        assert np.isfinite(losses[-1]) and np.isfinite(norm.item()) and norm.item() > 0
    print("losses over three steps:", losses)
    assert losses[2] < losses[0]
