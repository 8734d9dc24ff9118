"""TrainStep(loss="preference"): the preference-pair step against torch.autograd over the CPU oracle's logits, the LoRA
learner that starts on its own reference, graph replay under a changing pair assignment, the untouched cross-entropy and
policy plans, and one rollout → pairs → step round trip."""
import math

import numpy as np
import pytest
import torch

from test_policy_step_gpu import oracle_logits, rows_of
from test_train_step_gpu import cos, make_batch

pytestmark = pytest.mark.gpu

B, L = 4, 20
PAIR = [1, -1, 2, -2]


def restated_loss(logits, tg, pair, ref, cfg, S):
    """The torch restatement over [B·S, V] oracle logits (log_softmax, logsigmoid, means) → (loss, [ℓ_k], dict of statistics)."""
    valid = (tg != -100).view(len(pair), S)
    lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)
    logp = lsm.gather(1, tg.clamp(min=0)[:, None])[:, 0].view(len(pair), S)
    d = logp - ref.double().view(len(pair), S)
    delta = [d[b][valid[b]].sum() if cfg.seq_norm == "sum" else d[b][valid[b]].mean() for b in range(len(pair))]
    P = max(abs(p) for p in pair)
    total, per = 0.0, []
    for k in range(1, P + 1):
        rc = sum(delta[b] for b in range(len(pair)) if pair[b] == k)
        rr = sum(delta[b] for b in range(len(pair)) if pair[b] == -k)
        h = cfg.beta * (rc - rr) - cfg.margin
        lk = -(1 - cfg.label_smoothing) * torch.nn.functional.logsigmoid(h) - cfg.label_smoothing * torch.nn.functional.logsigmoid(-h)
        nll = -torch.cat([logp[b][valid[b]] for b in range(len(pair)) if pair[b] == k]).mean()
        total = total + lk + cfg.sft_coef * nll
        per.append(dict(pref=lk.item(), margin=(cfg.beta * (rc - rr)).item(), reward_chosen=(cfg.beta * rc).item(),
                        reward_rejected=(cfg.beta * rr).item(), nll=nll.item(), accuracy=float(rc > rr)))
    return total / P, per, {k: float(np.mean([p[k] for p in per])) for k in per[0]}


@pytest.fixture(scope="module")
def tiny(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    return dims, w, sd, make_batch(dims, B, L)


def test_preference_gradients_match_autograd(dev, tiny):
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    dims, w, sd, (ids, mask, labels, pv) = tiny
    stage = "vla-train"
    cfg = PreferenceLossConfig(beta=0.2, label_smoothing=0.1, sft_coef=0.2, temperature=0.9)
    sd = {k: v.clone() for k, v in sd.items()}
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    logits = oracle_logits(sd, dims, ids, mask, pv)
    S = logits.shape[0] // B
    tg = rows_of(labels, -100).reshape(-1)
    on = labels != -100
    with torch.no_grad():                                   # the oracle's own log π of the labelled tokens, label-aligned
        lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)
        lp_rows = torch.where(tg != -100, lsm.gather(1, tg.clamp(min=0)[:, None])[:, 0], torch.zeros(()).double()).view(B, -1)
        lp = torch.zeros(B, L, dtype=torch.float64)
        lp[:, 1:] = lp_rows[:, 256:]
    g = torch.Generator().manual_seed(9)
    ref = torch.where(on, lp.float() + 0.3 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    want, per, stats = restated_loss(logits, tg, PAIR, rows_of(ref, 0.0).reshape(-1), cfg, S)
    want.backward()

    ts = TrainStep(w, stage, B, L + 2, loss="preference", preference=cfg)          # planned longer than the batch
    ts.set_batch(ids, mask, pv, labels)
    with pytest.raises(RuntimeError):
        ts.backward()                                                               # no pair assignment yet
    ts.set_preference_batch(PAIR, ref)
    loss = ts.forward()
    ts.backward()
    got = {k: v.item() for k, v in ts.preference_stats().items()}
    scale = float(np.mean([abs(p["pref"]) for p in per]))
    print(f"loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |l_k| {scale:.4f}); stats {got}")
    print("oracle stats", stats)
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    assert got["n_pairs"] == 2 and got["loss"] == loss.item() and got["accuracy"] == stats["accuracy"]
    for k in ("pref", "margin", "reward_chosen", "reward_rejected", "nll"):            # the file's loss bound, floor 1
        assert abs(got[k] - stats[k]) <= 2e-3 * max(abs(stats[k]), 1.0), k
    ps, ss = ts.pair_stats(), ts.sequence_stats()
    assert tuple(ps["h"].shape) == (2,) and tuple(ss["n"].shape) == (B,) and ss["n"].tolist() == [8.0] * B
    assert abs(got["loss"] - (ps["loss"].mean() + cfg.sft_coef * ps["nll"].mean()).item()) <= 1e-5 * max(abs(got["loss"]), 1.0)
    worst = 1.0
    for n in names:
        got_g, ref_g = ts.store.named_grad(n).float().cpu(), sd[n].grad
        s = ref_g.abs().max().item()
        assert s > 0, n
        c = cos(got_g, ref_g)
        worst = min(worst, c)
        err = (got_g - ref_g).abs().max().item()
        assert c > 0.99 and err <= 0.06 * s, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {s:.3g}"
    print(f"worst gradient cosine {worst:.5f}")
    tl = ts.token_logprobs().cpu()
    assert tuple(tl.shape) == (B, L) and (tl[~on] == 0).all()
    print(f"max |token_logprobs − oracle| = {(tl[on].double() - lp[on]).abs().max().item():.3g}")
    bad = ref.clone()
    bad[on.nonzero()[0][0], on.nonzero()[0][1]] = float("-inf")
    for args in ((PAIR, bad), (PAIR,), ([1, -1, 3, -3], ref), ([1, 1, 2, -2], ref), ([1, -1, 2], ref), ([1.0, -1.0, 2.0, -2.0], ref)):
        with pytest.raises(ValueError):
            ts.set_preference_batch(*args)
    ts.set_preference_batch([0, 0, 1, -1], bad)                                       # … but not on a sequence in no pair
    with pytest.raises(ValueError):
        TrainStep(w, stage, B, L + 2, loss="policy", preference=cfg)
    with pytest.raises(ValueError):
        TrainStep(w, stage, B, L + 2, loss="preference", preference=PreferenceLossConfig(token_range=(4, 8)))


def test_lora_learner_starts_on_its_reference(dev):
    """PEFT's initial state (B = 0) with ref = the step's own token_logprobs(): loss = log 2 and margin = 0; only lora_B has
    a gradient; five AdamW steps at lr = 2e-2 on one fixed batch make the margin positive and the loss < log 2."""
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    ids, mask, labels, pv = make_batch(dims, B, L)
    lora = LoraAdapters(w, r=8)
    ts = TrainStep(w, "lora", B, L + 2, lora=lora, loss="preference", preference=PreferenceLossConfig(beta=0.5))
    ts.set_batch(ids, mask, pv, labels)
    ts.forward()                                            # no pairs yet: the forward that records the reference
    ref = ts.token_logprobs().clone()
    assert bool((ref[(labels != -100).to(dev)] < 0).all())
    ts.set_preference_batch(PAIR, ref)
    loss = ts.forward().item()
    st = {k: v.item() for k, v in ts.preference_stats().items()}
    print("at the reference:", st)
    assert abs(loss - math.log(2)) <= 1e-4 and abs(st["margin"]) <= 1e-4 and st["accuracy"] == 0 and st["n_pairs"] == 2
    ts.backward()
    grads = lora.state_dict({u.key: ts.store.grad[u.offset:u.offset + u.numel] for u in ts.store.units})
    assert all(v.abs().sum() > 0 for k, v in grads.items() if "lora_B" in k)
    assert all(v.abs().sum() == 0 for k, v in grads.items() if "lora_A" in k)      # B = 0: nothing reaches A yet
    for _ in range(5):
        ts.step(2e-2)
    loss = ts.forward().item()
    st = {k: v.item() for k, v in ts.preference_stats().items()}
    print("after five steps:", st)
    assert st["margin"] > 0 and loss < math.log(2) and st["reward_chosen"] > st["reward_rejected"]


def test_graph_replay_is_bit_identical_and_serves_another_pair_assignment(dev, tiny):
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, _, (ids, mask, labels, pv) = tiny
    ts = TrainStep(w, "vla-train", B, L + 2, loss="preference",
                   preference=PreferenceLossConfig(beta=0.3, seq_norm="mean", reference_free=True, margin=0.5, sft_coef=0.1))
    ts.set_batch(ids, mask, pv, labels)
    outs = (ts.stats, ts.dlogits, ts.pair_stats_buf, ts.seq_stats_buf)

    def run(graph):
        for t in outs:
            t.zero_()
        loss = ts.forward(graph=graph).item()
        ts.backward(graph=graph)
        return [loss] + [t.clone() for t in outs]
    same = lambda a, b: a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    ts.set_preference_batch(PAIR)
    eager = run(False)
    assert eager[1][1].item() == 2 and eager[2].abs().sum() > 0
    assert same(run(True), eager) and same(run(True), eager)            # the capture, then a replay
    ts.set_preference_batch([-1, 0, 1, 1])                              # one 2-vs-1 pair and a sequence in none: P = 1
    replay = run(True)
    assert replay[1][1].item() == 1 and not same(replay, eager)
    assert same(run(False), replay)
    S = ts.S
    assert (replay[2].view(B, S, -1)[1] == 0).all() and replay[3][1].abs().sum() == 0


def test_other_losses_are_untouched_by_a_preference_step(dev):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    ids, mask, labels, pv = make_batch(dims, B, L)
    on = labels != -100
    A = torch.where(on, torch.randn(B, L, generator=torch.Generator().manual_seed(2)) + 0.3, torch.zeros(B, L))
    q = torch.where(on, torch.full((B, L), -5.0), torch.zeros(B, L))

    def run(kind):
        ts = TrainStep(w, "vla-train", B, L + 2, loss=kind, **({"policy": PolicyLossConfig(temperature=0.8)} if kind == "policy" else {}))
        ts.set_batch(ids, mask, pv, labels)
        if kind == "policy":
            ts.set_policy_batch(A, q)
        loss = ts.forward().item()
        ts.backward()
        return (loss, [op.name for op in ts.forward_ops], [op.name for op in ts.backward_ops], ts.dlogits.clone(),
                {n: ts.store.named_grad(n).clone() for n in trainable_names(w, "vla-train")})
    before = {kind: run(kind) for kind in ("ce", "policy")}
    pref = TrainStep(w, "vla-train", B, L + 2, loss="preference", preference=PreferenceLossConfig(reference_free=True))
    pref.set_batch(ids, mask, pv, labels)
    pref.set_preference_batch(PAIR)
    pref.forward()
    pref.backward()
    fo, bo = [op.name for op in pref.forward_ops], [op.name for op in pref.backward_ops]
    assert fo[:-1] == before["ce"][1][:-1] and fo[-1] == "bl_preference_loss_f32"            # only the loss boundary differs
    assert bo[1:] == before["ce"][2][1:] and bo[0] == "bl_policy_loss_backward_f32"
    for kind in ("ce", "policy"):
        a, b = before[kind], run(kind)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3]), kind
        assert all(torch.equal(a[4][n], b[4][n]) for n in a[4]), kind
        assert not any("preference" in name for name in a[1] + a[2])


def test_rollouts_to_preference_step_end_to_end(dev):
    from bridgelang_amd import sampling as S
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.rl import pairs_from_rewards, preference_batch
    from bridgelang_amd.training.step import TrainStep
    from test_engine_gpu import make_inputs
    from test_lora_inference_gpu import new_model
    model = new_model(dev)
    Bp, K, n, temp = 2, 4, 7, 1.3
    ids, pv = make_inputs(model.dims, Bp, 10, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    lora = LoraAdapters(model.weights, r=8)
    model.attach_adapters(lora)
    rng = model.action_token_range()
    actions, tokens, _ = model.sample_actions(ids, pv, "bridge_orig", S.SamplingParams(temperature=temp, seed=[5, 6]), num_samples=K,
                                              action_tokens_only=True)
    rewards = -np.abs(actions - 0.1).sum(-1)                                            # synthetic: prefer actions near 0.1
    c, r, keep = pairs_from_rewards(rewards)
    assert bool(keep.all())
    chosen, rejected = tokens[np.arange(Bp), c.numpy()], tokens[np.arange(Bp), r.numpy()]
    score = lambda tok, **kw: model.score_actions(ids, pv, token_ids=tok, sampling=S.SamplingParams(temperature=temp),
                                                  action_tokens_only=True, **kw)[:, 0]
    ref_c, ref_r = score(chosen, use_adapters=False), score(rejected, use_adapters=False)
    batch = preference_batch(ids, None, chosen, rejected, ref_c, ref_r, token_range=rng)
    assert batch["pair"].tolist() == [1, -1, 2, -2] and batch["input_ids"].shape == (2 * Bp, 10 + n + 1)
    ts = TrainStep(model.weights, "lora", 2 * Bp, batch["input_ids"].shape[1], lora=lora, loss="preference",
                   preference=PreferenceLossConfig(beta=0.5, temperature=temp, token_range=rng), refresh_adapted=True)
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv.repeat_interleave(2, 0), batch["labels"])
    ts.set_preference_batch(batch["pair"], batch["ref_logprobs"])
    gap = lambda: (score(chosen).sum(-1) - score(rejected).sum(-1))
    before = gap()
    assert np.array_equal(before, ref_c.sum(-1) - ref_r.sum(-1))                        # B = 0: the adapted policy is the base
    # At the reference h_k ≈ 0 and ℓ'_k ≈ −1/2 for every pair, so the step descends −β/(2P)·∇Σ_k Δ_k: to first order it is
    # the SUM of the pairs' gaps that must rise (one pair may pay for another), and lr = 5e-3 keeps AdamW's first step
    # (±lr per adapter entry) inside that first-order range on this model.
    loss, norm = ts.step(5e-3)
    st = {k: v.item() for k, v in ts.preference_stats().items()}
    print("first step:", st)
    assert np.isfinite(loss.item()) and norm.item() > 0 and st["n_pairs"] == Bp and abs(st["margin"]) < 0.05
    after = gap()
    print("log π(chosen) − log π(rejected) under the adapters:", before, "→", after)
    assert after.sum() > before.sum()
    assert np.array_equal(score(chosen, use_adapters=False), ref_c)                     # the reference did not move
    model.detach_adapters()
