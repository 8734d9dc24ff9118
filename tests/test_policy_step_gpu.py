"""TrainStep(loss="policy"): the clipped-surrogate policy-gradient step against torch.autograd over the CPU oracle's logits,
its on-policy and graph-replay properties, the unchanged default (cross-entropy) plan, and one rollout → step round trip."""
import numpy as np
import pytest
import torch

from oracle import restate as R
from test_train_step_gpu import cos, make_batch

pytestmark = pytest.mark.gpu

B, L = 3, 20


def rows_of(x, fill):
    """[B, L] aligned with the labels → [B, S - 1] aligned with logits[:, :-1] (oracle_loss's label placement)."""
    full = torch.cat([x[:, :1], torch.full((x.shape[0], 256), fill, dtype=x.dtype), x[:, 1:]], 1)
    return full[:, 1:]


def oracle_logits(sd, dims, ids, mask, pv):
    om = R.OracleModel.from_dims(sd, dims)
    logits, _, _ = om.prefill(ids, pv, attention_mask=mask)
    return logits[:, :-1].reshape(-1, dims.vocab)


def restated_loss(logits, tg, A, q, ref, cfg):
    """The torch restatement of the policy loss (log_softmax, minimum, clamp) → (loss, per-row dict) over valid rows."""
    valid = tg != -100
    lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)[valid]
    logp = lsm.gather(1, tg[valid][:, None])[:, 0]
    A, q = A[valid].double(), q[valid].double()
    ratio = torch.exp(logp - q)
    lo, hi = 1 - cfg.clip_low, 1 + cfg.clip_high
    pg = -torch.minimum(ratio * A, ratio.clamp(lo, hi) * A)
    H = -(lsm.exp() * lsm).sum(-1)
    d = ref[valid].double() - logp
    kl = torch.exp(d) - d - 1
    row = pg - cfg.entropy_coef * H + cfg.kl_coef * kl
    active = ((A >= 0) & (ratio <= hi)) | ((A < 0) & (ratio >= lo))
    lr = logp - q
    stats = dict(loss=row.mean(), n_valid=valid.sum(), pg=pg.mean(), entropy=H.mean(), kl=kl.mean(), clip_frac=(~active).double().mean(),
                 approx_kl=(torch.expm1(lr) - lr).mean(), ratio=ratio.mean())
    return row.mean(), row, ratio, logp, stats


@pytest.fixture(scope="module")
def tiny(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    ids, mask, labels, pv = make_batch(dims, B, L)
    return dims, w, sd, (ids, mask, labels, pv)


def test_policy_gradients_match_autograd(dev, tiny):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    dims, w, sd, (ids, mask, labels, pv) = tiny
    stage = "vla-train"
    cfg = PolicyLossConfig(temperature=0.9, clip_low=0.2, clip_high=0.2, entropy_coef=0.01, kl_coef=0.05)
    sd = {k: v.clone() for k, v in sd.items()}
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    logits = oracle_logits(sd, dims, ids, mask, pv)
    tg = rows_of(labels, -100).reshape(-1)
    on = labels != -100
    with torch.no_grad():                                   # the oracle's own log π of the labelled tokens, label-aligned
        lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)
        lp_rows = torch.where(tg != -100, lsm.gather(1, tg.clamp(min=0)[:, None])[:, 0], torch.zeros(()).double()).view(B, -1)
        lp = torch.zeros(B, L, dtype=torch.float64)
        lp[:, 1:] = lp_rows[:, 256:]
    g = torch.Generator().manual_seed(9)
    A = torch.where(on, torch.randn(B, L, generator=g) + 0.5, torch.zeros(B, L))                 # non-zero mean
    # behaviour policy = the oracle's, moved by log-ratios of ±0.5 (clipped on one side each) and ±0.05 (inside): far from
    # the boundaries log 0.8 / log 1.2 compared with the bf16 noise between the device's and the oracle's log π
    shift = torch.tensor([0.5, -0.05, 0.05, -0.5, 0.0])[torch.arange(B * L) % 5].view(B, L)
    q = torch.where(on, lp.float() - shift, torch.zeros(B, L))
    ref = torch.where(on, lp.float() + 0.2 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    want, row, ratio, _, stats = restated_loss(logits, tg, rows_of(A, 0.0).reshape(-1), rows_of(q, 0.0).reshape(-1),
                                               rows_of(ref, 0.0).reshape(-1), cfg)
    assert ((ratio - 0.8).abs().min() > 0.03) and ((ratio - 1.2).abs().min() > 0.03) and 0 < stats["clip_frac"] < 1
    want.backward()

    ts = TrainStep(w, stage, B, L + 2, loss="policy", policy=cfg)          # planned longer than the batch
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, q, ref)
    loss = ts.forward()
    ts.backward()
    got_stats = {k: v.item() for k, v in ts.policy_stats().items()}
    scale = row.abs().mean().item()
    print(f"loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |row_loss| {scale:.4f}); stats {got_stats}")
    print("oracle stats", {k: float(v.detach()) for k, v in stats.items()})
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    assert got_stats["n_valid"] == int(on.sum()) and got_stats["loss"] == loss.item()
    assert got_stats["clip_frac"] == pytest.approx(float(stats["clip_frac"]), abs=1e-6)      # no ratio within reach of a boundary
    for k in ("pg", "entropy", "kl", "approx_kl", "ratio"):                                  # the file's loss bound, floor 1
        assert abs(got_stats[k] - float(stats[k])) <= 2e-3 * max(abs(float(stats[k])), 1.0), k
    worst = 1.0
    for n in names:
        got, ref_g = ts.store.named_grad(n).float().cpu(), sd[n].grad
        s = ref_g.abs().max().item()
        assert s > 0, n
        c = cos(got, ref_g)
        worst = min(worst, c)
        err = (got - ref_g).abs().max().item()
        assert c > 0.99 and err <= 0.06 * s, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {s:.3g}"
    print(f"worst gradient cosine {worst:.5f}")
    # token_logprobs(): the device's log π, label-aligned, against the oracle's
    tl = ts.token_logprobs().cpu()
    assert tuple(tl.shape) == (B, L) and (tl[~on] == 0).all()
    print(f"max |token_logprobs − oracle| = {(tl[on].double() - lp[on]).abs().max().item():.3g}")
    with pytest.raises(ValueError):
        bad = q.clone()
        bad[on.nonzero()[0][0], on.nonzero()[0][1]] = float("-inf")
        ts.set_policy_batch(A, bad, ref)
    with pytest.raises(ValueError):
        ts.set_policy_batch(A, q)                                                            # kl_coef set: ref needed


def test_on_policy_ratio_is_one_and_graph_replay_is_bit_identical(dev, tiny):
    from bridgelang_amd.training.policy_loss import STAT_NAMES, PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, _, (ids, mask, labels, pv) = tiny
    ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=PolicyLossConfig(temperature=0.8, entropy_coef=0.01))
    on = labels != -100
    A = torch.where(on, torch.randn(B, L, generator=torch.Generator().manual_seed(2)) + 0.3, torch.zeros(B, L))
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, torch.zeros(B, L))
    ts.forward()
    lp = ts.token_logprobs().clone()
    assert tuple(lp.shape) == (B, L) and bool((lp[on.to(dev)] < 0).all())
    ts.set_policy_batch(A, lp)
    ts.forward()
    st = ts.policy_stats()
    valid = ts.targets != -100
    assert bool((ts.row_stats[valid, 2] == 1.0).all()) and st["ratio"].item() == 1.0 and st["clip_frac"].item() == 0.0
    assert st["approx_kl"].item() == 0.0 and st["n_valid"].item() == int(on.sum())
    # off-policy again, eager vs captured replay
    ts.set_policy_batch(A, lp - 0.3 * torch.sign(A).to(dev))
    eager_loss = ts.forward().item()
    eager = ts.stats.clone()
    ts.backward()
    eager_dl = ts.dlogits.clone()
    for _ in range(2):                                       # the capture, then a replay
        ts.stats.zero_()
        ts.dlogits.zero_()
        loss = ts.forward(graph=True).item()
        ts.backward(graph=True)
        assert loss == eager_loss and torch.equal(ts.stats, eager) and torch.equal(ts.dlogits, eager_dl)
    assert len(STAT_NAMES) == 8 and ts.stats[5].item() > 0


def test_default_loss_is_unchanged(dev):
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    ids, mask, labels, pv = make_batch(dims, B, L)
    out = {}
    for kw in ({}, {"loss": "ce"}):
        w = allocate(dims, dev).fill_synthetic(seed=3)
        ts = TrainStep(w, "vla-train", B, L + 2, **kw)
        ts.set_batch(ids, mask, pv, labels)
        loss = ts.forward()
        ts.backward()
        grads = {n: ts.store.named_grad(n).clone() for n in trainable_names(w, "vla-train")}
        out[bool(kw)] = (loss.item(), grads, [op.name for op in ts.forward_ops], [op.name for op in ts.backward_ops])
        assert not hasattr(ts, "row_stats") and tuple(ts.mean_cnt.shape) == (2,)
    a, b = out[False], out[True]
    assert a[0] == b[0] and a[2] == b[2] and a[3] == b[3]
    assert all(torch.equal(a[1][n], b[1][n]) for n in a[1])
    assert a[2][-1] == "bl_cross_entropy_f32" and a[3][0] == "bl_cross_entropy_backward_f32"
    assert not any(name.startswith("bl_policy_") for name in a[2] + a[3])
    pol = TrainStep(w, "vla-train", B, L + 2, loss="policy")
    fo, bo = [op.name for op in pol.forward_ops], [op.name for op in pol.backward_ops]
    assert fo[:-1] == a[2][:-1] and fo[-1] == "bl_policy_loss_f32"                     # only the loss boundary differs
    assert bo[1:] == a[3][1:] and bo[0] == "bl_policy_loss_backward_f32"
    with pytest.raises(ValueError):
        TrainStep(w, "vla-train", B, L + 2, loss="ppo")


def test_rollout_to_step_end_to_end(dev):
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
    Bp, K, n, temp = 2, 4, 7, 1.3
    ids, pv = make_inputs(model.dims, Bp, 10, seed=31)
    actions, tokens, lp = model.sample_actions(ids.to(dev), pv.to(dev), "bridge_orig", S.SamplingParams(temperature=temp, seed=[5, 6]),
                                               num_samples=K)                          # temperature only
    rewards = -np.abs(actions - 0.1).sum(-1)                                            # synthetic: prefer actions near 0.1
    adv = group_advantages(rewards)
    assert tuple(adv.shape) == (Bp, K) and float(adv.abs().max()) > 0
    batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(Bp * K, n), lp.reshape(Bp * K, n), adv.reshape(-1))
    l = batch["input_ids"].shape[1]
    assert l == 10 + n + 1
    ts = TrainStep(model.weights, "vla-train", Bp * K, l, loss="policy", policy=PolicyLossConfig(temperature=temp))
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv.repeat_interleave(K, 0), batch["labels"])
    ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
    loss, norm = ts.step(1e-3)
    first = {k: v.item() for k, v in ts.policy_stats().items()}
    print("rollout vs training forward:", first)
    assert np.isfinite(loss.item()) and np.isfinite(norm.item()) and norm.item() > 0
    assert first["n_valid"] == Bp * K * n
    ts.forward()
    second = ts.policy_stats()["ratio"].item()
    print("mean ratio after the update:", second)
    assert np.isfinite(second) and second != 1.0 and second != first["ratio"]
