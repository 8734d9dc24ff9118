"""TrainStep(loss="policy", policy=PolicyLossConfig(ratio_level="action")): the action-level importance ratio against
torch.autograd over the CPU oracle's logits, the one op that differs in the plans, the on-policy and graph-replay properties,
and one rollout → step round trip."""
import numpy as np
import pytest
import torch

from oracle import restate as R
from test_train_step_gpu import cos, make_batch

pytestmark = pytest.mark.gpu

B, L = 3, 20


def rows_of(x, fill):
    """[B, L] aligned with the labels → [B, S - 1] aligned with logits[:, :-1] (the oracle's label placement)."""
    full = torch.cat([x[:, :1], torch.full((x.shape[0], 256), fill, dtype=x.dtype), x[:, 1:]], 1)
    return full[:, 1:]


def oracle_logits(sd, dims, ids, mask, pv):
    om = R.OracleModel.from_dims(sd, dims)
    logits, _, _ = om.prefill(ids, pv, attention_mask=mask)
    return logits[:, :-1]                                   # [B, S - 1, vocab]


def restated_action_loss(logits, tg, A, q, ref, cfg):
    """The action-level loss in torch over [B, R, V] logits and [B, R] per-row inputs: one ratio per sequence from the sum
    (or mean) of its labelled tokens' log-ratios, clipped once; entropy and KL per token; a token mean."""
    valid = tg != -100
    lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)
    logp = lsm.gather(2, tg.clamp(min=0)[..., None])[..., 0]
    A, q, ref = A.double(), q.double(), ref.double()
    s = torch.where(valid, logp - q, torch.zeros(()).double()).sum(1)
    n = valid.sum(1)
    if cfg.ratio_norm == "mean":
        s = s / n.clamp(min=1)
    ratio = torch.exp(s)[:, None].expand_as(A)
    lo, hi = 1 - cfg.clip_low, 1 + cfg.clip_high
    pg = -torch.minimum(ratio * A, ratio.clamp(lo, hi) * A)
    H = -(lsm.exp() * lsm).sum(-1)
    d = ref - logp
    kl = torch.exp(d) - d - 1
    row = (pg - cfg.entropy_coef * H + cfg.kl_coef * kl)[valid]
    active = (((A >= 0) & (ratio <= hi)) | ((A < 0) & (ratio >= lo)))[valid]
    sv = s[:, None].expand_as(A)[valid]
    stats = dict(loss=row.mean(), n_valid=valid.sum(), pg=pg[valid].mean(), entropy=H[valid].mean(), kl=kl[valid].mean(),
                 clip_frac=(~active).double().mean(), approx_kl=(torch.expm1(sv) - sv).mean(), ratio=ratio[valid].mean())
    return row.mean(), row, s, logp, stats


@pytest.fixture(scope="module")
def tiny(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    ids, mask, labels, pv = make_batch(dims, B, L)
    return dims, w, sd, (ids, mask, labels, pv)


@pytest.mark.parametrize("norm", ["sum", "mean"])
def test_action_level_gradients_match_autograd(dev, tiny, norm):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    dims, w, sd, (ids, mask, labels, pv) = tiny
    stage = "vla-train"
    cfg = PolicyLossConfig(temperature=0.9, clip_low=0.2, clip_high=0.2, entropy_coef=0.01, kl_coef=0.05, ratio_level="action",
                           ratio_norm=norm)
    sd = {k: v.clone() for k, v in sd.items()}
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    logits = oracle_logits(sd, dims, ids, mask, pv)
    tg = rows_of(labels, -100)
    on = labels != -100
    n_tok = on.sum(1)
    with torch.no_grad():                                   # the oracle's own log π of the labelled tokens, label-aligned
        lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)
        lp_rows = torch.where(tg != -100, lsm.gather(2, tg.clamp(min=0)[..., None])[..., 0], torch.zeros(()).double())
        lp = torch.zeros(B, L, dtype=torch.float64)
        lp[:, 1:] = lp_rows[:, 256:]
    g = torch.Generator().manual_seed(9)
    A = torch.where(on, torch.randn(B, L, generator=g) + 0.5, torch.zeros(B, L))
    # behaviour policy = the oracle's, moved so that the ACTIONS' log-ratios are +0.6 (clipped above), −0.02 (inside) and
    # −0.6 (clipped below): far from log 0.8 / log 1.2 compared with the bf16 noise between the device's and the oracle's log π,
    # which the sum takes n times
    s_want = torch.tensor([0.6, -0.02, -0.6])
    shift = (s_want if norm == "mean" else s_want / n_tok)[:, None].expand(B, L)
    q = torch.where(on, (lp - shift).float(), torch.zeros(B, L))
    ref = torch.where(on, lp.float() + 0.2 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    want, row, s, _, stats = restated_action_loss(logits, tg, rows_of(A, 0.0), rows_of(q, 0.0), rows_of(ref, 0.0), cfg)
    assert (s.detach() - s_want).abs().max() < 1e-4 and 0 < stats["clip_frac"] < 1
    want.backward()

    ts = TrainStep(w, stage, B, L + 2, loss="policy", policy=cfg)          # planned longer than the batch
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, q, ref)
    loss = ts.forward()
    ts.backward()
    got_stats = {k: v.item() for k, v in ts.policy_stats().items()}
    act = {k: v.cpu() for k, v in ts.action_stats().items()}
    scale = row.abs().mean().item()
    print(f"[{norm}] loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |row_loss| {scale:.4f}); stats {got_stats}")
    print("oracle stats", {k: float(v.detach()) for k, v in stats.items()})
    print("action log-ratios", act["log_ratio"].tolist(), "vs", s.detach().tolist())
    assert all(tuple(v.shape) == (B,) for v in act.values()) and torch.equal(act["n"], n_tok.float())
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    assert got_stats["n_valid"] == int(on.sum()) and got_stats["loss"] == loss.item()
    assert got_stats["clip_frac"] == pytest.approx(float(stats["clip_frac"]), abs=1e-6)
    # The token-level file bounds each statistic by 2e-3 (floor 1): one token's log π differs by a bf16-sized ε between the
    # device and the oracle. Entropy and KL are still per token. What depends on the ratio sees the ACTION's log-ratio: under
    # "sum" the n_G token differences add up, so it may be off by n_G·ε and those statistics get n_G times the bound.
    fold = int(n_tok.max()) if norm == "sum" else 1
    for k, times in (("pg", fold), ("entropy", 1), ("kl", 1), ("approx_kl", fold), ("ratio", fold)):
        ref_v = float(stats[k].detach())
        assert abs(got_stats[k] - ref_v) <= 2e-3 * times * max(abs(ref_v), 1.0), k
    worst = 1.0
    for n in names:
        got, ref_g = ts.store.named_grad(n).float().cpu(), sd[n].grad
        sc = ref_g.abs().max().item()
        assert sc > 0, n
        c = cos(got, ref_g)
        worst = min(worst, c)
        err = (got - ref_g).abs().max().item()
        assert c > 0.99 and err <= 0.06 * sc, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {sc:.3g}"
    print(f"worst gradient cosine {worst:.5f}")
    tl = ts.token_logprobs().cpu()                          # token_logprobs() keeps working
    assert tuple(tl.shape) == (B, L) and (tl[~on] == 0).all() and (tl[on] < 0).all()


def test_only_the_loss_op_differs_and_token_level_has_no_action_stats(dev, tiny):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, _, _ = tiny
    with pytest.raises(RuntimeError):
        TrainStep(w, "vla-train", B, L + 2).action_stats()
    for rng in (None, (31744, 256)):
        token = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=PolicyLossConfig(token_range=rng))
        fo, bo = [op.name for op in token.forward_ops], [op.name for op in token.backward_ops]
        assert fo[-1] == ("bl_policy_loss_f32" if rng is None else "bl_policy_loss_range_f32") and not hasattr(token, "group_stats")
        with pytest.raises(RuntimeError):
            token.action_stats()
        for norm in ("sum", "mean"):
            ts = TrainStep(w, "vla-train", B, L + 2, loss="policy",
                           policy=PolicyLossConfig(token_range=rng, ratio_level="action", ratio_norm=norm))
            fa, ba = [op.name for op in ts.forward_ops], [op.name for op in ts.backward_ops]
            assert fa[:-1] == fo[:-1] and fa[-1] == "bl_policy_loss_grouped_f32" and fa.count(fa[-1]) == 1
            assert ba == bo and tuple(ts.group_stats.shape) == (B, 4)


@pytest.mark.parametrize("norm", ["sum", "mean"])
def test_on_policy_ratio_is_one_and_graph_replay_is_bit_identical(dev, tiny, norm):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, _, (ids, mask, labels, pv) = tiny
    labels = labels.clone()
    labels[1] = -100                                         # a sequence without an action: an empty group
    ts = TrainStep(w, "vla-train", B, L + 2, loss="policy",
                   policy=PolicyLossConfig(temperature=0.8, entropy_coef=0.01, ratio_level="action", ratio_norm=norm))
    on = labels != -100
    A = torch.where(on, torch.randn(B, L, generator=torch.Generator().manual_seed(2)) + 0.3, torch.zeros(B, L))
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, torch.zeros(B, L))
    ts.forward()
    lp = ts.token_logprobs().clone()
    ts.set_policy_batch(A, lp)
    ts.forward()
    st, act = ts.policy_stats(), ts.action_stats()
    full = torch.tensor([True, False, True], device=dev)
    assert bool((act["ratio"][full] == 1.0).all()) and bool((act["log_ratio"] == 0.0).all()) and bool((ts.group_stats[1] == 0).all())
    assert act["n"].tolist() == on.sum(1).tolist()
    valid = ts.targets != -100
    assert bool((ts.row_stats[valid, 2] == 1.0).all()) and st["ratio"].item() == 1.0 and st["clip_frac"].item() == 0.0
    assert st["approx_kl"].item() == 0.0 and st["n_valid"].item() == int(on.sum())
    # off-policy again, eager vs captured replay
    ts.set_policy_batch(A, lp - 0.3 * torch.sign(A).to(dev))
    eager_loss = ts.forward().item()
    eager, eager_groups = ts.stats.clone(), ts.group_stats.clone()
    ts.backward()
    eager_dl = ts.dlogits.clone()
    assert bool(torch.isfinite(eager_dl.float()).all()) and bool((eager_groups[full, 1] != 1.0).all())
    for _ in range(2):                                       # the capture, then a replay
        ts.stats.zero_()
        ts.group_stats.zero_()
        ts.dlogits.zero_()
        loss = ts.forward(graph=True).item()
        ts.backward(graph=True)
        assert loss == eager_loss and torch.equal(ts.stats, eager) and torch.equal(ts.group_stats, eager_groups)
        assert torch.equal(ts.dlogits, eager_dl)


def test_rollout_to_action_level_step_end_to_end(dev):
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
    adv = group_advantages(-np.abs(actions - 0.1).sum(-1))                              # synthetic: prefer actions near 0.1
    batch = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(Bp * K, n), lp.reshape(Bp * K, n), adv.reshape(-1))
    l = batch["input_ids"].shape[1]
    ts = TrainStep(model.weights, "vla-train", Bp * K, l, loss="policy", policy=PolicyLossConfig(temperature=temp, ratio_level="action"))
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv.repeat_interleave(K, 0), batch["labels"])
    ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
    loss = ts.forward()
    act = {k: v.cpu() for k, v in ts.action_stats().items()}
    tl = ts.token_logprobs().cpu()
    on = batch["labels"] != -100
    per_seq = torch.where(on, tl.double(), torch.zeros(()).double()).sum(1)
    print("action ratios, rollout vs training forward:", act["ratio"].tolist())
    assert np.isfinite(loss.item()) and bool((act["n"] == n).all()) and bool(torch.isfinite(act["ratio"]).all())
    assert (act["logp"].double() - per_seq).abs().max() <= 1e-5
    # the action's log-ratio is its log π minus the rollout's: the sum of the n reported log-probabilities
    old = torch.where(on, batch["old_logprobs"].double(), torch.zeros(()).double()).sum(1)
    assert (act["log_ratio"].double() - (per_seq - old)).abs().max() <= 1e-4
    loss2, norm = ts.step(1e-3)
    assert np.isfinite(loss2.item()) and np.isfinite(norm.item()) and norm.item() > 0
