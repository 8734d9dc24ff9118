"""TrainStep(loss="policy") with the rollout correction (PolicyLossConfig.rollout_is_cap): the step with μ = old_logprobs
against the same step without the correction, bit for bit; a weighted step's dlogits against the specification over the
step's own logits, and graph replay; self-proximal against the explicit proximal policy; the unchanged plans; and one closed
loop from an e4m3 rollout under LoRA adapters to a corrected step. Bounds are those of tests/test_action_ratio_gpu.py
(helpers copied, not imported)."""
import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import IS_STAT_NAMES, STAT_NAMES, PolicyLossConfig, policy_loss
from test_train_step_gpu import make_batch

pytestmark = pytest.mark.gpu

B, L = 3, 20
CAP, MASK = 1.5, (0.5, 3.0)
# per unit (a labelled token at token level, a sequence at action level), in turn: π_θ/π_prox and π_prox/μ wanted. With cap
# 1.5 and mask (0.5, 3): truncated, masked above, untouched, masked below, untouched
RATIOS, RHOS = (1.6, 0.5, 1.1, 0.7, 1.0), (2.0, 4.0, 0.8, 0.3, 1.2)
LEVELS = [("token", "sum"), ("action", "sum"), ("action", "mean")]
BASE = dict(temperature=0.9, clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.05)


def grad_close(got, ref, what, tol):
    got, ref = got.float().cpu(), ref.float()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def scalars_close(got, ref, what):
    """The project's bound on loss scalars, per value: 1e-4 of max(|ref|, 1)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.abs(got - ref) > 1e-4 * np.maximum(np.abs(ref), 1.0)
    assert not bad.any(), f"{what}: got {got[bad][:4]} vs {ref[bad][:4]} at {np.argwhere(bad)[:4].ravel()}"


@pytest.fixture(scope="module")
def batch():
    from bridgelang_amd.weights import tiny_dims
    ids, mask, labels, pv = make_batch(tiny_dims(), B, L)
    on = labels != -100
    # Every unpadded token of the batch is a different one. The embedding gradient is accumulated with float atomics
    # (embed_bwd_kernel: dW[id] += dx), so it has the same bits in two backward passes only where no embedding row gets
    # three or more non-zero terms — and every sequence of make_batch starts with token 1. The bit-for-bit comparisons of
    # "every gradient buffer" below are over a batch on which every gradient IS reproducible.
    for b in range(B):
        for j in range(int(mask[b].sum())):
            ids[b, j] = 31744 + (11 * (8 * b + int(on[b, :j].sum()))) % 256 if on[b, j] else 100 + b * L + j
    labels = torch.where(on, ids, labels)
    assert len(set(ids[mask].tolist())) == int(mask.sum()) and int(on.sum()) == 8 * B
    g = torch.Generator().manual_seed(9)
    A = torch.where(on, torch.randn(B, L, generator=g) + 0.5, torch.zeros(B, L))
    noise = torch.where(on, 0.2 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    return ids, mask, labels, pv, on, A, noise


def fresh_weights(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    return allocate(tiny_dims(), dev).fill_synthetic(seed=3)


def placed(lp, on, level, norm, given=True):
    """q and μ [B, L] from the step's own log π `lp`, so that unit k has the ratio and the ρ wanted in its turn."""
    q, mu = lp.clone(), lp.clone()
    k = 0
    for b in range(B):
        pos = on[b].nonzero()[:, 0]
        for unit in ([pos] if level == "action" else [p[None] for p in pos]):
            share = 1 if (norm == "mean" or level == "token") else len(unit)
            if given:
                q[b, unit] -= float(np.log(RATIOS[k % 5])) / share
            mu[b, unit] = q[b, unit] - float(np.log(RHOS[k % 5])) / share
            k += 1
    return (q if given else None), mu


def specification(ts, cfg, self_proximal=False):
    """The fp64 specification over the step's own logits and its own per-row inputs. Only the labelled rows go in: every
    sequence's labelled rows in order, padded with ignored rows to the longest, which keeps every group and every row-order
    sum. → (result, the rows picked, in the order of the result's valid rows)."""
    S = ts.S
    tg = ts.targets.cpu().view(B, S)
    m = int((tg != -100).sum(1).max())
    pick = [(tg[b] != -100).nonzero()[:, 0] + b * S for b in range(B)]
    rows = torch.cat(pick)
    n = ts.logits.shape[1]
    logits, targets = np.zeros((B * m, n)), np.full(B * m, -100, dtype=np.int64)
    per_row = {k: np.zeros(B * m) for k in ("advantages", "old_logprob", "ref_logprob", "behaviour_logprob")}
    for b, p in enumerate(pick):
        sl = slice(b * m, b * m + len(p))
        logits[sl] = ts.logits[p.to(ts.logits.device)].double().cpu().numpy()
        targets[sl] = ts.targets.cpu()[p].numpy()
        for k in per_row:
            per_row[k][sl] = getattr(ts, k).cpu()[p].double().numpy()
    res = policy_loss(logits, targets, per_row["advantages"], None if self_proximal else per_row["old_logprob"],
                      per_row["ref_logprob"] if cfg.kl_coef else None, cfg, group_rows=m,
                      behaviour_logprobs=per_row["behaviour_logprob"])
    return res, rows


def check_clear_and_mixed(want, cfg):
    v = want.valid
    rho = np.exp(want.log_rho[v])
    for bound in (cfg.rollout_is_cap,) + tuple(cfg.rollout_is_mask or ()):
        if 0 < bound < np.inf:
            assert (np.abs(rho / bound - 1) >= 1e-3).all(), bound
    assert want.truncated.any() and (v & ~want.masked & ~want.truncated).any()
    assert bool(want.masked.any()) == (cfg.rollout_is_mask is not None)


@pytest.mark.parametrize("level,norm", LEVELS)
def test_behaviour_equal_to_proximal_is_the_uncorrected_step_bit_for_bit(dev, batch, level, norm):
    from bridgelang_amd.training.step import TrainStep, trainable_names
    ids, mask, labels, pv, on, A, noise = batch
    out = {}
    for corrected in (False, True):
        w = fresh_weights(dev)
        cfg = PolicyLossConfig(ratio_level=level, ratio_norm=norm, rollout_is_cap=2.0 if corrected else None, **BASE)
        ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=cfg)
        ts.set_batch(ids, mask, pv, labels)
        extra = dict(behaviour_logprobs=torch.zeros(B, L)) if corrected else {}
        ts.set_policy_batch(A, torch.zeros(B, L), torch.zeros(B, L), **extra)
        ts.forward()
        lp = ts.token_logprobs().cpu()
        q, _ = placed(lp, on, level, norm)
        extra = dict(behaviour_logprobs=q) if corrected else {}
        ts.set_policy_batch(A, q, lp + noise, **extra)
        loss, norm_ = ts.step(1e-3)
        names = trainable_names(w, "vla-train")
        out[corrected] = (loss.item(), norm_.item(), ts.stats.clone(), ts.row_stats.clone(), ts.dlogits.clone(),
                          {n: ts.store.named_grad(n).clone() for n in names}, {k: v.clone() for k, v in w.state_dict().items()})
        if corrected:
            assert ts.is_stats.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
            tw = ts.token_weights().cpu()
            assert tuple(tw.shape) == (B, L) and (tw[on] == 1).all() and (tw[~on] == 0).all()
        else:
            assert 0 < ts.stats[5].item() < 1                                  # a case that exercises the clip
    a, b = out[False], out[True]
    assert a[0] == b[0] and a[1] == b[1] and all(torch.equal(a[i], b[i]) for i in (2, 3, 4))
    assert all(torch.equal(a[5][n], b[5][n]) for n in a[5]) and len(a[5]) > 0
    assert all(torch.equal(a[6][k], b[6][k]) for k in a[6])


@pytest.mark.parametrize("level,norm", LEVELS)
def test_weighted_step_matches_specification_and_graph_replay_is_bit_identical(dev, batch, level, norm):
    from bridgelang_amd.training.step import TrainStep
    ids, mask, labels, pv, on, A, noise = batch
    cfg = PolicyLossConfig(ratio_level=level, ratio_norm=norm, rollout_is_cap=CAP, rollout_is_mask=MASK, **BASE)
    ts = TrainStep(fresh_weights(dev), "vla-train", B, L + 2, loss="policy", policy=cfg)
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, None, torch.zeros(B, L), behaviour_logprobs=torch.zeros(B, L))
    ts.forward()                                            # the step's own logits and log π, to place q and μ from
    logits0 = ts.logits.clone()
    lp = ts.token_logprobs().cpu()
    q, mu = placed(lp, on, level, norm)
    ts.set_policy_batch(A, q, lp + noise, behaviour_logprobs=mu)
    want, rows = specification(ts, cfg)
    check_clear_and_mixed(want, cfg)                        # on the specification alone
    v = want.valid
    assert want.clipped.any() and (v & ~want.clipped).any()
    loss = ts.forward().item()
    ts.backward()
    assert torch.equal(ts.logits, logits0)
    st, ist = ts.stats.cpu().numpy(), ts.is_stats.cpu().numpy()
    got_w = ts.is_rows[rows.to(dev), 1].cpu().numpy()
    print(f"[{level} {norm}] loss {loss:.6f} vs {want.loss:.6f}; rollout statistics {ist[:6]} vs {want.is_stats[:6]}")
    scalars_close(st, want.stats, "step statistics")
    scalars_close(ist, want.is_stats, "rollout statistics")
    assert {k: v_.item() for k, v_ in ts.rollout_stats().items()} == dict(zip(IS_STAT_NAMES, ist[:6].tolist()))
    scalars_close(got_w, want.weight[v], "w")
    assert np.array_equal(got_w == 0, want.masked[v]) and np.array_equal(got_w == np.float32(CAP), want.truncated[v])
    assert np.array_equal(ts.row_stats[rows.to(dev), 4].cpu().numpy(), want.clipped[v].astype(np.float32))
    tw = ts.token_weights().cpu()
    assert tuple(tw.shape) == (B, L) and np.array_equal(tw[on].numpy(), got_w) and (tw[~on] == 0).all()
    dl = ts.dlogits.float().cpu()
    grad_close(dl[rows], torch.from_numpy(want.dlogits[v]), "dlogits", 1e-2)
    ignored = torch.ones(dl.shape[0], dtype=torch.bool)
    ignored[rows] = False
    assert (dl[ignored] == 0).all() and (ts.is_rows.cpu()[ignored] == 0).all()
    eager = [t.clone() for t in (ts.stats, ts.is_stats, ts.is_rows, ts.row_stats, ts.dlogits)]
    for _ in range(2):                                       # the capture, then a replay
        for t in (ts.stats, ts.is_stats, ts.is_rows, ts.dlogits):
            t.zero_()
        assert ts.forward(graph=True).item() == loss
        ts.backward(graph=True)
        assert all(torch.equal(x, y) for x, y in zip(eager, (ts.stats, ts.is_stats, ts.is_rows, ts.row_stats, ts.dlogits)))


@pytest.mark.parametrize("level,norm", LEVELS)
def test_self_proximal_is_the_explicit_proximal_policy_bit_for_bit(dev, batch, level, norm):
    from bridgelang_amd.training.step import TrainStep, trainable_names
    ids, mask, labels, pv, on, A, noise = batch
    cfg = PolicyLossConfig(ratio_level=level, ratio_norm=norm, rollout_is_cap=CAP, rollout_is_mask=MASK, **BASE)
    w = fresh_weights(dev)
    ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=cfg)
    names = trainable_names(w, "vla-train")
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, None, torch.zeros(B, L), behaviour_logprobs=torch.zeros(B, L))
    ts.forward(graph=True)                                  # the self-proximal plan's graph; the explicit form below has its own
    lp = ts.token_logprobs().clone()
    _, mu = placed(lp.cpu(), on, level, norm, given=False)
    ref = lp.cpu() + noise
    ts.set_policy_batch(A, None, ref, behaviour_logprobs=mu)
    want, _ = specification(ts, cfg, self_proximal=True)
    check_clear_and_mixed(want, cfg)
    out = []
    for old in (None, lp):                                  # self-proximal, then forward() → token_logprobs() → old_logprobs
        ts.set_policy_batch(A, old, ref, behaviour_logprobs=mu)
        ts.forward(graph=True)
        ts.backward()
        st = ts.policy_stats()
        assert st["ratio"].item() == 1.0 and st["clip_frac"].item() == 0.0 and st["approx_kl"].item() == 0.0
        assert sorted(ts._graphs) == (["fwd_self"] if old is None else ["fwd", "fwd_self"])       # one graph per plan, none dropped
        out.append((ts.stats.clone(), ts.is_stats.clone(), ts.is_rows.clone(), ts.row_stats.clone(), ts.dlogits.clone(),
                    {n: ts.store.named_grad(n).clone() for n in names}))
    a, b = out
    assert all(torch.equal(a[i], b[i]) for i in range(5)) and all(torch.equal(a[5][n], b[5][n]) for n in names)
    scalars_close(a[1].cpu().numpy(), want.is_stats, "rollout statistics")
    wts = a[2][:, 1]
    assert bool((wts == CAP).any()) and bool((wts[ts.targets != -100] == 0).any())


def test_plans_and_batch_validation(dev, batch):
    from bridgelang_amd.training.step import TrainStep
    ids, mask, labels, pv, on, A, noise = batch
    w = fresh_weights(dev)
    z = torch.zeros(B, L)
    plans = {}
    for key, kw in (("token", {}), ("range", dict(token_range=(0, 32064))), ("action", dict(ratio_level="action"))):
        plain = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=PolicyLossConfig(**kw))
        fixed = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=PolicyLossConfig(rollout_is_cap=2.0, **kw))
        fo, bo = [op.name for op in plain.forward_ops], [op.name for op in plain.backward_ops]
        plans[key] = fo[-1]
        assert "bl_policy_loss_is_f32" not in fo + bo and not hasattr(plain, "is_rows")
        assert [op.name for op in fixed.forward_ops] == fo[:-1] + ["bl_policy_loss_is_f32"]       # only the forward's loss op differs
        assert [op.name for op in fixed.forward_ops_self] == fo[:-1] + ["bl_policy_loss_is_f32"] and not hasattr(plain, "forward_ops_self")
        assert fixed.forward_ops_self[:-1] == fixed.forward_ops[:-1]                              # … and the two proximal modes share the rest
        assert fixed.forward_ops[-1].args[7] is not None and fixed.forward_ops_self[-1].args[7] is None      # old_logprob: given / NULL
        assert [op.name for op in fixed.backward_ops] == bo
    assert plans == {"token": "bl_policy_loss_f32", "range": "bl_policy_loss_range_f32", "action": "bl_policy_loss_grouped_f32"}
    plain.set_batch(ids, mask, pv, labels)
    fixed.set_batch(ids, mask, pv, labels)
    with pytest.raises(ValueError, match="behaviour_logprobs"):
        plain.set_policy_batch(A, z, behaviour_logprobs=z)
    with pytest.raises(ValueError, match="self-proximal"):
        plain.set_policy_batch(A, None)
    with pytest.raises(RuntimeError):
        plain.rollout_stats()
    with pytest.raises(RuntimeError):
        plain.token_weights()
    with pytest.raises(ValueError, match="behaviour_logprobs"):
        fixed.set_policy_batch(A, z)
    bad = z.clone()
    bad[on.nonzero()[0][0], on.nonzero()[0][1]] = float("-inf")
    with pytest.raises(ValueError, match="behaviour_logprobs"):
        fixed.set_policy_batch(A, None, behaviour_logprobs=bad)
    with pytest.raises(ValueError):
        fixed.set_policy_batch(A, z, behaviour_logprobs=z[:, :-1])
    fixed.set_policy_batch(A, None, behaviour_logprobs=torch.where(on, z, torch.full_like(z, float("nan"))))      # off the labels: not read
    assert list(fixed.rollout_stats()) == list(IS_STAT_NAMES) and len(STAT_NAMES) == 8


def test_e4m3_rollout_to_corrected_step_end_to_end(dev):
    """sample_actions through the e4m3 prefill under LoRA adapters → policy_batch(rollout_is=True) → one self-proximal step:
    what the learner's first update sees of the rollout engine's numerics (printed)."""
    from bridgelang_amd import sampling as S
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.rl import group_advantages, policy_batch
    from bridgelang_amd.training.step import TrainStep
    from test_engine_gpu import make_inputs
    from test_lora_inference_gpu import new_model
    model = new_model(dev)
    Bp, K, n, cap = 2, 8, 7, 2.0
    ids, pv = make_inputs(model.dims, Bp, 10, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    rng = model.action_token_range()
    lora = LoraAdapters(model.weights, r=8)
    model.attach_adapters(lora, fp8=True)
    model.fp8 = True
    try:
        actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", S.SamplingParams(temperature=1.0, seed=[5, 6]), num_samples=K,
                                                   action_tokens_only=True)
        adv = group_advantages(-np.abs(actions - 0.1).sum(-1))
        b = policy_batch(ids.repeat_interleave(K, 0), None, tokens.reshape(Bp * K, n), lp.reshape(Bp * K, n), adv.reshape(-1),
                         token_range=rng, rollout_is=True)
        assert "old_logprobs" not in b
        cfg = PolicyLossConfig(temperature=1.0, token_range=rng, rollout_is_cap=cap, rollout_is_mask=(0.25, 4.0))
        ts = TrainStep(model.weights, "lora", Bp * K, b["input_ids"].shape[1], lora=lora, loss="policy", policy=cfg,
                       max_grad_norm=float("inf"), refresh_adapted=True)
        ts.set_batch(b["input_ids"], b["attention_mask"], pv.repeat_interleave(K, 0), b["labels"])
        ts.set_policy_batch(b["advantages"], b.get("old_logprobs"), behaviour_logprobs=b["behaviour_logprobs"])
        loss, norm = ts.step(0.05)
        stats = {k: v.item() for k, v in ts.rollout_stats().items()}
        wts = ts.token_weights().cpu()
        on = b["labels"] != -100
        print(f"\ne4m3 rollout vs the bf16 training forward under LoRA, {int(on.sum())} tokens: {stats}; "
              f"max |λ| {ts.is_rows[:, 0].abs().max().item():.5f}")
        assert np.isfinite(loss.item()) and np.isfinite(norm.item()) and norm.item() > 0
        assert all(np.isfinite(v) for v in stats.values()) and ts.policy_stats()["ratio"].item() == 1.0
        assert bool((wts >= 0).all()) and bool((wts <= cap).all()) and bool((wts[on] > 0).any()) and (wts[~on] == 0).all()
        assert ts.policy_stats()["n_valid"].item() == Bp * K * n
    finally:
        model.fp8 = False
        model.detach_adapters()
