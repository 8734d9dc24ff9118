"""TrainStep(loss="policy", value=ValueLossConfig(...)): the critic inside the policy step against torch.autograd over the
CPU oracle (value = the oracle's final-norm output times the head), against the fp64 definition on the device's own hn, and
its plan / optimizer / graph / collective / option properties. The tiny model, B = 3, L = 20, as test_policy_step_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import restate as R
from test_policy_step_gpu import restated_loss, rows_of
from test_train_step_gpu import cos, make_batch
from test_value_head_gpu import value_tolerances

pytestmark = pytest.mark.gpu

B, L = 3, 20
CLIP = 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    return dims, w, sd, make_batch(dims, B, L)


def fresh_weights(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    return allocate(tiny_dims(), dev).fill_synthetic(seed=3)


def drawn_head(dims, dev, seed=4):
    from bridgelang_amd.training.value_head import ValueHead
    vh = ValueHead(dims.llm_dim, dev, init_std=0.02, seed=seed)
    vh.bias.fill_(0.125)
    return vh


def spread(v, on, c, dist=0.2, seed=6):
    """Returns and old values around given values `v` (label- or sequence-aligned): v − vo cycles through ±0.5c and ±2c, R
    lies dist … 3·dist from v, so both branches of the max are taken and none is within reach of bf16 noise (outside the
    range |e| and |ec| differ by c whenever dist >= c). R lies above v three times out of four: with as many returns below
    as above, the bias gradient Σ dv would be a cancelling sum, whose own size is no scale to measure an error against.
    `dist` sets the conditioning of the LOSS comparison: ½e² moves by e·Δv under the forward's bf16 noise Δv ≈ 2^-8·|v| ≈ 3e-3
    of the value (|v| < 1 here), i.e. by 2Δv / |e| of itself; the critic-only case, whose whole loss is the value loss, takes
    returns 4 … 12 away (a fresh critic against undiscounted returns), where that is below the file's 2e-3."""
    k = (torch.arange(v.numel()) % 8).view(v.shape)
    off = torch.tensor([0.5, 2.0, -2.0, -0.5, 2.0, -2.0, 0.5, -0.5])[k] * c
    side = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0, -1.0])[k]
    m = dist * (1.0 + 2.0 * torch.rand(v.shape, generator=torch.Generator().manual_seed(seed)))
    z = torch.zeros_like(v)
    return torch.where(on, v + side * m, z), torch.where(on, v - off, z)


def definition_on_device(ts, inv_world=1.0):
    """The fp64 definition evaluated on what the device's kernels read: ts.hn, the live head, the step's row inputs."""
    from bridgelang_amd.training.value_loss import value_loss
    vh, cfg = ts.value_head, ts.value
    hn = ts.hn.float().cpu().double().numpy()
    Rr, vo = ts.returns.cpu().double().numpy(), ts.old_values.cpu().double().numpy()
    ref = value_loss(hn, ts.targets.cpu().numpy(), vh.weight.float().cpu().double().numpy(), float(vh.bias.float().item()), Rr,
                     vo if cfg.clip is not None else None, cfg, group_rows=ts.S, policy_loss=float(ts.stats[0].item()), inv_world=1.0)
    idx = ref.index
    tol, tdv, _ = value_tolerances(hn[idx], vh.weight.float().cpu().double().numpy(), float(vh.bias.float().item()), Rr[idx],
                                   vo[idx] if cfg.clip is not None else None, ref, cfg.coef, inv_world, float(ts.stats[0].item()))
    return ref, tol


def check_head_against_definition(ts, backward=True):
    """values(), the statistics and (after a backward pass) the head's gradients within the kernel test's derived bounds."""
    ref, tol = definition_on_device(ts)
    idx = ref.index
    got = ts.value_rows.cpu().double().numpy()
    assert (np.abs(got[idx, 0] - ref.value[idx]) <= tol["v"] + 2.0 ** -116).all()
    assert np.array_equal(ts.value_index.cpu().numpy()[:len(idx)], idx) and int(ts.value_count.item()) == len(idx)
    stats = ts.vstats.cpu().double().numpy()
    assert np.isfinite(stats).all() and (np.abs(stats - ref.stats) <= tol["stats"] + 2.0 ** -116).all(), (stats, ref.stats)
    if backward:
        dw = ts.store.grad_view("value_head.weight").cpu().double().numpy()
        db = float(ts.store.grad_view("value_head.bias")[0].item())
        assert (np.abs(dw - ref.dw) <= tol["dw"] + 2.0 ** -116).all() and abs(db - ref.db) <= tol["db"] + 2.0 ** -116
    return ref


GRAD_CASES = [("vla-train", "token", False), ("lora", "action", False), ("vla-train", "action", True)]


@pytest.mark.parametrize("stage,level,zero_adv", GRAD_CASES, ids=[f"{s}-{l}" + ("-critic-only" if z else "") for s, l, z in GRAD_CASES])
def test_gradients_match_autograd(dev, tiny, stage, level, zero_adv):
    """Policy loss + coef · value loss through the whole model against autograd over the oracle; with all advantages 0 (and no
    entropy / KL term) every trunk gradient comes through the value path alone and must meet the same thresholds."""
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, _, sd0, (ids, mask, labels, pv) = tiny
    w = fresh_weights(dev)
    cfg = PolicyLossConfig(temperature=0.9, entropy_coef=0.0 if zero_adv else 0.01)
    vcfg = ValueLossConfig(coef=0.5, clip=CLIP, level=level)
    vh = drawn_head(dims, dev)
    lora = mods = None
    sd = {k: v.clone() for k, v in sd0.items()}
    if stage == "lora":
        from bridgelang_amd.training.lora import LoraAdapters
        from test_lora_gpu import effective_sd, random_adapters
        lora = LoraAdapters(w, r=32)
        ad_sd = random_adapters(lora, seed=7)
        lora.load_state_dict(ad_sd)
        mods = [m for ad in lora.adapters for m in ad.modules]
        params = {k: v.clone().requires_grad_(True) for k, v in ad_sd.items()}
        model_sd = effective_sd(sd, params, lora.scaling, mods)
    else:
        params = {n: sd[n].requires_grad_(True) for n in trainable_names(w, stage)}
        model_sd = sd
    ts = TrainStep(w, stage, B, L + 2, loss="policy", policy=cfg, value=vcfg, value_head=vh, lora=lora)
    assert ts.value_head is vh
    on = labels != -100
    by_action = level == "action"
    # ---- first forward: the device's own values and log π, which the batch is then built around ----
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(torch.zeros(B, L), torch.zeros(B, L))
    ts.set_value_batch(torch.zeros(B) if by_action else torch.zeros(B, L), torch.zeros(B) if by_action else torch.zeros(B, L))
    ts.forward()
    v_dev, lp_dev = ts.values().cpu(), ts.token_logprobs().cpu()
    assert tuple(v_dev.shape) == ((B,) if by_action else (B, L)) and (by_action or bool((v_dev[~on] == 0).all()))
    Rt, vo = spread(v_dev, torch.ones(B, dtype=torch.bool) if by_action else on, CLIP, dist=4.0 if zero_adv else 0.2)
    g = torch.Generator().manual_seed(9)
    A = torch.zeros(B, L) if zero_adv else torch.where(on, torch.randn(B, L, generator=g) + 0.5, torch.zeros(B, L))
    shift = torch.tensor([0.5, -0.05, 0.05, -0.5, 0.0])[torch.arange(B * L) % 5].view(B, L)
    q = torch.where(on, lp_dev - shift, torch.zeros(B, L))
    ts.set_policy_batch(A, q)
    ts.set_value_batch(Rt, vo)
    loss = ts.forward()
    ts.backward()
    assert loss.item() == ts.value_stats()["total"].item()
    ref_dev = check_head_against_definition(ts)
    # ---- the oracle: logits and the final-norm output, the same loss in torch ----
    om = R.OracleModel.from_dims(model_sd, dims)
    trace = {}
    logits, _, _ = om.prefill(ids, pv, attention_mask=mask, trace=trace)
    hn_o = R.rmsnorm(R.Prec(True, "blas"), trace["llm"][-1], model_sd["language_model.model.norm.weight"].float(), dims.rms_eps)
    w_h = vh.weight.float().cpu().clone().requires_grad_(True)
    b_h = vh.bias.float().cpu().clone().requires_grad_(True)
    tg = rows_of(labels, -100).reshape(-1)
    pol, row, ratio, _, pstats = restated_loss(logits[:, :-1].reshape(-1, dims.vocab), tg, rows_of(A, 0.0).reshape(-1),
                                               rows_of(q, 0.0).reshape(-1), torch.zeros(tg.shape[0]), cfg)
    v_all = (hn_o[:, :-1] @ w_h + b_h)                              # [B, S − 1], aligned with the rows
    valid = (tg != -100).view(B, -1)
    if by_action:
        sel = torch.zeros_like(valid)
        sel[torch.arange(B), valid.float().argmax(dim=1)] = True
        R_rows, vo_rows = Rt[:, None].expand_as(valid), vo[:, None].expand_as(valid)
    else:
        sel, R_rows, vo_rows = valid, rows_of(Rt, 0.0), rows_of(vo, 0.0)
    v_o, R_o, vo_o = v_all[sel].double(), R_rows[sel].double(), vo_rows[sel].double()
    e = v_o - R_o
    ec = vo_o + (v_o - vo_o).clamp(-CLIP, CLIP) - R_o
    l = 0.5 * torch.maximum(e * e, ec * ec)
    want = pol + vcfg.coef * l.mean()
    # no row of the oracle's is within bf16 noise of a branch change either
    d_o = (v_o - vo_o).detach().abs()
    outside = d_o > CLIP
    assert ((d_o - CLIP).abs().min() > 0.05) and ((e.detach().abs() - ec.detach().abs()).abs()[outside].min() > 0.05)
    clipped_o = (ec * ec > e * e).detach()
    assert 0 < clipped_o.double().mean() < 1
    if not zero_adv:
        assert ((ratio - 0.8).abs().min() > 0.03) and ((ratio - 1.2).abs().min() > 0.03)
    want.backward()
    got_v = torch.from_numpy(ref_dev.value[ref_dev.index])
    print(f"max |values() − oracle value| = {(ts.value_rows[:, 0].cpu()[torch.from_numpy(ref_dev.index)].double() - v_o.detach()).abs().max().item():.3g} "
          f"(|v| up to {got_v.abs().max().item():.3g})")
    scale = row.detach().abs().mean().item() + vcfg.coef * l.detach().mean().item()
    vs = {k: v.item() for k, v in ts.value_stats().items()}
    print(f"total {loss.item():.6f} vs oracle {want.item():.6f} (scale {scale:.4f}); value stats {vs}")
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    assert vs["n"] == int(sel.sum()) and vs["clip_frac"] == pytest.approx(float(clipped_o.double().mean()), abs=1e-6)
    if zero_adv:
        assert not bool(ts.dlogits.any())                          # the policy path contributes exactly nothing
    # ---- every trainable tensor, and the head's two ----
    if lora is not None:
        got = lora.state_dict({u.key: ts.store.grad_view(u).reshape(-1) for u in ts.store.units if u.key.startswith("lora.")})
    else:
        got = {n: ts.store.named_grad(n).float().cpu() for n in params}
    got["value_head.weight"], params["value_head.weight"] = ts.store.grad_view("value_head.weight").cpu(), w_h
    got["value_head.bias"], params["value_head.bias"] = ts.store.grad_view("value_head.bias")[:1].cpu(), b_h
    worst = 1.0
    for n, p in params.items():
        gg, ref_g = got[n].float().cpu(), p.grad
        s = ref_g.abs().max().item()
        if zero_adv and n == "language_model.lm_head.weight":      # not on the value path: no gradient at all
            assert s == 0 and not bool(gg.any())
            continue
        assert s > 0, n
        c = cos(gg, ref_g)
        worst = min(worst, c)
        err = (gg - ref_g).abs().max().item()
        assert c > 0.99 and err <= 0.06 * s, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {s:.3g}"
    print(f"worst gradient cosine {worst:.5f} over {len(params)} tensors")
    with pytest.raises(ValueError):
        ts.set_value_batch(Rt)                                     # clip set: old values needed
    with pytest.raises(ValueError):
        bad = Rt.clone()
        bad[(0,) if by_action else tuple(on.nonzero()[0])] = float("nan")
        ts.set_value_batch(bad, vo)
    with pytest.raises(ValueError):
        ts.set_value_batch(Rt[:-1], vo[:-1])


def policy_inputs(labels, seed=2):
    on = labels != -100
    A = torch.where(on, torch.randn(B, L, generator=torch.Generator().manual_seed(seed)) + 0.3, torch.zeros(B, L))
    return on, A, torch.where(on, torch.full((B, L), -5.0), torch.zeros(B, L))


def value_inputs(level, seed=3):
    g = torch.Generator().manual_seed(seed)
    shape = (B,) if level == "action" else (B, L)
    return torch.randn(shape, generator=g), 0.3 * torch.randn(shape, generator=g)


def test_detach_leaves_the_trunk_alone(dev, tiny):
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, w, _, (ids, mask, labels, pv) = tiny
    on, A, q = policy_inputs(labels)
    Rt, vo = value_inputs("token")
    names = trainable_names(w, "vla-train")
    grads = {}
    for mode in ("none", "attached", "detached"):
        kw = {} if mode == "none" else dict(value=ValueLossConfig(level="token", detach=mode == "detached"), value_head=drawn_head(dims, dev))
        ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", **kw)
        ts.set_batch(ids, mask, pv, labels)
        ts.set_policy_batch(A, q)
        if mode != "none":
            ts.set_value_batch(Rt, vo)
        ts.forward()
        ts.backward()
        grads[mode] = {n: ts.store.named_grad(n).clone() for n in names}
        if mode != "none":
            grads[mode]["head"] = (ts.store.grad_view("value_head.weight").clone(), ts.store.grad_view("value_head.bias").clone())
            assert bool(grads[mode]["head"][0].any())
    for n in names:
        assert torch.equal(grads["detached"][n], grads["none"][n]), n
    assert any(not torch.equal(grads["attached"][n], grads["none"][n]) for n in names)
    assert all(torch.equal(a, b) for a, b in zip(grads["attached"]["head"], grads["detached"]["head"]))


def test_off_means_off(dev, tiny):
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, w, _, _ = tiny
    names = lambda ts: ([op.name for op in ts.forward_ops], [op.name for op in ts.backward_ops])
    fo, bo = names(TrainStep(w, "vla-train", B, L + 2, loss="policy"))
    off = TrainStep(w, "vla-train", B, L + 2, loss="policy", value=None, value_head=None)
    assert names(off) == (fo, bo) and off.value_head is None and not hasattr(off, "value_rows")
    assert fo[-1] == "bl_policy_loss_f32" and bo[0] == "bl_policy_loss_backward_f32"
    assert not any(n.startswith("bl_value_") for n in fo + bo)
    assert {u.key for u in off.store.units}.isdisjoint({"value_head.weight", "value_head.bias"})
    for kw in (dict(), dict(detach=True)):
        on = TrainStep(w, "vla-train", B, L + 2, loss="policy", value=ValueLossConfig(**kw))
        fv, bv = names(on)
        assert fv == fo + ["bl_value_head_f32"]
        i = bv.index("bl_value_head_backward_f32")
        assert bv[:i] + bv[i + 1:] == bo and i == bo.index("bl_rmsnorm_backward_bf16")     # right ahead of the final norm's backward
        assert not on.value_head.weight.any() and tuple(on.value_head.weight.shape) == (dims.llm_dim,)      # created, zero
    with pytest.raises(ValueError):
        TrainStep(w, "vla-train", B, L + 2, value=ValueLossConfig())                      # the critic trains with loss="policy"
    with pytest.raises(ValueError):
        TrainStep(w, "vla-train", B, L + 2, loss="policy", value_head=drawn_head(dims, dev))
    from bridgelang_amd.training.step import ParamStore
    with pytest.raises(ValueError):                                                       # a caller's store must carry the head
        TrainStep(w, "vla-train", B, L + 2, loss="policy", value=ValueLossConfig(), store=ParamStore(w, "vla-train", defer_grads=True))
    with pytest.raises(RuntimeError):
        off.values()
    with pytest.raises(RuntimeError):
        off.set_value_batch(torch.zeros(B))


def test_optimizer_picks_the_head_up(dev, tiny):
    """Adam's first step from a zero head: every master moves by lr against the sign of its gradient (weight decay acts on
    zeros), and the live bf16 tensors are the rounded masters."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, _, _, (ids, mask, labels, pv) = tiny
    w = fresh_weights(dev)
    lr, eps = 1e-3, 1e-8
    ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", value=ValueLossConfig(level="token"), max_grad_norm=1e9, weight_decay=0.1,
                   eps=eps)
    on, A, q = policy_inputs(labels)
    Rt, _ = value_inputs("token")
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, q)
    ts.set_value_batch(Rt, torch.zeros(B, L))                      # v = vo = 0: inside the clip range
    ts.forward()
    ts.backward()
    g = {n: ts.store.grad_view(n).double().cpu().clone() for n in ("value_head.weight", "value_head.bias")}
    ts.clip_grad_norm()
    ts.optimizer_step(lr)
    masters = ts.store.master_state_dict()
    for n, live in (("value_head.weight", ts.value_head.weight), ("value_head.bias", ts.value_head.bias)):
        m, gn = masters[n].double().cpu().reshape(-1), g[n].reshape(-1)
        big = gn.abs() > 1e-3 * gn.abs().max()
        assert bool(big.any()) and gn.abs().max() > 1e-4
        want = -lr * gn / (gn.abs() + eps)
        assert bool((torch.sign(m[big]) == -torch.sign(gn[big])).all()), n
        assert (m[big] - want[big]).abs().max().item() <= 1e-4 * lr, n
        assert (m[big].abs() - lr).abs().max().item() <= 1e-3 * lr, n
        assert torch.equal(live.cpu().reshape(-1), masters[n].cpu().reshape(-1).to(torch.bfloat16)), n


def test_three_steps_eager_equal_graph_replay(dev, tiny):
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, _, _, _ = tiny
    out = {}
    for graph in (False, True):
        w = fresh_weights(dev)
        ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", value=ValueLossConfig(level="action"), value_head=drawn_head(dims, dev))
        log = []
        for step in range(3):
            ids, mask, labels, pv = make_batch(dims, B, L, seed=20 + step)
            on, A, q = policy_inputs(labels, seed=step)
            Rt, vo = value_inputs("action", seed=30 + step)
            ts.set_batch(ids, mask, pv, labels)
            ts.set_policy_batch(A, q)
            ts.set_value_batch(Rt, vo)
            ts.step(1e-3, graph=graph)
            log.append((ts.values().clone(), ts.vstats.clone()))
        out[graph] = (log, ts.store.full_master().clone())
    for (v0, s0), (v1, s1) in zip(out[False][0], out[True][0]):
        assert torch.equal(v0, v1) and torch.equal(s0, s1) and bool(torch.isfinite(s0).all())
    assert torch.equal(out[False][1], out[True][1])
    assert not torch.equal(out[False][0][0][0], out[False][0][2][0])       # the values moved


@pytest.mark.parametrize("option", ["recompute", "fp8", "shard_params"])
def test_options_run_with_the_head(dev, tiny, option):
    """One step on vla-full-train under each option: finite statistics, and the head's outputs and gradients are the
    definition's on the hn the option's forward produced."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, _, _, (ids, mask, labels, pv) = tiny
    w = fresh_weights(dev)
    ts = TrainStep(w, "vla-full-train", B, L + 2, loss="policy", value=ValueLossConfig(level="token"), value_head=drawn_head(dims, dev),
                   **{option: True})
    on, A, q = policy_inputs(labels)
    Rt, vo = value_inputs("token")
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, q)
    ts.set_value_batch(Rt, vo)
    loss = ts.forward()
    ts.backward()
    check_head_against_definition(ts)
    norm = ts.clip_grad_norm()
    ts.optimizer_step(1e-3)
    assert np.isfinite(loss.item()) and np.isfinite(norm.item()) and norm.item() > 0
    ts.forward()
    assert bool(torch.isfinite(ts.vstats).all()) and bool(torch.isfinite(ts.stats).all())


_WORKER = r'''
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, os.environ["BL_ROOT"]); sys.path.insert(0, os.path.join(os.environ["BL_ROOT"], "tests"))
from test_train_step_gpu import make_batch
from bridgelang_amd.training.step import TrainStep
from bridgelang_amd.training.value_head import ValueHead
from bridgelang_amd.training.value_loss import ValueLossConfig
from bridgelang_amd.weights import allocate, tiny_dims
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)               # RCCL, one rank
dims = tiny_dims()
B, L = 2, 20
out = {}
for mode in ("plain", "comm", "comm-fullshard"):
    w = allocate(dims, dev).fill_synthetic(seed=3)
    vh = ValueHead(dims.llm_dim, dev, init_std=0.02, seed=4)
    kw = {} if mode == "plain" else dict(force_comm=True, shard_params="fullshard" in mode)
    ts = TrainStep(w, "vla-full-train", B, L, loss="policy", value=ValueLossConfig(level="token"), value_head=vh, max_grad_norm=1.0,
                   weight_decay=0.1, **kw)
    log = []
    for step in range(2):
        ids, mask, labels, pv = make_batch(dims, B, L, seed=50 + step)
        on = labels != -100
        g = torch.Generator().manual_seed(step)
        A = torch.where(on, torch.randn(B, L, generator=g), torch.zeros(B, L))
        ts.set_batch(ids, mask, pv, labels)
        ts.set_policy_batch(A, torch.where(on, torch.full((B, L), -5.0), torch.zeros(B, L)))
        ts.set_value_batch(torch.randn(B, L, generator=g), 0.3 * torch.randn(B, L, generator=g))
        loss, norm = ts.step(1e-3)
        log.append((loss.item(), norm.item(), ts.vstats.cpu().tolist(), ts.values().cpu().tolist()))
    masters = ts.store.master_state_dict(ts.comm)
    out[mode] = (log, masters["value_head.weight"].cpu(), masters["value_head.bias"].cpu(), ts.store.full_master(ts.comm).cpu())
    assert ts.comm.active == (mode != "plain")
for mode in ("comm", "comm-fullshard"):
    assert out[mode][0] == out["plain"][0], (mode, out[mode][0], out["plain"][0])
    assert all(torch.equal(a, b) for a, b in zip(out[mode][1:], out["plain"][1:])), mode
assert out["plain"][1].abs().max() > 0
print("VALUE_COMM_OK", out["plain"][0][-1][:2], flush=True)
dist.destroy_process_group()
'''


def test_force_comm_on_one_rank_is_bit_identical(dev, tmp_path):
    """The head's two replicated, unmarked buckets through the real collectives (a one-rank RCCL group, force_comm=True), with
    and without parameter sharding: losses, statistics, values and every master equal the collective-free run's bits."""
    from test_train_dist_gpu import _free_port
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, BL_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "VALUE_COMM_OK" in p.stdout, p.stdout[-3000:]


def test_gae_round_trip_and_saved_head(dev, tiny):
    """Rollout values → rl.gae → set_policy_batch / set_value_batch → step; the head saved from the optimizer's masters and
    loaded into a fresh one values the batch exactly as the trained one."""
    from bridgelang_amd.training.rl import gae
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_head import ValueHead
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, _, _, (ids, mask, labels, pv) = tiny
    w = fresh_weights(dev)
    vcfg = ValueLossConfig(level="action")
    ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", value=vcfg, value_head=drawn_head(dims, dev))
    on = labels != -100
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(torch.zeros(B, L), torch.zeros(B, L))
    ts.set_value_batch(torch.zeros(B), torch.zeros(B))
    ts.forward()                                                   # the learner values its own rollout states
    v_old, lp_old = ts.values().cpu().clone(), ts.token_logprobs().cpu().clone()
    rewards = torch.tensor([[0.3, -0.2, 1.0]])                     # the B sequences are the steps of one trajectory
    adv, ret = gae(rewards, v_old[None, :], last_values=torch.tensor([0.1]), gamma=0.99, lam=0.95)
    assert tuple(adv.shape) == (1, B) and bool(torch.isfinite(adv).all())
    ts.set_policy_batch(torch.where(on, adv[0][:, None].expand(B, L), torch.zeros(B, L)), lp_old)
    ts.set_value_batch(ret[0], v_old)
    loss, norm = ts.step(1e-3)
    st = {k: v.item() for k, v in ts.value_stats().items()}
    print("value stats of the step:", st)
    assert np.isfinite(loss.item()) and norm.item() > 0 and st["n"] == B and st["clip_frac"] == 0.0      # on-policy: vo = v
    assert ts.policy_stats()["ratio"].item() == 1.0
    ts.forward()
    after = ts.values().clone()
    assert not torch.equal(after.cpu(), v_old)
    fresh = ValueHead(dims.llm_dim, dev).load_state_dict(ts.value_head.state_dict(masters=ts.store.master_state_dict()))
    assert torch.equal(fresh.weight, ts.value_head.weight) and torch.equal(fresh.bias, ts.value_head.bias)
    ts2 = TrainStep(w, "vla-train", B, L + 2, loss="policy", value=vcfg, value_head=fresh)
    ts2.set_batch(ids, mask, pv, labels)
    ts2.set_policy_batch(torch.zeros(B, L), torch.zeros(B, L))
    ts2.set_value_batch(torch.zeros(B), torch.zeros(B))
    ts2.forward()
    assert torch.equal(ts2.values(), after)
