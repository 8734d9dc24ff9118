"""TrainStep(loss="distill"): the distillation step against torch.autograd over the CPU oracle's logits, graph replay under a
changing teacher, the untouched cross-entropy and policy plans, one sample → score → distil round trip on the tiny model,
and the error paths of `set_distill_batch` and of the constructor."""
import numpy as np
import pytest
import torch

from test_policy_step_gpu import oracle_logits, rows_of
from test_train_step_gpu import cos, make_batch

pytestmark = pytest.mark.gpu

B, L = 4, 20
ACTIONS = (31744, 256)


def action_batch(dims):
    """make_batch with the labels on the 7 action tokens alone: the EOS label lies outside the action range."""
    ids, mask, labels, pv = make_batch(dims, B, L)
    labels = torch.where((labels >= ACTIONS[0]) & (labels < sum(ACTIONS)), labels, torch.full_like(labels, -100))
    return ids, mask, labels, pv


def teacher_for(labels, seed, sharp=2.0, positive=False):
    """[B, L, 256] fp32: a random distribution on every labelled position (NaN elsewhere: never read)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.softmax(sharp * torch.randn(B, L, ACTIONS[1], generator=g, dtype=torch.float64), dim=-1)
    if not positive:
        q = torch.where(torch.rand(B, L, ACTIONS[1], generator=g) < 0.3, torch.zeros((), dtype=torch.float64), q)
        q = q / q.sum(-1, keepdim=True)
    return torch.where((labels != -100)[..., None], q.float(), torch.full((), float("nan")))


def rows3(x):
    """rows_of for a vector per token: [B, L, C] → [B·(S − 1), C]."""
    full = torch.cat([x[:, :1], torch.zeros(x.shape[0], 256, x.shape[2], dtype=x.dtype), x[:, 1:]], 1)
    return full[:, 1:].reshape(-1, x.shape[2])


def restated_loss(logits, tg, q, cfg):
    """The torch restatement (log_softmax over the range, plain sums, a mean) → (loss, dict of statistics)."""
    first, count = cfg.token_range
    valid = tg != -100
    lp = torch.log_softmax(logits.double()[:, first:first + count] / cfg.temperature, dim=-1)[valid]
    p, qq = lp.exp(), q.double()[valid]
    xlogy = torch.special.xlogy
    if cfg.kind == "forward_kl":
        D = (xlogy(qq, qq) - qq * lp).sum(-1)
    elif cfg.kind == "reverse_kl":
        D = (p * (lp - qq.log())).sum(-1)
    else:
        mix = cfg.beta * qq + (1 - cfg.beta) * p
        D = cfg.beta * (xlogy(qq, qq) - xlogy(qq, mix)).sum(-1) + (1 - cfg.beta) * (p * (lp - mix.log())).sum(-1)
    nll = -lp.gather(1, (tg[valid] - first)[:, None])[:, 0]
    row = D + cfg.sft_coef * nll
    idx = torch.arange(count, dtype=torch.float64)
    stats = dict(loss=row.mean(), n_valid=valid.sum(), divergence=D.mean(), entropy=-(p * lp).sum(-1).mean(),
                 teacher_entropy=-xlogy(qq, qq).sum(-1).mean(), agreement=(p.argmax(-1) == qq.argmax(-1)).double().mean(), nll=nll.mean(),
                 bin_gap=((p - qq) * idx).sum(-1).abs().mean())
    return row.mean(), row.detach(), {k: v.detach() for k, v in stats.items()}


@pytest.fixture(scope="module")
def tiny(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    return dims, w, sd, action_batch(dims)


@pytest.mark.parametrize("kind,beta,sft", [("forward_kl", 0.5, 0.3), ("jsd", 0.4, 0.2)])
def test_distill_gradients_match_autograd(dev, tiny, kind, beta, sft):
    from bridgelang_amd.training.distill_loss import DISTILL_STAT_NAMES, DistillLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    dims, w, sd, (ids, mask, labels, pv) = tiny
    stage = "vla-train"
    cfg = DistillLossConfig(kind=kind, beta=beta, temperature=0.9, sft_coef=sft, token_range=ACTIONS)
    sd = {k: v.clone() for k, v in sd.items()}
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    logits = oracle_logits(sd, dims, ids, mask, pv)
    tg = rows_of(labels, -100).reshape(-1)
    on = labels != -100
    teacher = teacher_for(labels, seed=21)
    want, row, stats = restated_loss(logits, tg, rows3(torch.nan_to_num(teacher)), cfg)
    want.backward()

    ts = TrainStep(w, stage, B, L + 2, loss="distill", distill=cfg)          # planned longer than the batch
    assert [op.name for op in ts.forward_ops][-1] == "bl_distill_loss_f32" and ts.backward_ops[0].name == "bl_distill_loss_backward_f32"
    ts.set_batch(ids, mask, pv, labels)
    ts.set_distill_batch(teacher)
    loss = ts.forward()
    ts.backward()
    got = {k: v.item() for k, v in ts.distill_stats().items()}
    scale = row.abs().mean().item()
    print(f"{kind}: loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |row_loss| {scale:.4f}); stats {got}")
    print("oracle stats", {k: float(v.detach()) for k, v in stats.items()})
    assert tuple(got) == DISTILL_STAT_NAMES
    assert abs(loss.item() - want.item()) <= 2e-3 * scale
    assert got["n_valid"] == int(on.sum()) == 7 * B and got["loss"] == loss.item()
    assert got["teacher_entropy"] == pytest.approx(float(stats["teacher_entropy"]), rel=1e-5)      # the teacher is the same on both sides
    for k in ("divergence", "entropy", "nll", "bin_gap"):                                          # the file's loss bound, floor 1
        assert abs(got[k] - float(stats[k])) <= 2e-3 * max(abs(float(stats[k])), 1.0), k
    assert abs(got["agreement"] - float(stats["agreement"])) <= 1.0 / (7 * B) + 1e-6               # at most one near-tie of the student's
    worst = 1.0
    for n in names:
        g, ref_g = ts.store.named_grad(n).float().cpu(), sd[n].grad
        s = ref_g.abs().max().item()
        assert s > 0, n
        c = cos(g, ref_g)
        worst = min(worst, c)
        err = (g - ref_g).abs().max().item()
        assert c > 0.99 and err <= 0.06 * s, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {s:.3g}"
    print(f"worst gradient cosine {worst:.5f}")
    tl = ts.token_logprobs().cpu()                          # row slot 0 is where the policy loss has it
    assert tuple(tl.shape) == (B, L) and (tl[~on] == 0).all() and (tl[on] < 0).all()
    outside = torch.ones(dims.vocab, dtype=torch.bool)
    outside[ACTIONS[0]:sum(ACTIONS)] = False
    assert bool((ts.dlogits[:, outside.to(dev)] == 0).all()) and bool((ts.dlogits[ts.targets == -100] == 0).all())


def test_one_captured_graph_serves_two_teachers(dev, tiny):
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, _, (ids, mask, labels, pv) = tiny
    ts = TrainStep(w, "vla-train", B, L + 2, loss="distill",
                   distill=DistillLossConfig(kind="reverse_kl", temperature=0.8, sft_coef=0.1, token_range=ACTIONS))
    ts.set_batch(ids, mask, pv, labels)
    teachers = [teacher_for(labels, seed=s, positive=True) for s in (5, 6)]
    eager = []
    for t in teachers:
        ts.set_distill_batch(t)
        loss = ts.forward().item()
        ts.backward()
        eager.append((loss, ts.stats.clone(), ts.row_stats.clone(), ts.dlogits.clone()))
    assert eager[0][0] != eager[1][0] and np.isfinite(eager[0][0]) and np.isfinite(eager[1][0])
    for _ in range(2):                                       # the capture with teacher 0, then replays
        for t, (loss, stats, rs, dl) in zip(teachers, eager):
            ts.set_distill_batch(t)
            ts.stats.zero_()
            ts.dlogits.zero_()
            got = ts.forward(graph=True).item()
            ts.backward(graph=True)
            assert got == loss and torch.equal(ts.stats, stats) and torch.equal(ts.row_stats, rs) and torch.equal(ts.dlogits, dl)
    assert len(ts._graphs) >= 2


def test_ce_and_policy_steps_are_untouched(dev):
    """The cross-entropy and policy steps built BEFORE a distill step and the ones built AFTER it give the same bits for a fixed
    batch, and the distill plan differs from the cross-entropy plan at the loss boundary alone."""
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    ids, mask, labels, pv = action_batch(dims)
    on = labels != -100
    A = torch.where(on, torch.randn(B, L, generator=torch.Generator().manual_seed(2)) + 0.3, torch.zeros(B, L))
    q = torch.where(on, torch.full((B, L), -5.0), torch.zeros(B, L))
    w = allocate(dims, dev).fill_synthetic(seed=3)

    def run(loss, **kw):
        ts = TrainStep(w, "vla-train", B, L + 2, loss=loss, **kw)
        ts.set_batch(ids, mask, pv, labels)
        if loss == "policy":
            ts.set_policy_batch(A, q)
        if loss == "distill":
            ts.set_distill_batch(teacher_for(labels, seed=3))
        out = ts.forward().clone()
        ts.backward()
        return out, ts.dlogits.clone(), ts.store.grad.clone(), [op.name for op in ts.forward_ops], [op.name for op in ts.backward_ops]
    pol = dict(policy=PolicyLossConfig(temperature=0.9, entropy_coef=0.01, token_range=ACTIONS))
    before = [run("ce"), run("policy", **pol)]
    dist = run("distill", distill=DistillLossConfig(kind="jsd", token_range=ACTIONS))
    after = [run("ce"), run("policy", **pol)]
    for a, b in zip(before, after):
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]
    ce = before[0]
    assert dist[3][:-1] == ce[3][:-1] and dist[4][1:] == ce[4][1:]
    assert not any(name.startswith("bl_distill") for r in before + after for name in r[3] + r[4])
    assert bool(torch.isfinite(dist[0])) and float(dist[2].abs().max()) > 0


def test_sample_score_distill_round_trip(dev):
    """The teacher is the learner's own base weights seen through the inference engine: the step's divergence against it is
    the engine-versus-learner gap (printed, not gated) and must be strictly below the divergence against the same teacher
    rows permuted across positions; the two arg-maxes agree everywhere."""
    from bridgelang_amd import sampling as S
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    from bridgelang_amd.training import rl
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.step import TrainStep
    from test_engine_gpu import make_inputs
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    model = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=W.tiny_dims()).init_synthetic(seed=11)
    assert model.action_token_range() == ACTIONS
    Bp, n, temp = 4, 7, 1.0
    ids, pv = make_inputs(model.dims, Bp, 10, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    _, tokens, _ = model.sample_actions(ids, pv, "bridge_orig", S.SamplingParams(temperature=temp, seed=[5, 6, 7, 8]), action_tokens_only=True)
    tokens = np.asarray(tokens).reshape(Bp, n)
    _, wt, bins = model.score_actions(ids, pv, token_ids=tokens, sampling=S.SamplingParams(temperature=temp), return_bins=True,
                                      action_tokens_only=True, use_adapters=False)
    wt, bins = np.asarray(wt).reshape(Bp, n, 2), np.asarray(bins).reshape(Bp, n, ACTIONS[1])
    batch = rl.distill_batch(ids.cpu(), None, tokens, bins, wt, token_range=ACTIONS)
    l = batch["input_ids"].shape[1]
    ts = TrainStep(model.weights, "vla-train", Bp, l, loss="distill",
                   distill=DistillLossConfig(kind="forward_kl", temperature=temp, token_range=ACTIONS))
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv.cpu(), batch["labels"])
    on = batch["labels"] != -100
    mixed = batch["teacher_probs"].clone()
    mixed[on] = batch["teacher_probs"][on].roll(3, dims=0)                  # every position gets another position's teacher
    ts.set_distill_batch(mixed)
    ts.forward()
    permuted = {k: v.item() for k, v in ts.distill_stats().items()}
    ts.set_distill_batch(batch["teacher_probs"])
    loss, norm = ts.step(1e-3)
    own = {k: v.item() for k, v in ts.distill_stats().items()}
    print(f"self-distillation through the engine: divergence {own['divergence']:.3e} (permuted teacher {permuted['divergence']:.3e}), "
          f"bin_gap {own['bin_gap']:.3e}, agreement {own['agreement']}, loss {loss.item():.3e}, grad norm {norm.item():.3e}")
    assert own["n_valid"] == Bp * n and np.isfinite(loss.item()) and np.isfinite(norm.item())
    assert 0 <= own["divergence"] < permuted["divergence"]
    assert own["agreement"] == 1.0
    assert own["teacher_entropy"] == permuted["teacher_entropy"] or abs(own["teacher_entropy"] - permuted["teacher_entropy"]) < 1e-5


def test_error_paths(dev, tiny):
    from bridgelang_amd.training.distill_loss import DistillLossConfig
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.preference_loss import PreferenceLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    dims, w, _, (ids, mask, labels, pv) = tiny
    for kw in (dict(loss="ce", distill=DistillLossConfig()), dict(loss="policy", distill=DistillLossConfig()),
               dict(loss="distill", policy=PolicyLossConfig()), dict(loss="distill", preference=PreferenceLossConfig()),
               dict(loss="distill", value=ValueLossConfig()), dict(loss="distill", distill=DistillLossConfig(token_range=(31740, 256))),
               dict(loss="distil")):
        with pytest.raises(ValueError):
            TrainStep(w, "vla-train", B, L + 2, **kw)
    with pytest.raises(RuntimeError):
        TrainStep(w, "vla-train", B, L + 2).set_distill_batch(torch.zeros(B, L, 256))
    with pytest.raises(RuntimeError):
        TrainStep(w, "vla-train", B, L + 2).distill_stats()
    ts = TrainStep(w, "vla-train", B, L + 2, loss="distill", distill=DistillLossConfig(kind="reverse_kl", token_range=ACTIONS))
    assert tuple(ts.teacher.shape) == (B * ts.S, 256) and ts.teacher.dtype == torch.float32
    ts.set_batch(ids, mask, pv, labels)
    for call in (ts.forward, ts.backward):                  # the teacher comes first
        with pytest.raises(RuntimeError, match="set_distill_batch"):
            call()
    good = teacher_for(labels, seed=1, positive=True)
    on = labels != -100
    b, t = (int(x) for x in on.nonzero()[0])
    for what, edit in (("shape", lambda q: q[:, :, :128]), ("shape", lambda q: q[:, :-1]), ("non-finite", lambda q: q.index_put((torch.tensor(b), torch.tensor(t), torch.tensor(3)), torch.tensor(float("inf")))),
                       (">= 0", lambda q: q.index_put((torch.tensor(b), torch.tensor(t), torch.tensor(3)), torch.tensor(-0.01))),
                       ("sums to", lambda q: q * 1.01), ("reverse_kl", lambda q: q.index_put((torch.tensor(b), torch.tensor(t), q[b, t].argmin()), torch.tensor(0.0)))):   # its smallest bin: the mass stays
        with pytest.raises(ValueError, match=what):
            ts.set_distill_batch(edit(good.clone()))
        with pytest.raises(RuntimeError):                   # a refused teacher is no teacher
            ts.forward()
    ts.set_distill_batch(good)
    assert np.isfinite(ts.forward().item())
    ts.set_batch(ids, mask, pv, labels)                     # a new batch invalidates the teacher
    with pytest.raises(RuntimeError, match="set_distill_batch"):
        ts.forward()
    with pytest.raises(ValueError, match="outside"):        # the EOS label lies outside the action range
        ts.set_batch(*make_batch(dims, B, L)[:2], pv, make_batch(dims, B, L)[2])
