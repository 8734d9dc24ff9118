"""The restricted policy above the kernels: TrainStep(loss="policy") with `token_range` against torch.autograd over the CPU
oracle's logits, its on-policy and graph-replay properties and its plan; then one rollout → score → step round trip with
`action_tokens_only=True` on every call, the staggered pipeline against the engine, and one server request."""
import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from test_policy_step_gpu import B, L, oracle_logits, restated_loss, rows_of
from test_train_step_gpu import cos, make_batch

pytestmark = pytest.mark.gpu

ACTIONS = (31744, 256)


@pytest.fixture(scope="module")
def tiny(dev):
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    ids, mask, labels, pv = make_batch(dims, B, L)
    labels = torch.where(labels == 2, torch.full_like(labels, -100), labels)        # EOS was never sampled: not an action
    on = labels != -100
    assert int(on.sum()) == 7 * B and bool(((labels[on] >= ACTIONS[0]) & (labels[on] < sum(ACTIONS))).all())
    return dims, w, sd, (ids, mask, labels, pv)


def test_ranged_policy_gradients_match_autograd(dev, tiny):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep, trainable_names
    dims, w, sd, (ids, mask, labels, pv) = tiny
    first, count = ACTIONS
    stage = "vla-train"
    cfg = PolicyLossConfig(temperature=0.9, clip_low=0.2, clip_high=0.2, entropy_coef=0.01, kl_coef=0.05, token_range=ACTIONS)
    sd = {k: v.clone() for k, v in sd.items()}
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    logits = oracle_logits(sd, dims, ids, mask, pv)[:, first:first + count]         # the loss restated over the slice
    tg = rows_of(labels, -100).reshape(-1)
    tg = torch.where(tg != -100, tg - first, tg)
    on = labels != -100
    with torch.no_grad():
        lsm = torch.log_softmax(logits.double() / cfg.temperature, dim=-1)
        lp_rows = torch.where(tg != -100, lsm.gather(1, tg.clamp(min=0)[:, None])[:, 0], torch.zeros(()).double()).view(B, -1)
        lp = torch.zeros(B, L, dtype=torch.float64)
        lp[:, 1:] = lp_rows[:, 256:]
    g = torch.Generator().manual_seed(9)
    A = torch.where(on, torch.randn(B, L, generator=g) + 0.5, torch.zeros(B, L))
    shift = torch.tensor([0.5, -0.05, 0.05, -0.5, 0.0])[torch.arange(B * L) % 5].view(B, L)
    q = torch.where(on, lp.float() - shift, torch.zeros(B, L))
    ref = torch.where(on, lp.float() + 0.2 * torch.randn(B, L, generator=g), torch.zeros(B, L))
    want, row, ratio, _, stats = restated_loss(logits, tg, rows_of(A, 0.0).reshape(-1), rows_of(q, 0.0).reshape(-1),
                                               rows_of(ref, 0.0).reshape(-1), cfg)
    assert ((ratio - 0.8).abs().min() > 0.03) and ((ratio - 1.2).abs().min() > 0.03) and 0 < stats["clip_frac"] < 1
    want.backward()

    ts = TrainStep(w, stage, B, L + 2, loss="policy", policy=cfg)
    ts.set_batch(ids, mask, pv, labels)
    ts.set_policy_batch(A, q, ref)
    loss = ts.forward()
    ts.backward()
    got_stats = {k: v.item() for k, v in ts.policy_stats().items()}
    scale = row.abs().mean().item()
    print(f"loss {loss.item():.6f} vs oracle {want.item():.6f} (mean |row_loss| {scale:.4f}); stats {got_stats}")
    print("oracle stats", {k: float(v.detach()) for k, v in stats.items()})
    assert abs(loss.item() - want.item()) <= 2e-3 * scale                           # the bounds of test_policy_step_gpu.py
    assert got_stats["n_valid"] == int(on.sum()) and got_stats["loss"] == loss.item()
    assert got_stats["clip_frac"] == pytest.approx(float(stats["clip_frac"]), abs=1e-6)
    for k in ("pg", "entropy", "kl", "approx_kl", "ratio"):
        assert abs(got_stats[k] - float(stats[k])) <= 2e-3 * max(abs(float(stats[k])), 1.0), k
    assert got_stats["entropy"] <= np.log(count) + 1e-3                             # the entropy of a 256-way policy
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
    dl = ts.dlogits.view(-1, ts.dlogits.shape[-1])[:, :dims.vocab].float()
    assert bool((dl[:, :first] == 0).all()) and bool((dl[:, first + count:] == 0).all()) and bool((dl[:, first:first + count] != 0).any())
    tl = ts.token_logprobs().cpu()
    assert tuple(tl.shape) == (B, L) and (tl[~on] == 0).all()
    print(f"max |token_logprobs − oracle| = {(tl[on].double() - lp[on]).abs().max().item():.3g}")
    with pytest.raises(ValueError, match="token_range"):                            # a labelled token the policy cannot produce
        bad = labels.clone()
        bad[on.nonzero()[0][0], on.nonzero()[0][1]] = 2
        ts.set_batch(ids, mask, pv, bad)


def test_ranged_on_policy_ratio_graph_replay_and_plan(dev, tiny):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    dims, w, _, (ids, mask, labels, pv) = tiny
    ts = TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=PolicyLossConfig(temperature=0.8, entropy_coef=0.01, token_range=ACTIONS))
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
    ts.set_policy_batch(A, lp - 0.3 * torch.sign(A).to(dev))
    eager_loss = ts.forward().item()
    eager = ts.stats.clone()
    ts.backward()
    eager_dl = ts.dlogits.clone()
    for _ in range(2):                                       # the capture, then a replay
        ts.stats.zero_()
        ts.dlogits.fill_(3.0)
        loss = ts.forward(graph=True).item()
        ts.backward(graph=True)
        assert loss == eager_loss and torch.equal(ts.stats, eager) and torch.equal(ts.dlogits, eager_dl)
    assert ts.stats[5].item() > 0
    plain = TrainStep(w, "vla-train", B, L + 2, loss="policy")
    fo, bo = [op.name for op in ts.forward_ops], [op.name for op in ts.backward_ops]
    pf, pb = [op.name for op in plain.forward_ops], [op.name for op in plain.backward_ops]
    assert fo[:-1] == pf[:-1] and (pf[-1], fo[-1]) == ("bl_policy_loss_f32", "bl_policy_loss_range_f32")
    assert bo[1:] == pb[1:] and (pb[0], bo[0]) == ("bl_policy_loss_backward_f32", "bl_policy_loss_backward_range_f32")
    for bad in ((31740, 256), (31744, 324), (31744, 250)):
        with pytest.raises(ValueError, match="token_range"):
            TrainStep(w, "vla-train", B, L + 2, loss="policy", policy=PolicyLossConfig(token_range=bad))


# ---- the model surface -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=W.tiny_dims()).init_synthetic(seed=11)


def in_range(tokens):
    tokens = np.asarray(tokens)
    return bool(((tokens >= ACTIONS[0]) & (tokens < sum(ACTIONS))).all())


def test_rollout_score_and_step_with_action_tokens_only(model, dev):
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import group_advantages, policy_batch
    from bridgelang_amd.training.step import TrainStep
    from test_engine_gpu import make_inputs
    assert model.action_token_range() == ACTIONS
    Bp, K, n, temp = 2, 4, 7, 1.3
    ids, pv = make_inputs(model.dims, Bp, 10, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    sp = S.SamplingParams(temperature=temp, seed=[5, 6])
    free = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=K)[1]
    actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=K, action_tokens_only=True)
    assert tokens.shape == (Bp, K, n) and in_range(tokens) and not in_range(free)    # the flag is what keeps the draws inside
    assert np.isfinite(lp).all() and (lp <= 0).all()
    for j in range(K):                                                               # copy j = the single call with the derived seed
        spj = S.SamplingParams(temperature=temp, seed=S.derive_seed(np.array(sp.seed), j))
        a, tok, wt = model.predict_action(ids, "bridge_orig", pixel_values=pv, sampling=spj, return_weights=True, action_tokens_only=True)
        assert np.array_equal(a, actions[:, j]) and np.array_equal(tok, tokens[:, j]) and np.array_equal(S.logprob(wt), lp[:, j])
    # the scorer under the same restricted policy returns the sampler's log-probabilities bit for bit
    scored, wt, bins = model.score_actions(ids, pv, token_ids=tokens, sampling=S.SamplingParams(temperature=temp), return_bins=True,
                                           action_tokens_only=True)
    assert np.array_equal(scored, lp) and np.array_equal(model.score_actions(ids, pv, token_ids=tokens, action_tokens_only=True,
                                                                             sampling=S.SamplingParams(temperature=temp)), lp)
    assert bins.shape == (Bp, K, n, 256) and np.array_equal(bins.astype(np.int64).sum(-1), wt[..., 1])
    assert np.isneginf(model.score_actions(ids, pv, token_ids=free, sampling=S.SamplingParams(temperature=temp),
                                           action_tokens_only=True)[~((free >= ACTIONS[0]) & (free < sum(ACTIONS)))]).all()
    # constrained greedy decoding: the argmax over the action tokens of the logits the engine saw
    greedy = model.predict_action(ids, "bridge_orig", pixel_values=pv, action_tokens_only=True)
    eng = model.engine(Bp, ids.shape[1], n, sample=True, vocab_range=ACTIONS)
    want = ACTIONS[0] + eng.logits[:, :, ACTIONS[0]:sum(ACTIONS)].argmax(-1).t().cpu().numpy()
    assert np.array_equal(eng.gen_ids.t().cpu().numpy(), want) and np.array_equal(greedy, model.actions_from_token_ids(want, "bridge_orig"))
    # rollout → batch → one step of the learner with the same range
    adv = group_advantages(-np.abs(actions - 0.1).sum(-1))
    flat = lambda x: x.reshape(Bp * K, n)
    with pytest.raises(ValueError, match="action_tokens_only=True"):
        policy_batch(ids.cpu().repeat_interleave(K, 0), None, flat(free), flat(lp), adv.reshape(-1), token_range=ACTIONS)
    batch = policy_batch(ids.cpu().repeat_interleave(K, 0), None, flat(tokens), flat(lp), adv.reshape(-1), token_range=ACTIONS)
    l = batch["input_ids"].shape[1]
    ts = TrainStep(model.weights, "vla-train", Bp * K, l, loss="policy", policy=PolicyLossConfig(temperature=temp, token_range=ACTIONS))
    ts.set_batch(batch["input_ids"], batch["attention_mask"], pv.cpu().repeat_interleave(K, 0), batch["labels"])
    ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
    loss, norm = ts.step(1e-3)
    first = {k: v.item() for k, v in ts.policy_stats().items()}
    print("rollout vs training forward, restricted policy:", first)
    assert np.isfinite(loss.item()) and np.isfinite(norm.item()) and norm.item() > 0
    assert first["n_valid"] == Bp * K * n


def test_pipeline_with_vocab_range_equals_engine(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    from test_sampling_gpu import _ctx, _params
    c = _ctx(dev)
    PB, PL, N = 2, 12, 9
    batches = []
    for s in range(N):
        ids, pv = c["make_inputs"](c["dims"], PB, PL, seed=60 + s)
        batches.append((ids.to(dev), pv.to(dev), None if s == 2 else _params(PB, 10 + s)))
    eng = OpenVLAEngine(c["w"], PB, PL, sample=True, vocab_range=ACTIONS)
    assert sum(o.name == "bl_sample_range_f32" for o in eng.all_ops()) == eng.n_new
    assert [o.name.replace("_range", "") for o in eng.all_ops()] == [o.name for o in OpenVLAEngine(c["w"], PB, PL, sample=True).all_ops()]
    want = []
    for ids, pv, sp in batches:
        eng.set_sampling(sp if sp is not None else S.SamplingParams(temperature=0.0))
        eng.set_inputs(ids, pv)
        eng.run_eager()
        want.append((eng.gen_ids.t().clone().cpu(), eng.gen_wt.permute(1, 0, 2).clone().cpu()))
        assert in_range(want[-1][0].numpy())
    pipe = StaggeredDecodePipeline(c["w"], PB, PL, sample=True, vocab_range=ACTIONS)
    for e in pipe.engines:
        e.set_inputs(batches[0][0], batches[0][1])
    pipe.capture()
    got = []
    for s, (ids, pv, sp) in enumerate(batches):
        out = pipe.step(ids, pv, sampling=sp)
        if s >= pipe.slots - 1:
            got.append(tuple(o.clone().cpu() for o in out))
    got += [tuple(o.cpu() for o in x) for x in pipe.flush()]
    assert len(got) == N
    for s in range(N):
        assert torch.equal(got[s][0], want[s][0]), f"batch {s}: ids differ from the engine's"
        assert torch.equal(got[s][1], want[s][1]), f"batch {s}: weight pairs differ from the engine's"
    for kw in (dict(vocab_range=ACTIONS), dict(sample=True, vocab_range=(31742, 256)), dict(score=True, score_range=(31000, 8), vocab_range=ACTIONS)):
        with pytest.raises(ValueError):
            OpenVLAEngine(c["w"], PB, PL, **kw)


def test_server_request_with_action_tokens_only(model, dev):
    from PIL import Image
    from bridgelang_amd import serve
    from bridgelang_amd.extern.hf.processing_prismatic import PrismaticProcessor
    from test_serve_gpu import CharTokenizer
    proc = PrismaticProcessor(tokenizer=CharTokenizer())
    instr = "grasp the snack bag"
    img = np.random.default_rng(0).integers(0, 256, (224, 224, 3), dtype=np.uint8)
    x = proc(serve.get_openvla_prompt(instr, "openvla/openvla-7b"), Image.fromarray(img).convert("RGB"))
    sp = S.SamplingParams(temperature=1.3, seed=77)
    kw = dict(input_ids=x["input_ids"].to(dev), pixel_values=x["pixel_values"].to(dev, torch.bfloat16), unnorm_key="bridge_orig",
              sampling=sp, return_weights=True)
    want_a, want_tok, want_wt = model.predict_action(action_tokens_only=True, **kw)
    assert in_range(want_tok) and not in_range(model.predict_action(**kw)[1])
    with pytest.raises(ValueError):
        serve.OpenVLAServer(model, proc, action_tokens_only=True)
    server = serve.OpenVLAServer(model, proc, max_batch=1, max_wait_ms=1, sample=True, action_tokens_only=True)
    try:
        got = serve.decode_tree(server.predict_action({"image": serve.encode_ndarray(img), "instruction": instr, "unnorm_key": "bridge_orig",
                                                       "temperature": 1.3, "seed": 77, "return_logprob": True}))
        assert np.array_equal(got["action"], np.asarray(want_a).reshape(-1))
        assert np.array_equal(got["logprob"], S.logprob(want_wt).reshape(-1))
    finally:
        server.close()
