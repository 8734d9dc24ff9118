"""The critic at inference on the HIP path (reduced-width model): `attach_value_head` / `return_values=` on `predict_action`,
`sample_actions`, `score_actions`; `OpenVLAEngine(value=, value_head=)`, `StaggeredDecodePipeline(value=)` and
`OpenVLAServer(value_head=)` with `"return_value"`.

Everything but the last test is exact: the value op only reads residual rows, so ids / logits / actions are those of the run
without it, and a value is the bits of `ops.rmsnorm` → `train_ops.value_head` (tests/test_value_predict_gpu.py) over the row
it belongs to — a sequence's own row, whatever batch, padding, pipeline slot or server batch it rides in.

Rollout against learner (the one tolerance, measured): V_e = predict_action(return_values="action"), V_l = `ts.values()` of a
plain TrainStep("vla-train", value=...) over the same weights, V_o = the oracle's fp64 `hn_o @ w + b`. Two independent bf16
evaluations of one quantity: max|V_e − V_o| <= 2·max|V_l − V_o|, the margin tests/test_lora_inference_gpu.py gives such a pair.
The head is a draw plus the smallest correction that puts the oracle's value one row earlier at least 0.5 from V_o on every
state; the test asserts that this is at least 8·max|V_l − V_o|, so a value read from the wrong row fails. Measured on an MI355X (16 states): see DESIGN.md §6g."""
import numpy as np
import pytest
import torch

from test_engine_gpu import make_inputs
from test_lora_inference_gpu import STATS, dyadic_adapters, new_model
from test_value_predict_gpu import composition

pytestmark = pytest.mark.gpu

B, L, N = 2, 10, 7
KEY = "bridge_orig"
VALUE_OP = "bl_value_predict_f32"


def drawn_head(dev, seed=4, init_std=0.05, dim=512):
    from bridgelang_amd.training.value_head import ValueHead
    vh = ValueHead(dim, dev, init_std=init_std, seed=seed)
    vh.bias.fill_(0.125)
    return vh


@pytest.fixture(scope="module")
def st(dev):
    """Model, head, inputs and the head-free results — computed once, compared against, never modified."""
    model = new_model(dev)
    ids, pv = make_inputs(model.dims, B, L, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    return dict(model=model, vh=drawn_head(dev), ids=ids, pv=pv)


@pytest.fixture()
def attached(st):
    st["model"].attach_value_head(st["vh"])
    yield st
    st["model"].detach_value_head()


def bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def names(eng):
    return [op.name for op in eng.all_ops()]


def padded_batch(dims, lens, width, seed):
    ids, pv = make_inputs(dims, len(lens), width, seed=seed)
    mask = torch.zeros(len(lens), width, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, n - 1] = 29871
        ids[b, n:] = 32000
        mask[b, :n] = 1
    return ids, pv, mask


def test_errors_and_off_means_off(st, dev):
    from bridgelang_amd import sampling as S
    model, vh, ids, pv = st["model"], st["vh"], st["ids"], st["pv"]
    call = lambda **kw: model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key=KEY, **kw)
    with pytest.raises(ValueError):
        call(return_values="action")                                  # no head attached
    with pytest.raises(ValueError):
        model.attach_value_head(drawn_head(dev, dim=256))             # dim != llm_dim
    assert VALUE_OP not in names(model.engine(B, L))
    lora = dyadic_adapters(model)
    pids, ppv, pmask = padded_batch(model.dims, [12, 7], 12, seed=52)
    sp = S.SamplingParams(temperature=1.3, seed=[5, 6])
    #        call kwargs                                                       engine kwargs (prompt length, flags)
    plans = [(dict(), dict(prompt_len=L)),
             (dict(sampling=sp, return_weights=True), dict(prompt_len=L, sample=True)),
             (dict(input_ids=pids.to(dev), pixel_values=ppv.to(dev), attention_mask=pmask.to(dev)), dict(prompt_len=13, padded=True)),
             (dict(use_adapters=True), dict(prompt_len=L, use_adapters=True))]
    model.attach_value_head(vh)
    try:
        assert model._value_head is vh
        with pytest.raises(ValueError):
            call(return_values="state")
        for ckw, ekw in plans:
            if "use_adapters" in ckw:
                model.attach_adapters(lora)
            kw = {**dict(input_ids=ids, pixel_values=pv, unnorm_key=KEY), **ckw}
            want = model.predict_action(**kw)
            e0 = model.engine(B, **ekw)
            tok0, lg0, n0 = e0.gen_ids.clone(), e0.logits.clone(), names(e0)
            assert VALUE_OP not in n0
            for level, extra in (("action", 1), ("token", N)):
                got = model.predict_action(return_values=level, **kw)
                e1 = model.engine(B, value=level, **ekw)
                assert e1 is not e0 and e1.value == level
                assert torch.equal(e1.gen_ids, tok0) and torch.equal(e1.logits, lg0), (ekw, level)
                n1 = names(e1)
                assert [n for n in n1 if n != VALUE_OP] == n0 and n1.count(VALUE_OP) == extra, (ekw, level)
                head = got[:-1] if len(got) > 2 else got[0]
                for a, b in zip(head if isinstance(head, tuple) else (head,), want if isinstance(want, tuple) else (want,)):
                    assert np.array_equal(np.asarray(a), np.asarray(b)), (ekw, level)
                v = got[-1]
                assert v.dtype == np.float32 and v.shape == ((B,) if level == "action" else (B, N)) and np.isfinite(v).all()
                if level == "token":
                    assert bits(v[:, 0], v_action), "values[0] of the token level is the action level's value"
                v_action = v
    finally:
        model.detach_adapters()
        model.detach_value_head()
    assert model._value_head is None and not any("value" in str(k) for k in model._engines)


def test_the_right_rows_exactly(st, dev):
    from bridgelang_amd.engine import OpenVLAEngine
    model, vh, ids, pv = st["model"], st["vh"], st["ids"], st["pv"]
    w = model.weights
    with pytest.raises(ValueError):
        OpenVLAEngine(w, B, L, value="action")                        # no head
    with pytest.raises(ValueError):
        OpenVLAEngine(w, B, L, value="state", value_head=vh)
    for n_new, level in ((N, "token"), (1, "action"), (1, "token")):
        eng = OpenVLAEngine(w, B, L, n_new=n_new, value=level, value_head=vh)
        eng.generate(ids, pv)
        _, want = composition(eng.xd, w.norm, vh.weight, vh.bias, eng.dims.rms_eps)     # xd as the last step left it
        assert bits(eng.values[n_new - 1], want), (n_new, level)
        assert tuple(eng.value_result().shape) == ((B,) if level == "action" else (B, n_new))


def test_every_sequence_on_its_own(attached, dev):
    from bridgelang_amd import sampling as S
    model = attached["model"]
    lens = [12, 2, 7]                                                 # one full-length, the shortest possible, one between
    ids, pv, mask = (t.to(dev) for t in padded_batch(model.dims, lens, 12, seed=61))
    call = lambda i, p, **kw: model.predict_action(input_ids=i, pixel_values=p, unnorm_key=KEY, return_values="token", **kw)
    act, val = call(ids, pv, attention_mask=mask)
    alone = [call(ids[b:b + 1, :n], pv[b:b + 1]) for b, n in enumerate(lens)]
    for b in range(len(lens)):
        assert np.array_equal(act[b], np.asarray(alone[b][0]).reshape(-1)) and bits(val[b:b + 1], alone[b][1]), f"sequence {b}"
    perm = [2, 0, 1]
    act_p, val_p = call(ids[perm], pv[perm], attention_mask=mask[perm])
    assert np.array_equal(act_p, act[perm]) and bits(val_p, val[perm])
    assert len({float(x) for x in val[:, 0]}) == len(lens), "different states, equal values: nothing was checked"
    # sampled copies share their state
    i2, p2 = attached["ids"], attached["pv"]
    _, v_greedy = model.predict_action(input_ids=i2, pixel_values=p2, unnorm_key=KEY, return_values="action")
    sp = S.SamplingParams(temperature=1.3, seed=[5, 6])
    a, tok, lp, v_tok = model.sample_actions(i2, p2, KEY, sp, num_samples=3, return_values="token")
    assert v_tok.shape == (B, 3, N) and v_tok.dtype == np.float32
    for j in range(3):
        assert bits(v_tok[:, j, 0], v_greedy), f"copy {j}"
    a2, tok2, lp2, v_act = model.sample_actions(i2, p2, KEY, sp, num_samples=3, return_values="action")
    assert np.array_equal(tok2, tok) and np.array_equal(lp2, lp) and bits(v_act, v_greedy)
    assert not np.array_equal(tok[:, 0], tok[:, 1]) and not bits(v_tok[:, 0, 1:], v_tok[:, 1, 1:])
    # scoring the drawn tokens walks the same rows
    lp3, v_sc = model.score_actions(i2, p2, token_ids=tok, sampling=S.SamplingParams(temperature=1.3), return_values="token")
    assert np.array_equal(lp3, lp) and bits(v_sc, v_tok)
    assert bits(model.score_actions(i2, p2, token_ids=tok, return_values="action")[1], v_greedy)


@pytest.mark.parametrize("level,graphs", [("action", False), ("token", True)])
def test_pipeline_returns_the_engines_values(st, dev, level, graphs):
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    model, vh = st["model"], st["vh"]
    w, n_new, n_batches = model.weights, 3, 5
    batches = [tuple(t.to(dev) for t in make_inputs(model.dims, B, L, seed=70 + s)) for s in range(n_batches)]
    eng = OpenVLAEngine(w, B, L, n_new=n_new, value=level, value_head=vh)
    want = []
    for ids, pv in batches:
        tok = eng.generate(ids, pv).clone()
        want.append((tok, eng.value_result().clone()))
    pipe = StaggeredDecodePipeline(w, B, L, n_new=n_new, value=level, value_head=vh)
    assert sum(op.name == VALUE_OP for op in pipe.merged_ops[0]) == (n_new - 1 if level == "token" else 0)
    if graphs:
        for e in pipe.engines:
            e.set_inputs(*batches[0])
        pipe.capture()
    got = []
    for k, (ids, pv) in enumerate(batches):
        out = pipe.step(ids, pv)
        if k >= pipe.slots - 1:
            got.append(tuple(o.clone() for o in out))
    got += pipe.flush()
    assert len(got) == n_batches
    for k, ((tok, val), (wtok, wval)) in enumerate(zip(got, want)):
        assert torch.equal(tok, wtok) and bits(val, wval), f"batch {k}"
    assert not bits(want[0][1], want[1][1])


def test_server_answers_return_value(st, dev):
    from PIL import Image
    from bridgelang_amd import serve
    from bridgelang_amd.extern.hf.processing_prismatic import PrismaticProcessor
    from test_serve_gpu import CharTokenizer
    vla, vh = st["model"], st["vh"]
    proc = PrismaticProcessor(tokenizer=CharTokenizer())
    rng = np.random.default_rng(7)
    reqs = [(instr, rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)) for instr in ("lift", "open the jar", "stack it", "lift")]
    xs = [proc(serve.get_openvla_prompt(i, "openvla/openvla-7b"), Image.fromarray(img).convert("RGB")) for i, img in reqs]
    payload = lambda r, **kw: {"image": serve.encode_ndarray(r[1]), "instruction": r[0], "unnorm_key": KEY, **kw}
    server = serve.OpenVLAServer(vla, proc, max_wait_ms=20, pipeline_batch=2, pad_to=max(x["input_ids"].shape[1] for x in xs) + 1,
                                 value_head=vh)
    try:
        assert vla._value_head is vh
        want = [vla.predict_action(input_ids=x["input_ids"].to(dev), pixel_values=x["pixel_values"].to(dev, torch.bfloat16),
                                   unnorm_key=KEY, do_sample=False, return_values="action") for x in xs]
        made = [server._make_request({"image": r[1], "instruction": r[0], "unnorm_key": KEY, "return_value": i != 3})
                for i, r in enumerate(reqs)]
        for r in made:
            server._q.put(r)
        out = [r.future.result(timeout=120) for r in made]
        for i in range(3):
            assert set(out[i]) == {"action", "value"} and isinstance(out[i]["value"], float)
            assert np.array_equal(out[i]["action"], want[i][0]) and np.float32(out[i]["value"]) == want[i][1][0], f"request {i}"
        assert isinstance(out[3], np.ndarray) and np.array_equal(out[3], want[3][0])       # not asked for: the plain answer
        assert server.pipelines_built == 1 and any(len(set(b)) >= 2 for b in server.batch_lengths)
        wire = serve.decode_tree(server.predict_action(payload(reqs[1], return_value=True)))  # the HTTP body, json-ready
        assert np.array_equal(wire["action"], want[1][0]) and np.float32(wire["value"]) == want[1][1][0]
    finally:
        server.close()
        vla.detach_value_head()
    plain = serve.OpenVLAServer(vla, proc, max_wait_ms=20)
    try:
        assert plain.predict_action(payload(reqs[0], return_value=True)) == "error"
        assert isinstance(serve.decode_tree(plain.predict_action(payload(reqs[0]))), np.ndarray)
    finally:
        plain.close()


def test_adapters_select_the_trunk(st, dev):
    model, vh, ids, pv = st["model"], st["vh"], st["ids"], st["pv"]
    call = lambda m, **kw: m.predict_action(input_ids=ids, pixel_values=pv, unnorm_key=KEY, return_values="token", **kw)
    lora = dyadic_adapters(model)
    merged = new_model(dev, seed=3).load_state_dict(lora.merged_state_dict()).attach_value_head(vh)
    model.attach_value_head(vh)
    try:
        a_base, v_base = call(model)
        a_m, v_m = call(merged)
        model.attach_adapters(lora)
        a_on, v_on = call(model, use_adapters=True)
        a_off, v_off = call(model, use_adapters=False)
        assert np.array_equal(a_on, a_m) and bits(v_on, v_m)
        assert np.array_equal(a_off, a_base) and bits(v_off, v_base)
        assert not bits(v_on, v_off)
        assert bits(call(model)[1], v_on)                              # None: the attached adapters
    finally:
        model.detach_adapters()
        model.detach_value_head()


def test_live_head_no_rebuild(st, dev, tmp_path):
    """The engine reads the head's tensors in place: one optimizer step over the attached head shows on the next replay of the
    graph captured before it; the head saved from the optimizer's masters loads to the same bits."""
    from bridgelang_amd import weights as W
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    from test_train_step_gpu import make_batch
    model, ids, pv = st["model"], st["ids"], st["pv"]
    vh = drawn_head(dev, seed=9)
    model.attach_value_head(vh)
    try:
        call = lambda: model.predict_action(input_ids=ids, pixel_values=pv, unnorm_key=KEY, return_values="action")
        eng = model.engine(B, L, value="action")
        eng.set_inputs(ids, pv)
        eng.capture()
        a0, v0 = call()
        # a learner over its own copy of the trunk, training THIS head
        w2 = W.allocate(W.tiny_dims(), dev).fill_synthetic(seed=3)
        bids, bmask, blabels, bpv = make_batch(w2.dims, 3, 20)
        ts = TrainStep(w2, "vla-train", 3, 22, loss="policy", policy=PolicyLossConfig(), value=ValueLossConfig(coef=0.5, clip=None),
                       value_head=vh)
        ts.set_batch(bids, bmask, bpv, blabels)
        ts.set_policy_batch(torch.zeros(3, 20), torch.zeros(3, 20))
        ts.set_value_batch(torch.full((3,), 4.0))
        ts.step(1e-2)
        a1, v1 = call()
        assert model.engine(B, L, value="action") is eng and eng._graph is not None
        assert np.array_equal(a1, a0) and not bits(v1, v0)
        fresh = OpenVLAEngine(model.weights, B, L, value="action", value_head=vh)       # built after the step
        fresh.generate(ids, pv)
        assert bits(v1, fresh.value_result())
        vh.bias.add_(0.5)                                              # and a plain in-place write
        assert not bits(call()[1], v1)
        vh.bias.sub_(0.5)
        vh.save(tmp_path, masters=ts.store.master_state_dict())
        model.load_value_head(tmp_path)
        assert model._value_head is not vh and bits(model._value_head.weight.float(), vh.weight.float())
        assert model.engine(B, L, value="action") is not eng
        assert bits(call()[1], v1)
    finally:
        model.detach_value_head()


def test_rollout_against_learner(st, dev):
    from oracle import restate as R
    from bridgelang_amd.training.policy_loss import PolicyLossConfig
    from bridgelang_amd.training.rl import policy_batch
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.training.value_loss import ValueLossConfig
    model = st["model"]
    dims, Bs, n_batches = model.dims, 4, 4
    sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
    om = R.OracleModel.from_dims(sd, dims)
    vh = drawn_head(dev)
    model.attach_value_head(vh)
    try:
        ts, hn_rows, batches = None, [], []
        for s in range(n_batches):
            ids, pv = make_inputs(dims, Bs, L, seed=80 + s)
            trace = {}
            om.prefill(ids, pv, trace=trace)
            hn_o = R.rmsnorm(R.Prec(True, "blas"), trace["llm"][-1], sd["language_model.model.norm.weight"].float(), dims.rms_eps)
            S = hn_o.shape[1]
            assert S == dims.n_patches + L
            hn_rows.append(hn_o[:, S - 2:].double())                  # the last prompt position but one, and the last
            tokens = model.generate(ids.to(dev), N, pixel_values=pv.to(dev))[:, -N:].cpu()
            batch = policy_batch(ids, None, tokens, torch.zeros(Bs, N), torch.zeros(Bs), values=torch.zeros(Bs), returns=torch.zeros(Bs))
            if ts is None:
                ts = TrainStep(model.weights, "vla-train", Bs, batch["input_ids"].shape[1], loss="policy", policy=PolicyLossConfig(),
                               value=ValueLossConfig(coef=0.5, clip=0.2, level="action"), value_head=vh)
            batches.append((ids, pv, batch))
        hn2 = torch.cat(hn_rows, dim=0)                                # [16, 2, D] fp64
        # The head: a draw (std 0.05) plus the smallest correction, inside the span of the oracle's 16 row differences, that puts
        # every state's value at least GAP away from the value one row earlier. (A larger init_std cannot do that: the gap and
        # both errors are linear in w, so their quotient does not move with its scale.) Oracle rows alone decide it.
        GAP = 0.5
        w0 = vh.weight.float().cpu().double()
        d = hn2[:, 1] - hn2[:, 0]
        g0 = d @ w0
        target = torch.where(g0 >= 0, torch.ones_like(g0), -torch.ones_like(g0)) * g0.abs().clamp(min=GAP)
        vh.weight.copy_((w0 + torch.linalg.pinv(d) @ (target - g0)).to(dev, torch.bfloat16))
        w64, b64 = vh.weight.float().cpu().double(), float(vh.bias.float().item())
        v_o, v_prev = hn2[:, 1] @ w64 + b64, hn2[:, 0] @ w64 + b64
        v_l = []
        for ids, pv, batch in batches:
            ts.set_batch(batch["input_ids"], batch["attention_mask"], pv, batch["labels"])
            ts.set_policy_batch(batch["advantages"], batch["old_logprobs"])
            ts.set_value_batch(batch["returns"], batch["old_values"])
            ts.forward()
            v_l.append(ts.values().cpu().double())
        err_l = float((torch.cat(v_l) - v_o).abs().max())
        gap = float((v_prev - v_o).abs().min())
        print(f"\nlearner max|V_l - V_o| {err_l:.5f}, min |V_o(prev row) - V_o| {gap:.5f}, |w| {float(w64.norm()):.3f} (drawn {float(w0.norm()):.3f})")
        assert err_l > 0 and gap >= 8 * err_l, "the head does not separate the neighbouring row: the condition on the inputs"
        v_e = torch.cat([torch.from_numpy(model.predict_action(input_ids=ids.to(dev), pixel_values=pv.to(dev), unnorm_key=KEY,
                                                               return_values="action")[1]) for ids, pv, _ in batches]).double()
        err_e = float((v_e - v_o).abs().max())
        print(f"rollout/learner over {len(v_o)} states: engine max|V_e - V_o| {err_e:.5f}, learner max|V_l - V_o| {err_l:.5f}, "
              f"ratio {err_e / err_l:.3f}; |V_o| up to {float(v_o.abs().max()):.3f}")
        assert err_e <= 2.0 * err_l
    finally:
        model.detach_value_head()
