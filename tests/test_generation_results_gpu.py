"""Every extra of `generate`, `predict_action`, `sample_actions` and `score_actions` asked for AT ONCE (reduced-width model):
weights / bins with `score_range`, the critic's values at both levels, `return_attention="both"` with `text_splits` — on an
un-padded batch and on a right-padded one. Each element of the combined return must be, bit for bit and in shape and
dtype, the element of the call that asks for that extra alone: the ops behind the extras only read, so an element that
differs has landed in the wrong slot (or was stacked wrongly across engine runs). With 9 copies / candidates at B = 2 an
engine run holds 16 // 2 = 8 of them, so the ninth forces a second run; copy j of `sample_actions` is checked against the
one call seeded `derive_seed(seed, j)`, candidate j of `score_actions` against the one-candidate call."""
import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd.attention_taps import ActionAttention
from test_engine_gpu import make_inputs
from test_lora_inference_gpu import new_model
from test_value_inference_gpu import drawn_head, padded_batch

pytestmark = pytest.mark.gpu

B, L, N, K = 2, 10, 7, 9
KEY = "bridge_orig"
CASES = [(c, level) for c in ("plain", "padded") for level in ("action", "token")]


@pytest.fixture(scope="module")
def st(dev):
    """The model with a value head, both batches and their settings — made once, never modified."""
    model = new_model(dev).attach_value_head(drawn_head(dev))
    ids, pv = make_inputs(model.dims, B, L, seed=31)
    pids, ppv, pmask = padded_batch(model.dims, [12, 7], 12, seed=52)
    first, count = model.action_token_range()
    g = torch.Generator().manual_seed(9)
    return dict(model=model, first=first, count=count,
                sp=S.SamplingParams(temperature=[1.3, 0.7], top_k=[0, 50], seed=[5, 6]),        # per-sequence: the tiling matters
                forced=first + torch.randint(0, count, (B, N), generator=g),
                cand=(first + torch.randint(0, count, (B, K, N), generator=g)).numpy(),
                plain=dict(ids=ids.to(dev), pv=pv.to(dev), mask=None, splits=torch.tensor([[4, 8], [3, 7]])),
                padded=dict(ids=pids.to(dev), pv=ppv.to(dev), mask=pmask.to(dev), splits=torch.tensor([[4, 8], [3, 5]])))


def same(a, b):
    """Equal in kind, shape, dtype and bits (an ActionAttention: in names, layers and both tensors)."""
    if isinstance(a, ActionAttention) or isinstance(b, ActionAttention):
        return (isinstance(a, ActionAttention) and isinstance(b, ActionAttention) and a.names == b.names and a.layers == b.layers
                and same(a.probs, b.probs) and same(a.segments, b.segments))
    if type(a) is not type(b):
        return False
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def kind(x):
    return str(x.dtype).replace("torch.", "")


def pick(att, j):
    """Copies / candidates j (an index or a slice) of a stacked ActionAttention."""
    return ActionAttention(probs=att.probs[:, j], segments=att.segments[:, j], names=att.names, layers=att.layers)


def check_kinds(got, lead, level, count):
    """What each named slot must hold, whatever call it came from; `lead`: the leading dimensions before the N tokens."""
    if "wt" in got:
        assert kind(got["wt"]) == "int64" and tuple(got["wt"].shape) == lead + (N, 2)
    for name in ("range_wt", "bin_wt"):
        if name in got:
            assert kind(got[name]) == "int32" and tuple(got[name].shape) == lead + (N, count)
    v = got["values"]
    assert kind(v) == "float32" and tuple(v.shape) == ((B,) if level == "action" else lead + (N,))
    att = got["attention"]
    assert isinstance(att, ActionAttention) and att.names == ("bos", "image", "text0", "text1", "text2", "generated")
    assert tuple(att.probs.shape[:len(lead) + 1]) == lead + (N,) and tuple(att.segments.shape[:len(lead) + 1]) == lead + (N,)
    assert att.segments.shape[-1] == 6 and att.probs.shape[-1] > 6 and att.probs.dtype == att.segments.dtype == torch.float32


def combined_against_alone(call, order, groups):
    """`call(**kw)` with the keywords of every group at once against the calls with one group's keywords: `order` names the
    elements of the full return, `groups` = {group: (keywords, the names they add)}; names in no group are always returned.
    → the combined return by name."""
    extra = {n for _, names in groups.values() for n in names}

    def run(gs):
        kw = {k: v for g in gs for k, v in groups[g][0].items()}
        names = [n for n in order if n not in extra or any(n in groups[g][1] for g in gs)]
        out = call(**kw)
        out = out if isinstance(out, tuple) else (out,)
        assert len(out) == len(names), (gs, len(out), names)
        return dict(zip(names, out))
    full = run(list(groups))
    assert list(full) == list(order)
    for g in groups:
        for name, x in run([g]).items():
            assert same(x, full[name]), f"{name}: asked for with {g} alone it differs from the combined call's"
    return full


def extras(st, case, level):
    c = st[case]
    return dict(values=(dict(return_values=level), ["values"]),
                attention=(dict(return_attention="both", text_splits=c["splits"]), ["attention"]))


@pytest.mark.parametrize("case,level", CASES)
def test_generate_sampled(st, case, level):
    model, c = st["model"], st[case]
    got = combined_against_alone(
        lambda **kw: model.generate(c["ids"], N, pixel_values=c["pv"], attention_mask=c["mask"], sampling=st["sp"], **kw),
        ["ids", "wt", "values", "attention"], dict(weights=(dict(return_weights=True), ["wt"]), **extras(st, case, level)))
    check_kinds(got, (B,), level, st["count"])
    assert got["ids"].dtype == torch.int64 and tuple(got["ids"].shape) == (B, c["ids"].shape[1] + N)
    assert torch.equal(got["ids"][:, :-N], c["ids"])


@pytest.mark.parametrize("case,level", CASES)
def test_generate_forced(st, case, level):
    model, c = st["model"], st[case]
    got = combined_against_alone(
        lambda **kw: model.generate(c["ids"], N, pixel_values=c["pv"], attention_mask=c["mask"], sampling=st["sp"],
                                    forced_ids=st["forced"], **kw),
        ["ids", "wt", "range_wt", "values", "attention"],
        dict(range=(dict(score_range=(st["first"], st["count"])), ["range_wt"]), **extras(st, case, level)))
    check_kinds(got, (B,), level, st["count"])
    assert torch.equal(got["ids"].cpu(), torch.cat([c["ids"].cpu(), st["forced"]], dim=1))


@pytest.mark.parametrize("case,level", CASES)
def test_predict_action(st, case, level):
    model, c = st["model"], st[case]
    got = combined_against_alone(
        lambda **kw: model.predict_action(input_ids=c["ids"], pixel_values=c["pv"], unnorm_key=KEY, attention_mask=c["mask"],
                                          sampling=st["sp"], **kw),
        ["action", "tokens", "wt", "values", "attention"],
        dict(weights=(dict(return_weights=True), ["tokens", "wt"]), **extras(st, case, level)))
    check_kinds(got, (B,), level, st["count"])
    assert got["tokens"].dtype == np.int64 and got["tokens"].shape == (B, N) and got["action"].shape == (B, N)
    assert np.array_equal(got["action"], model.actions_from_token_ids(got["tokens"], KEY))


@pytest.mark.parametrize("case,level", CASES)
def test_sample_actions(st, case, level):
    model, c, sp = st["model"], st[case], st["sp"]
    got = combined_against_alone(
        lambda **kw: model.sample_actions(c["ids"], c["pv"], KEY, sp, num_samples=K, attention_mask=c["mask"], **kw),
        ["actions", "tokens", "logprobs", "values", "attention"], extras(st, case, level))
    check_kinds(got, (B, K), level, st["count"])
    for name, dtype in (("actions", np.float64), ("tokens", np.int64), ("logprobs", np.float64)):
        assert got[name].dtype == dtype and got[name].shape == (B, K, N), name
    for j in range(K):      # copy j is the one call with copy j's seeds, extras included
        one = S.SamplingParams(temperature=sp.temperature, top_k=sp.top_k, seed=S.derive_seed(sp.seed, j))
        a, tok, wt, v, att = model.predict_action(input_ids=c["ids"], pixel_values=c["pv"], unnorm_key=KEY, attention_mask=c["mask"],
                                                  sampling=one, return_weights=True, return_values=level,
                                                  return_attention="both", text_splits=c["splits"])
        assert same(a, got["actions"][:, j]) and same(tok, got["tokens"][:, j]) and same(S.logprob(wt), got["logprobs"][:, j]), j
        assert same(v, got["values"] if level == "action" else got["values"][:, j]), j
        assert same(att, pick(got["attention"], j)), j
    assert not np.array_equal(got["tokens"][:, 0], got["tokens"][:, 8])


@pytest.mark.parametrize("case,level", CASES)
def test_score_actions(st, case, level):
    model, c, cand = st["model"], st[case], st["cand"]
    sp = S.SamplingParams(temperature=st["sp"].temperature, top_k=st["sp"].top_k)
    call = lambda tok, **kw: model.score_actions(c["ids"], c["pv"], token_ids=tok, sampling=sp, attention_mask=c["mask"], **kw)
    order = ["logprobs", "wt", "bin_wt", "values", "attention"]
    got = combined_against_alone(lambda **kw: call(cand, **kw), order,
                                 dict(bins=(dict(return_bins=True), ["wt", "bin_wt"]), **extras(st, case, level)))
    check_kinds(got, (B, K), level, st["count"])
    assert got["logprobs"].dtype == np.float64 and got["logprobs"].shape == (B, K, N)
    assert np.array_equal(got["logprobs"], S.logprob(got["wt"]))
    for j in range(K):      # candidate j is the one-candidate call, extras included
        one = dict(zip(order, call(cand[:, j], return_bins=True, return_values=level, return_attention="both", text_splits=c["splits"])))
        for name in ("logprobs", "wt", "bin_wt"):
            assert same(one[name], got[name][:, j:j + 1]), (name, j)
        assert same(one["values"], got["values"] if level == "action" else got["values"][:, j:j + 1]), j
        assert same(one["attention"], pick(got["attention"], slice(j, j + 1))), j
