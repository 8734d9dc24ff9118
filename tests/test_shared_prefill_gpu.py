"""One prefill shared by a prompt's samples, candidates and beams: bl_attention_decode_rope_shared_bf16 against the existing
decode kernel on replicated caches (bit for bit, guarded buffers), its argument checks, the group= engine against the
replicated engine (ids, weight pairs, logits: torch.equal, eager and captured), beams, the critic, and share_prefill=True on
the model surface against share_prefill=False."""
import ctypes as C

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from test_sampling_gpu import L, _ctx, _params

pytestmark = pytest.mark.gpu

H, HD = 2, 128
D = H * HD
GUARD = 4096


def _rand(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, device=dev) * scale).to(torch.bfloat16)


def _guarded(shape, gen, dev):
    """A contiguous bf16 tensor of `shape` inside a flat buffer with GUARD random elements on either side."""
    size = int(np.prod(shape))
    flat = _rand((size + 2 * GUARD,), gen, dev)
    return flat, flat[GUARD:GUARD + size].view(shape)


@pytest.fixture(scope="module")
def rope(dev):
    from bridgelang_amd.engine import rope_tables
    return rope_tables(HD, 2048, 10000.0, dev)


# (prefix_len, generated rows already present): the issue's grid, then pos = 320 | 321 on either side of the resident /
# streaming switch, with the generated rows inside one 64-key group and across two
PREFIX_GEN = [(pl, g) for pl in (1, 63, 64, 65, 267, 314) for g in (0, 1, 5)] + [(315, 5), (320, 0), (316, 5), (321, 0), (300, 21)]


# Long caches: pos = 2047 is the last position of the rope table, where 8 rows per workgroup hold 8 x 2048 scores + 8 x 4 x 128
# partial sums = 80 KiB of LDS (the limit the launcher raises to 96 KiB); the others put 100 … 200 generated rows into
# three or four 64-key groups, behind a streamed (1500) and a resident (1, 63) prefix
LONG_PREFIX_GEN = [(2000, 47), (1500, 100), (1, 200), (63, 130)]


@pytest.mark.parametrize("P,G", [(1, 1), (1, 16), (3, 5), (2, 3), (16, 1)])
def test_kernel_equals_the_existing_kernel_on_replicated_caches(dev, rope, P, G):
    assert {pl + g for pl, g in PREFIX_GEN} >= {320, 321}
    _kernel_against_replicated_caches(dev, rope, P, G, PREFIX_GEN)


@pytest.mark.parametrize("P,G", [(1, 8), (2, 3)])
def test_kernel_equals_the_existing_kernel_on_long_caches(dev, rope, P, G):
    assert max(pl + g for pl, g in LONG_PREFIX_GEN) == 2047 == rope[0].shape[0] - 1
    assert (8 * 2048 + 8 * 4 * 128) * 4 > 64 * 1024 and all(g > 64 for pl, g in LONG_PREFIX_GEN[1:])
    _kernel_against_replicated_caches(dev, rope, P, G, LONG_PREFIX_GEN)


def _kernel_against_replicated_caches(dev, rope, P, G, prefix_gen):
    from bridgelang_amd import ops
    cos, sin = rope
    R = P * G
    gen = torch.Generator(device=dev).manual_seed(1000 * P + G)
    for prefix_len, n_gen in prefix_gen:
        pos = prefix_len + n_gen
        cache_len, gen_len, ref_len = (prefix_len + 63) // 64 * 64, n_gen + 2, (pos + 1 + 63) // 64 * 64
        qkv = _rand((R, 3 * D), gen, dev)
        kp_f, kp = _guarded((P, H, cache_len, HD), gen, dev)
        vp_f, vp = _guarded((P, H, cache_len, HD), gen, dev)
        kg_f, kg = _guarded((R, H, gen_len, HD), gen, dev)
        vg_f, vg = _guarded((R, H, gen_len, HD), gen, dev)
        # the reference: every row's own cache = its prompt's rows, then its generated rows; row `pos` on holds noise
        kr, vr = _rand((R, H, ref_len, HD), gen, dev), _rand((R, H, ref_len, HD), gen, dev)
        for ref, pc, gc in ((kr, kp, kg), (vr, vp, vg)):
            ref[:, :, :prefix_len] = pc[:, :, :prefix_len].repeat_interleave(G, dim=0)
            ref[:, :, prefix_len:pos] = gc[:, :, :n_gen]
        o_ref = torch.zeros(R, D, dtype=torch.bfloat16, device=dev)
        ops.attention_decode_rope(qkv, kr, vr, o_ref, cos, sin, B=R, H=H, head_dim=HD, pos=pos)
        before = [t.clone() for t in (kp_f, vp_f, kg_f, vg_f)]
        for gq in (None, 2, 4, 8):
            tag = f"P={P} G={G} prefix={prefix_len} gen={n_gen} gq={gq}"
            for t, b in zip((kp_f, vp_f, kg_f, vg_f), before):
                t.copy_(b)
            o_f, o = _guarded((R, D), gen, dev)
            o_before = o_f.clone()
            ops.attention_decode_rope_shared(qkv, kp, vp, kg, vg, o, cos, sin, group=G, H=H, head_dim=HD, prefix_len=prefix_len,
                                             pos=pos, gq=gq)
            assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), f"{tag}: o"
            assert torch.equal(kg[:, :, n_gen].view(torch.int16), kr[:, :, pos].view(torch.int16)), f"{tag}: appended k row"
            assert torch.equal(vg[:, :, n_gen].view(torch.int16), vr[:, :, pos].view(torch.int16)), f"{tag}: appended v row"
            # every other byte: the prompt caches whole, the gen caches but for row n_gen, and all guards
            assert torch.equal(kp_f.view(torch.int16), before[0].view(torch.int16)), f"{tag}: prompt k cache written"
            assert torch.equal(vp_f.view(torch.int16), before[1].view(torch.int16)), f"{tag}: prompt v cache written"
            for now, b in ((kg_f, before[2]), (vg_f, before[3])):
                want = b.clone()
                want[GUARD:GUARD + R * H * gen_len * HD].view(R, H, gen_len, HD)[:, :, n_gen] = \
                    now[GUARD:GUARD + R * H * gen_len * HD].view(R, H, gen_len, HD)[:, :, n_gen]
                assert torch.equal(now.view(torch.int16), want.view(torch.int16)), f"{tag}: gen cache written outside row {n_gen}"
            assert torch.equal(o_f[:GUARD].view(torch.int16), o_before[:GUARD].view(torch.int16)) and \
                torch.equal(o_f[GUARD + R * D:].view(torch.int16), o_before[GUARD + R * D:].view(torch.int16)), f"{tag}: o guards"


def test_repeat_rows_kernel(dev):
    from bridgelang_amd import ops
    gen = torch.Generator(device=dev).manual_seed(7)
    for rows, group, width in ((1, 1, 8), (3, 5, 512), (2, 16, 520), (5, 3, 4096)):
        wide = _rand((rows, 2, width), gen, dev)
        for src in (wide[:, 0].contiguous(), wide[:, 1]):          # dense rows, and rows with a stride (a [B, S, D] last row)
            d_f, dst = _guarded((rows * group, width), gen, dev)
            want = d_f.clone()
            want[GUARD:GUARD + rows * group * width] = src.repeat_interleave(group, dim=0).reshape(-1)
            ops.repeat_rows(src, dst, group)
            assert torch.equal(d_f.view(torch.int16), want.view(torch.int16)), (rows, group, width)
    with pytest.raises(ValueError):
        ops.repeat_rows(wide[:, 0], torch.zeros(7, 4096, dtype=torch.bfloat16, device=dev), 3)


def test_kernel_argument_checks(dev, rope):
    """Every argument the entry point rejects returns its error code and launches nothing: o, and the caches, keep their bytes."""
    from bridgelang_amd import _lib, ops
    cos, sin = rope
    lib = _lib.load()
    gen = torch.Generator(device=dev).manual_seed(3)
    P, G, prefix_len, gen_len, cache_len = 2, 4, 20, 6, 64
    R = P * G
    qkv = _rand((R, 3 * D), gen, dev)
    kp, vp = _rand((P, H, cache_len, HD), gen, dev), _rand((P, H, cache_len, HD), gen, dev)
    kg, vg = _rand((R, H, gen_len, HD), gen, dev), _rand((R, H, gen_len, HD), gen, dev)
    o = _rand((R, D), gen, dev)
    mask = torch.ones(R, 64, dtype=torch.uint8, device=dev)
    keep = [t.clone() for t in (kp, vp, kg, vg, o)]
    cs = (H * cache_len * HD, cache_len * HD, HD)

    def call(pos=22, group=G, prefix=prefix_len, glen=gen_len, rows=R, hd=HD, key_mask=None, k_hs=None, kgen=kg, cos_t=cos, gq=None):
        d = ops._attn_desc(qkv, kp, vp, o, rows, H, 1, pos + 1, hd, (3 * D, HD, 3 * D),
                           cs if k_hs is None else (cs[0], k_hs, cs[2]), cs, (D, HD, D), False, HD ** -0.5, key_mask)
        args = (C.byref(d), None if cos_t is None else cos_t.data_ptr(), sin.data_ptr(), pos, group, prefix,
                None if kgen is None else kgen.data_ptr(), vg.data_ptr(), glen)
        stream = torch.cuda.current_stream().cuda_stream
        if gq is None:
            return lib.bl_attention_decode_rope_shared_bf16(*args, stream)
        return lib.bl_attention_decode_rope_shared_gq_bf16(*args, gq, stream)

    SHAPE, ARG = _lib.BL_E_SHAPE, _lib.BL_E_ARG
    bad = [("head_dim 64", dict(hd=64), SHAPE), ("group 0", dict(group=0), SHAPE), ("group 17", dict(group=17, rows=17), SHAPE),
           ("rows % group", dict(group=3), SHAPE), ("prefix_len 0", dict(prefix=0), SHAPE), ("pos < prefix_len", dict(pos=19), SHAPE),
           ("gen cache full", dict(pos=prefix_len + gen_len), SHAPE), ("pos 2048", dict(pos=2048, prefix=2045), SHAPE),
           ("prefix beyond a cache head", dict(k_hs=16 * HD), SHAPE), ("key mask", dict(key_mask=mask), ARG),
           ("null gen cache", dict(kgen=None), ARG), ("null rope table", dict(cos_t=None), ARG), ("gq 3", dict(gq=3), ARG)]
    for what, kw, code in bad:
        assert call(**kw) == code, what
    torch.cuda.synchronize()
    for t, b in zip((kp, vp, kg, vg, o), keep):
        assert torch.equal(t.view(torch.int16), b.view(torch.int16)), "a rejected call wrote something"
    assert call() == _lib.BL_OK and call(gq=8) == _lib.BL_OK
    torch.cuda.synchronize()
    assert not torch.equal(o.view(torch.int16), keep[4].view(torch.int16))
    # the tensor front end refuses the same with a reason, before the library is reached
    for kw in (dict(group=17), dict(prefix_len=0), dict(pos=prefix_len + gen_len), dict(pos=prefix_len - 1)):
        with pytest.raises(ValueError):
            ops.attention_decode_rope_shared(qkv, kp, vp, kg, vg, o, cos, sin, **{**dict(group=G, H=H, head_dim=HD, prefix_len=prefix_len, pos=22), **kw})


# ---- the group= engine against the replicated engine ---------------------------------------------------------------------------
ACTION_RANGE = (31744, 256)


def _row_params(rows, salt):
    """`_params`' mixed settings (a greedy row among them) over `rows` rows, every row with a seed of its own."""
    T, k, p, _ = _params(4, salt).resolve(4)
    return S.SamplingParams(temperature=np.resize(T, rows), top_k=np.resize(k, rows), top_p=np.resize(p, rows),
                            seed=[salt * 1000 + 17 * r - 5 for r in range(rows)])


def _forced(rows, n_new, salt, dev):
    g = torch.Generator().manual_seed(900 + salt)
    return torch.randint(ACTION_RANGE[0], sum(ACTION_RANGE), (rows, n_new), generator=g, dtype=torch.int64).to(dev)


def _same_run(a, b, tag):
    assert torch.equal(a.gen_ids, b.gen_ids), f"{tag}: gen_ids"
    for name in ("gen_wt", "gen_range_wt"):
        x, y = getattr(a, name, None), getattr(b, name, None)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), f"{tag}: {name}"
    for t in range(a.n_new):
        assert torch.equal(a.logits[t].view(torch.int32), b.logits[t].view(torch.int32)), f"{tag}: logits of step {t}"


@pytest.mark.parametrize("mode", ["sample", "score", "greedy"])
@pytest.mark.parametrize("P,G", [(1, 4), (3, 5), (2, 8)])
def test_engine_equals_replicated_engine(dev, P, G, mode):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    assert c["dims"].vocab >= sum(ACTION_RANGE)
    R = P * G
    kw = dict(sample=dict(sample=True), score=dict(score=True, score_range=ACTION_RANGE), greedy={})[mode]
    grp, rep = OpenVLAEngine(c["w"], R, L, group=G, **kw), OpenVLAEngine(c["w"], R, L, **kw)
    assert grp.P == P and grp.pixel_values.shape[0] == P and grp.k_cache[0].shape[0] == P and grp.k_gen[0].shape[:3] == (R, 4, grp.n_new - 1)
    names = [o.name for o in grp.all_ops()]
    assert names.count("bl_attention_decode_rope_shared_bf16") == (grp.n_new - 1) * c["dims"].llm_layers
    assert names.count("bl_repeat_rows_bf16") == 1 and "bl_attention_decode_rope_bf16" not in names

    def feed(seed, salt):
        ids, pv = c["make_inputs"](c["dims"], P, L, seed=seed)
        ids, pv = ids.to(dev), pv.to(dev)
        for e, (i, p) in ((grp, (ids, pv)), (rep, (ids.repeat_interleave(G, dim=0), pv.repeat_interleave(G, dim=0)))):
            if mode != "greedy":
                e.set_sampling(_row_params(R, salt))
            if mode == "score":
                e.set_forced_ids(_forced(R, e.n_new, salt, dev))
            e.set_inputs(i, p)
            e.replay()
        torch.cuda.synchronize()

    feed(61, 1)
    _same_run(grp, rep, "eager")
    first = grp.logits.clone()
    grp.capture(), rep.capture()
    feed(62, 2)
    _same_run(grp, rep, "captured, new inputs")
    assert not torch.equal(first, grp.logits), "the replay saw the new inputs"
    feed(61, 1)
    _same_run(grp, rep, "captured, first inputs again")
    assert torch.equal(first.view(torch.int32), grp.logits.view(torch.int32))
    with pytest.raises(ValueError):         # the P prompts, not the P·G rows
        grp.set_inputs(rep.input_ids, rep.pixel_values)


def test_engine_beams_equal_replicated_beams(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    from test_beam_gpu import _branches
    c = _ctx(dev)
    feeds = [c["make_inputs"](c["dims"], 1, L, seed=s) for s in (41, 42)]     # seed 41: the run test_beam_gpu proves to reorder
    ids, pv = torch.cat([f[0] for f in feeds]).to(dev), torch.cat([f[1] for f in feeds]).to(dev)
    grp, rep = OpenVLAEngine(c["w"], 8, L, beams=4, group=4), OpenVLAEngine(c["w"], 8, L, beams=4)
    for tag in ("eager", "captured"):
        if tag == "captured":
            grp.capture(), rep.capture()
        a, b = grp.generate(ids, pv), rep.generate(ids, pv)
        torch.cuda.synchronize()
        ta, tb = grp.beam_trace(), rep.beam_trace()
        assert _branches(tb.parents.cpu().numpy(), 4), "the run must reorder something"
        assert torch.equal(ta.tokens, tb.tokens) and torch.equal(ta.parents, tb.parents) and torch.equal(ta.wt, tb.wt), tag
        assert torch.equal(ta.scores.view(torch.int32), tb.scores.view(torch.int32)), tag
        ra, rb = grp.result(), rep.result()
        assert torch.equal(a, b) and torch.equal(ra.ids, rb.ids) and torch.equal(ra.wt, rb.wt), tag
        assert torch.equal(grp.logits.view(torch.int32), rep.logits.view(torch.int32)), tag
    names = [o.name for o in grp.all_ops()]
    assert names.count("bl_beam_reorder_kv_bf16") == grp.n_new - 2


def test_engine_critic_on_the_prompt_rows(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.training.value_head import ValueHead
    c = _ctx(dev)
    P, G = 3, 5
    vh = ValueHead(c["dims"].llm_dim, dev, init_std=0.05, seed=3)
    grp = OpenVLAEngine(c["w"], P * G, L, group=G, sample=True, value="action", value_head=vh)
    rep = OpenVLAEngine(c["w"], P * G, L, sample=True, value="action", value_head=vh)
    ids, pv = c["make_inputs"](c["dims"], P, L, seed=63)
    params = _row_params(P * G, 4)
    grp.generate(ids.to(dev), pv.to(dev), params)
    rep.generate(ids.to(dev).repeat_interleave(G, dim=0), pv.to(dev).repeat_interleave(G, dim=0), params)
    torch.cuda.synchronize()
    assert tuple(grp.values.shape) == (1, P) and tuple(grp.result().values.shape) == (P,)
    assert torch.equal(grp.values[0].view(torch.int32), rep.values[0][::G].view(torch.int32)) and bool((grp.values != 0).all())
    _same_run(grp, rep, "with the critic")


def test_engine_rejects_what_a_shared_prefill_does_not_combine_with(dev):
    from bridgelang_amd.attention_taps import AttnTaps
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.training.value_head import ValueHead
    c = _ctx(dev)
    vh = ValueHead(c["dims"].llm_dim, dev, init_std=0.05, seed=3)
    for kw in (dict(padded=True), dict(fp8=True), dict(attn_taps=AttnTaps(None, True, True)), dict(value="token", value_head=vh),
               dict(all_rows=True), dict(vision_only=True), dict(text_only=True), dict(beams=2), dict(group=3), dict(group=0),
               dict(group=17), dict(group=2.5), dict(batch=32, group=2)):
        kw = {**dict(batch=8, group=4), **kw}
        with pytest.raises(ValueError, match="group"):
            OpenVLAEngine(c["w"], kw.pop("batch"), L, **kw)


# ---- surface -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from test_lora_inference_gpu import new_model
    return new_model(dev)


def _inputs(model, dev, batch, seed=71):
    from test_engine_gpu import make_inputs
    ids, pv = make_inputs(model.dims, batch, 10, seed=seed)
    return ids.to(dev), pv.to(dev)


def _same(a, b, what):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)      # bytes, so that -inf, NaN and -0 count as they are
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: element {i}"


def _surface_calls(model, ids, pv, **kw):
    """Every surface call of the issue, once per value of share_prefill → {name: results}."""
    sp = S.SamplingParams(temperature=[1.0, 0.7], top_k=[0, 40], top_p=[0.95, 1.0], seed=[11, -5])
    first, count = model.action_token_range()
    cand = np.random.default_rng(5).integers(first, first + count, size=(2, 3, 7))
    out = {}
    for share in (False, True):
        k = dict(share_prefill=share, **kw)
        out[share] = dict(
            sample8=model.sample_actions(ids, pv, "bridge_orig", sampling=sp, num_samples=8, **k),
            sample20=model.sample_actions(ids, pv, "bridge_orig", sampling=sp, num_samples=20, action_tokens_only=True, **k),
            score=model.score_actions(ids, pv, token_ids=cand, sampling=sp, return_bins=True, **k),
            beams=model.beam_actions(ids, pv, "bridge_orig", num_beams=4, **k))
    return out


def test_surface_share_prefill_equals_the_replicated_calls(model, dev):
    ids, pv = _inputs(model, dev, 2)
    out = _surface_calls(model, ids, pv)
    for name in out[False]:
        _same(out[True][name], out[False][name], name)
    assert out[True]["sample20"][1].shape == (2, 20, 7) and out[True]["sample8"][2].dtype == np.float64
    assert any(("group", 4) in k and ("beams", 4) in k for k in model._engines), "group engines live in the model's LRU, keyed by group"
    # generate: beams, and K candidates per prompt as forced_ids [B, K, n]
    a = model.generate(ids, 7, pixel_values=pv, num_beams=4, num_return_sequences=2, return_weights=True, share_prefill=True)
    b = model.generate(ids, 7, pixel_values=pv, num_beams=4, num_return_sequences=2, return_weights=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(model.predict_action(ids, "bridge_orig", pixel_values=pv, num_beams=4, share_prefill=True),
                          model.predict_action(ids, "bridge_orig", pixel_values=pv, num_beams=4))
    forced = torch.from_numpy(out[False]["sample8"][1][:, :3].copy()).to(dev)
    prompt = model.with_empty_token(ids)
    got = model.generate(prompt, 7, pixel_values=pv, forced_ids=forced, share_prefill=True)
    want = model.generate(prompt.repeat_interleave(3, dim=0), 7, pixel_values=pv.repeat_interleave(3, dim=0), forced_ids=forced.reshape(6, 7))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # no silent fall-back
    mask = torch.ones_like(ids)
    mask[1, -2:] = 0
    for call in (lambda: model.sample_actions(ids, pv, "bridge_orig", num_samples=4, attention_mask=mask, share_prefill=True),
                 lambda: model.sample_actions(ids, pv, "bridge_orig", num_samples=4, return_attention="segments", share_prefill=True),
                 lambda: model.score_actions(ids, pv, token_ids=forced.cpu().numpy(), attention_mask=mask, share_prefill=True),
                 lambda: model.score_actions(ids, pv, token_ids=forced.cpu().numpy(), return_attention="full", share_prefill=True),
                 lambda: model.beam_actions(ids, pv, "bridge_orig", num_beams=4, attention_mask=mask, share_prefill=True),
                 lambda: model.generate(prompt, 7, pixel_values=pv, forced_ids=forced)):
        with pytest.raises(ValueError):
            call()


def test_surface_under_adapters_and_with_values(model, dev):
    from bridgelang_amd.training.value_head import ValueHead
    from test_lora_inference_gpu import dyadic_adapters
    ids, pv = _inputs(model, dev, 2, seed=72)
    model.attach_adapters(dyadic_adapters(model))
    model.attach_value_head(ValueHead(model.dims.llm_dim, dev, init_std=0.05, seed=3))
    try:
        out = _surface_calls(model, ids, pv, return_values="action")
        for name in out[False]:
            _same(out[True][name], out[False][name], f"adapters + values: {name}")
            assert out[True][name][-1].shape == (2,) and np.all(out[True][name][-1] != 0)
        base = model.sample_actions(ids, pv, "bridge_orig", sampling=S.SamplingParams(seed=3), num_samples=4, use_adapters=False, share_prefill=True)
        _same(base, model.sample_actions(ids, pv, "bridge_orig", sampling=S.SamplingParams(seed=3), num_samples=4, use_adapters=False), "base policy")
        with pytest.raises(ValueError):
            model.sample_actions(ids, pv, "bridge_orig", num_samples=4, return_values="token", share_prefill=True)
    finally:
        model.detach_value_head()
        model.detach_adapters()
