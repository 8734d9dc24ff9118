"""bl_sample_f32 and everything built on it, held to the specification bridgelang_amd/sampling.py BIT FOR BIT: the kernel
on planted ties and poisoned padding, the sample=True engine (eager, captured, right-padded, batch-invariant), the
staggered pipeline against the engine, and the model surface (`generate(sampling=)`, `predict_action`, `sample_actions`)."""
import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S

pytestmark = pytest.mark.gpu

V = 32064
GRID = [(T, k, p) for T in (0.5, 1.0, 2.0) for k in (0, 8, 50) for p in (0.5, 0.9, 0.95, 1.0)]


# ---- kernel against specification ----------------------------------------------------------------------------------------
def _rows(rows, n, seed):
    """bf16-rounded randn·3 logits with per-row settings cycling the grid (+ greedy rows), and planted hard cases."""
    g = torch.Generator().manual_seed(seed)
    l = (torch.randn(rows, n, generator=g) * 3).to(torch.bfloat16).float().numpy()
    T, k, p = (np.array([GRID[r % len(GRID)][c] for r in range(rows)]) for c in range(3))
    T[4::9] = 0.0                                                     # greedy rows between the sampled ones
    seeds = np.random.default_rng(seed).integers(-(1 << 63), (1 << 63) - 1, rows, dtype=np.int64)
    for r in range(rows):
        if r % 4 == 1 and k[r]:                                       # exact ties AT the k-th largest value, spread over the row
            kth = np.sort(l[r])[-int(k[r])]
            l[r, (np.arange(5) * 97 + r) % n] = kth
        if r % 4 == 2:                                                # coarse logits: the top-p boundary falls among equal weights
            l[r] = np.round(l[r] * 2) / 2
        if r % 4 == 3:
            l[r, (np.arange(3) * 131 + r) % n] = l[r].max()           # ties at the maximum (the greedy rule, the first rank)
    if rows > 7:
        l[7] = -1.25                                                  # all-equal rows: with top-p and top-k, and plain
        T[7], k[7], p[7] = 1.0, 8, 0.5
    if rows > 11:
        l[11] = 3.0
        T[11], k[11], p[11] = 2.0, 0, 1.0
    if rows > 20:
        k[20] = n + 5                                                 # top_k >= n: off
        p[21] = 1e-6                                                  # only the first-ranked token survives
    return l, T.astype(np.float32), k.astype(np.int32), p.astype(np.float32), seeds


@pytest.mark.parametrize("rows,n", [(256, V), (256, 260), (1, V), (5, 260)])
def test_kernel_equals_specification(dev, rows, n):
    """ids and both integers of wt; ld > n with +inf in the padding columns, which must not be read."""
    from bridgelang_amd import ops
    l, T, k, p, seeds = _rows(rows, n, seed=rows + n)
    step = 3
    want_ids, want_wt = S.sample_rows(l, T, k, p, seeds, step)
    ld = n + 12
    buf = torch.full((rows, ld), float("inf"), dtype=torch.float32)
    buf[:, :n] = torch.from_numpy(l)
    buf = buf.to(dev)
    ids = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    wt = torch.full((rows, 2), -1, dtype=torch.int64, device=dev)
    d = lambda a: torch.from_numpy(a).to(dev)
    ops.sample(buf[:, :n], d(T), d(k), d(p), d(seeds), step, ids, wt)
    got_ids, got_wt = ids.cpu().numpy(), wt.cpu().numpy()
    bad = np.flatnonzero((got_ids != want_ids) | (got_wt != want_wt).any(axis=1))
    assert bad.size == 0, [(int(r), float(T[r]), int(k[r]), float(p[r]), int(got_ids[r]), int(want_ids[r]), got_wt[r].tolist(),
                            want_wt[r].tolist()) for r in bad[:8]]
    greedy = T == 0
    assert np.array_equal(got_ids[greedy], l[greedy].argmax(-1)) and (got_wt[greedy] == 1).all()
    if rows > 1:
        arg = torch.empty(rows, dtype=torch.int64, device=dev)
        ops.argmax(buf[:, :n], arg)
        assert np.array_equal(got_ids[greedy], arg.cpu().numpy()[greedy])          # a greedy row IS bl_argmax_f32's answer


def test_kernel_rejects_shapes_it_cannot_hold(dev):
    from bridgelang_amd import ops
    from bridgelang_amd._lib import BridgeLangHipError
    def run(n):
        z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=dev)
        ops.sample(z(torch.float32, 2, n), z(torch.float32, 2), z(torch.int32, 2), z(torch.float32, 2), z(torch.int64, 2), 0,
                   z(torch.int64, 2), z(torch.int64, 2, 2))
    with pytest.raises(BridgeLangHipError, match="BL_E_SHAPE"):
        run(36484)                        # beyond what the LDS layout holds
    with pytest.raises(BridgeLangHipError, match="BL_E_SHAPE"):
        run(262)                          # n % 4 != 0
    with pytest.raises(TypeError):
        z = torch.zeros(2, device=dev)
        ops.sample(torch.zeros(2, 8, device=dev), z, z, z, z, 0, z, z)


# ---- tiny-model engine -----------------------------------------------------------------------------------------------------
B, L = 3, 11
_CTX = {}


def _ctx(dev):
    if not _CTX:
        from bridgelang_amd import weights as W
        from test_engine_gpu import make_inputs
        dims = W.tiny_dims()
        _CTX.update(dims=dims, w=W.allocate(dims, dev).fill_synthetic(seed=5), make_inputs=make_inputs)
    return _CTX


def _params(batch, salt):
    """Mixed per-sequence settings, one greedy row when the batch has three."""
    T = [1.0, 2.0, 0.0, 0.5][:batch]
    return S.SamplingParams(temperature=T, top_k=[50, 0, 8, 0][:batch], top_p=[0.95, 0.9, 1.0, 1.0][:batch],
                            seed=[salt * 1000 + 17 * b - 5 for b in range(batch)])


def _check_against_spec(eng, params, tag):
    """The run's own logits, copied to the host, through the specification step by step."""
    T, k, p, seed = params.resolve(eng.B)
    logits = eng.logits.cpu().numpy()
    ids, wt = eng.gen_ids.cpu().numpy(), eng.gen_wt.cpu().numpy()
    for t in range(eng.n_new):
        want_ids, want_wt = S.sample_rows(logits[t], T, k, p, seed, t)
        assert np.array_equal(ids[t], want_ids) and np.array_equal(wt[t], want_wt), f"{tag}: step {t}"
    return ids.T.copy(), wt.transpose(1, 0, 2).copy()


def test_engine_sampling_eager_captured_and_batch_invariant(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    ids, pv = c["make_inputs"](c["dims"], B, L, seed=21)
    eng = OpenVLAEngine(c["w"], B, L, sample=True)
    one = OpenVLAEngine(c["w"], 1, L, sample=True)
    greedy = OpenVLAEngine(c["w"], B, L)
    runs = []
    for salt, captured in ((1, False), (2, True), (3, True)):
        if captured and eng._graph is None:
            eng.capture()
        params = _params(B, salt)
        out = eng.generate(ids.to(dev), pv.to(dev), params)
        torch.cuda.synchronize()
        got_ids, got_wt = _check_against_spec(eng, params, f"captured={captured} salt={salt}")
        assert np.array_equal(out.cpu().numpy(), got_ids)
        runs.append(got_ids)
        T, k, p, seed = params.resolve(B)
        for b in range(B):                                     # the project's batch-invariance rule, for ids AND weights
            pb = S.SamplingParams(float(T[b]), int(k[b]), float(p[b]), int(seed[b]))
            alone = one.generate(ids[b:b + 1].to(dev), pv[b:b + 1].to(dev), pb).cpu().numpy()
            assert np.array_equal(alone[0], got_ids[b]), f"salt {salt}: sequence {b} differs from its batch-1 run"
            assert np.array_equal(one.gen_wt.cpu().numpy()[:, 0], got_wt[b])
    assert not np.array_equal(runs[1], runs[2])                # one graph, other seeds: other tokens
    want = greedy.generate(ids.to(dev), pv.to(dev)).cpu().numpy()
    got = eng.generate(ids.to(dev), pv.to(dev), S.SamplingParams(temperature=0.0)).cpu().numpy()
    assert np.array_equal(got, want) and torch.equal(eng.logits, greedy.logits)         # T = 0 serves greedy bit for bit
    # the sampling plan is the greedy plan with every argmax replaced by the draw; the default plan has no draw in it
    assert [o.name.replace("bl_argmax_f32", "bl_sample_f32") for o in greedy.all_ops()] == [o.name for o in eng.all_ops()]
    assert sum(o.name == "bl_argmax_f32" for o in greedy.all_ops()) == eng.n_new == sum(o.name == "bl_sample_f32" for o in eng.all_ops())
    with pytest.raises(ValueError):
        greedy.set_sampling(S.SamplingParams())


def test_engine_sampling_right_padded(dev):
    from bridgelang_amd.engine import OpenVLAEngine
    c = _ctx(dev)
    ids, pv = c["make_inputs"](c["dims"], B, L, seed=22)
    lens = [L, 4, 8]
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, n - 1] = 29871
        ids[b, n:] = 32000
        mask[b, :n] = 1
    eng = OpenVLAEngine(c["w"], B, L, padded=True, sample=True)
    params = _params(B, 4)
    eng.set_sampling(params)
    eng.set_padded_inputs(ids.to(dev), pv.to(dev), mask.to(dev))
    eng.run_eager()
    got_ids, got_wt = _check_against_spec(eng, params, "padded")
    T, k, p, seed = params.resolve(B)
    for b, n in enumerate(lens):
        one = OpenVLAEngine(c["w"], 1, n, sample=True)
        alone = one.generate(ids[b:b + 1, :n].to(dev), pv[b:b + 1].to(dev),
                             S.SamplingParams(float(T[b]), int(k[b]), float(p[b]), int(seed[b]))).cpu().numpy()
        assert np.array_equal(alone[0], got_ids[b]) and np.array_equal(one.gen_wt.cpu().numpy()[:, 0], got_wt[b]), \
            f"padded sequence {b} (length {n}) differs from its un-padded batch-1 run"


# ---- pipeline --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_pipeline_equals_engine(dev, padded):
    """Every submitted batch comes out with the ids and wt of OpenVLAEngine(sample=True) on that batch: through the captured
    slot rotations and through the drain. Batch 2 is submitted without settings (all greedy) and equals the greedy pipeline."""
    from bridgelang_amd.engine import OpenVLAEngine
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    c = _ctx(dev)
    PB, PL, N = 2, 12, 10
    g = torch.Generator().manual_seed(77)
    batches = []
    for s in range(N):
        ids, pv = c["make_inputs"](c["dims"], PB, PL, seed=60 + s)
        mask = torch.ones(PB, PL, dtype=torch.long)
        if padded and s != 0:
            for b, n in enumerate(torch.randint(2, PL + 1, (PB,), generator=g).tolist()):
                ids[b, n - 1] = 29871
                ids[b, n:] = 32000
                mask[b, n:] = 0
        batches.append((ids.to(dev), pv.to(dev), mask.to(dev), None if s == 2 else _params(PB, 10 + s)))
    eng = OpenVLAEngine(c["w"], PB, PL, padded=padded, sample=True)
    want = []
    for ids, pv, mask, sp in batches:
        eng.set_sampling(sp if sp is not None else S.SamplingParams(temperature=0.0))
        if padded:
            eng.set_padded_inputs(ids, pv, mask)
        else:
            eng.set_inputs(ids, pv)
        eng.run_eager()
        want.append((eng.gen_ids.t().clone().cpu(), eng.gen_wt.permute(1, 0, 2).clone().cpu()))

    def drive(pipe, sample):
        ids, pv, mask, _ = batches[0]
        for e in pipe.engines:
            e.set_padded_inputs(ids, pv, mask) if padded else e.set_inputs(ids, pv)
        pipe.capture()
        got = []
        for s, (ids, pv, mask, sp) in enumerate(batches):
            kw = dict(sampling=sp) if sample else {}
            out = pipe.step(ids, pv, mask, **kw) if padded else pipe.step(ids, pv, **kw)
            if s >= pipe.slots - 1:
                got.append(tuple(o.clone().cpu() for o in out) if sample else out.clone().cpu())
        return got + [tuple(o.cpu() for o in x) if sample else x.cpu() for x in pipe.flush()]

    got = drive(StaggeredDecodePipeline(c["w"], PB, PL, padded=padded, sample=True), True)
    assert len(got) == N
    for s in range(N):
        assert torch.equal(got[s][0], want[s][0]), f"batch {s}: ids differ from the engine's"
        assert torch.equal(got[s][1], want[s][1]), f"batch {s}: weight pairs differ from the engine's"
    greedy = drive(StaggeredDecodePipeline(c["w"], PB, PL, padded=padded), False)
    assert torch.equal(greedy[2], got[2][0]) and bool((got[2][1] == 1).all())
    if not padded:
        with pytest.raises(ValueError):
            StaggeredDecodePipeline(c["w"], PB, PL).step(batches[0][0], batches[0][1], sampling=S.SamplingParams())


# ---- surface ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}}}
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device=dev, dims=W.tiny_dims()).init_synthetic(seed=11)


def test_sample_actions_and_generate_surface(model, dev):
    from test_engine_gpu import make_inputs
    ids, pv = make_inputs(model.dims, 2, 10, seed=31)
    ids, pv = ids.to(dev), pv.to(dev)
    sp = S.SamplingParams(temperature=[1.0, 2.0], top_k=[50, 0], top_p=[0.95, 1.0], seed=[123, -9])
    actions, tokens, lp = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=4)
    assert actions.shape == (2, 4, 7) and tokens.shape == (2, 4, 7) and lp.shape == (2, 4, 7) and lp.dtype == np.float64
    assert np.all(lp <= 0) and np.all(np.isfinite(lp))
    for j in range(4):                                                 # copy j = one predict_action call with the derived seed
        spj = S.SamplingParams(sp.temperature, sp.top_k, sp.top_p, seed=S.derive_seed(np.array(sp.seed), j))
        a, tok, wt = model.predict_action(ids, "bridge_orig", pixel_values=pv, sampling=spj, return_weights=True)
        assert np.array_equal(a, actions[:, j]) and np.array_equal(tok, tokens[:, j])
        assert np.array_equal(S.logprob(wt), lp[:, j]) and np.array_equal(np.log(wt[..., 0] / wt[..., 1]), lp[:, j])
        assert np.array_equal(model.predict_action(ids, "bridge_orig", pixel_values=pv, sampling=spj), a)
    again = model.sample_actions(ids, pv, "bridge_orig", sp, num_samples=4)
    assert all(np.array_equal(x, y) for x, y in zip(again, (actions, tokens, lp)))      # same seeds, same result
    hot = S.SamplingParams(temperature=2.0, seed=[1, 2])
    other = S.SamplingParams(temperature=2.0, seed=[3, 4])
    assert not np.array_equal(model.sample_actions(ids, pv, "bridge_orig", hot)[1], model.sample_actions(ids, pv, "bridge_orig", other)[1])
    # generate(): prompt ‖ new tokens; a right-padded batch gives every sequence its own un-padded result
    full = model.with_empty_token(ids)
    out, wt = model.generate(full, 7, pixel_values=pv, sampling=sp, return_weights=True)
    assert tuple(out.shape) == (2, full.shape[1] + 7) and np.array_equal(out[:, -7:].cpu().numpy(), tokens[:, 0])
    short = torch.cat([full[1:, :5], torch.full((1, 1), 29871, device=dev), torch.full((1, full.shape[1] - 6), 32000, device=dev)], dim=1)
    both = torch.cat([full[:1], short], dim=0)
    mask = torch.ones_like(both)
    mask[1, 6:] = 0
    padded = model.generate(both, 7, pixel_values=pv, attention_mask=mask, sampling=sp)[:, -7:].cpu().numpy()
    alone = model.generate(short[:, :6], 7, pixel_values=pv[1:], sampling=S.SamplingParams(2.0, 0, 1.0, -9))[:, -7:].cpu().numpy()
    assert np.array_equal(padded[0], tokens[0, 0]) and np.array_equal(padded[1], alone[0])
    torch.manual_seed(3)
    a = model.generate(full, 7, pixel_values=pv, sampling=S.SamplingParams(temperature=2.0))
    torch.manual_seed(3)
    b = model.generate(full, 7, pixel_values=pv, sampling=S.SamplingParams(temperature=2.0))
    assert torch.equal(a, b)                                           # seed=None honours torch.manual_seed
    with pytest.raises(NotImplementedError, match="sampling="):
        model.generate(full, 7, pixel_values=pv, do_sample=True)
