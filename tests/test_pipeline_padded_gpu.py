"""StaggeredDecodePipeline(padded=True): batches of right-padded prompts of different lengths ride one set of slots and
graphs. Every batch must come out with exactly the ids and logits of the padded engine run on the same batch, and every
sequence with exactly the ids and logits of its own un-padded batch-1 run — eager and as captured graphs, with and
without the split vision stage, including the drain."""
import pytest
import torch

pytestmark = pytest.mark.gpu

L, N_BATCHES, N_NEW = 12, 11, 7
_REF = {}


def _batches(dims, B):
    """11 right-padded batches: lengths from a fixed seed in 2..12; batch 0 is all full length, batch 1 holds a length-2
    sequence (BOS + the empty token). Returns [(ids [B, L], pixel_values, mask [B, L], lengths)]."""
    from test_engine_gpu import make_inputs
    g = torch.Generator().manual_seed(1234 + B)
    out = []
    for s in range(N_BATCHES):
        ids, pv = make_inputs(dims, B, L, seed=40 + s)
        lens = torch.randint(2, L + 1, (B,), generator=g).tolist()
        if s == 0:
            lens = [L] * B
        if s == 1:
            lens[B - 1] = 2
        mask = torch.zeros(B, L, dtype=torch.long)
        for b, n in enumerate(lens):
            ids[b, n - 1] = 29871
            ids[b, n:] = 32000
            mask[b, :n] = 1
        out.append((ids, pv, mask, lens))
    return out


def _reference(dev, B):
    """Computed once per batch size and shared: per batch the padded engine's ids [B, 7] and logits [7, B, V], and per
    sequence the un-padded batch-1 engine's."""
    if B in _REF:
        return _REF[B]
    from bridgelang_amd import weights as W
    from bridgelang_amd.engine import OpenVLAEngine
    dims = W.tiny_dims()
    w = W.allocate(dims, dev).fill_synthetic(seed=3)
    batches = _batches(dims, B)
    eng = OpenVLAEngine(w, B, L, padded=True)
    alone = {}
    pad_ids, pad_lg, one_ids, one_lg = [], [], [], []
    for ids, pv, mask, lens in batches:
        eng.set_padded_inputs(ids.to(dev), pv.to(dev), mask.to(dev))
        eng.run_eager()
        pad_ids.append(eng.gen_ids.t().clone().cpu())
        pad_lg.append(eng.logits.clone().cpu())
        i1, l1 = [], []
        for b, n in enumerate(lens):
            if n not in alone:
                alone[n] = OpenVLAEngine(w, 1, n)
            i1.append(alone[n].generate(ids[b:b + 1, :n].to(dev), pv[b:b + 1].to(dev)).clone().cpu())
            l1.append(alone[n].logits.clone().cpu())
        one_ids.append(torch.cat(i1, dim=0))
        one_lg.append(torch.cat(l1, dim=1))
    _REF[B] = (w, batches, pad_ids, pad_lg, one_ids, one_lg)
    return _REF[B]


def _pipe(w, B, split, dev, batches, graphs):
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    pipe = StaggeredDecodePipeline(w, B, L, split_vision=split, padded=True)
    if graphs:
        ids, pv, mask, _ = batches[0]
        for e in pipe.engines:
            e.set_padded_inputs(ids.to(dev), pv.to(dev), mask.to(dev))
        pipe.capture()
        assert all(g is not None for g in pipe._graphs) and len(pipe._graphs) == pipe.slots     # every slot rotation
    return pipe


@pytest.mark.parametrize("B,split", [(2, False), (3, True)])
def test_padded_pipeline_matches_padded_engine_and_unpadded_runs(dev, B, split):
    w, batches, pad_ids, pad_lg, one_ids, one_lg = _reference(dev, B)
    for graphs in (False, True):
        pipe = _pipe(w, B, split, dev, batches, graphs)
        tag = f"graphs={graphs}"
        got = []
        for k, (ids, pv, mask, _) in enumerate(batches):
            # batch 0 is all full length: its mask may be left out (None = all ones)
            out = pipe.step(ids.to(dev), pv.to(dev), None if k == 0 else mask.to(dev)).clone()
            if k >= pipe.slots - 1:
                got.append(out.cpu())
            j = k - pipe.lag            # the batch whose prefill ran in this step: first-token logits
            if j >= 0:
                first = pipe.engines[j % pipe.slots].logits[0].cpu()
                assert torch.equal(first, pad_lg[j][0]), f"{tag} step {k}: prefill logits of batch {j} != padded engine"
                assert torch.equal(first, one_lg[j][0]), f"{tag} step {k}: prefill logits of batch {j} != un-padded runs"
            for g in range(1, pipe.n_new):       # this step ran decode iteration g of batch j
                j = k - g - pipe.lag
                if j >= 0:
                    rows = pipe.logits[(g - 1) * B:g * B].cpu()
                    assert torch.equal(rows, pad_lg[j][g]), f"{tag} step {k}: batch {j} iteration {g} != padded engine"
                    assert torch.equal(rows, one_lg[j][g]), f"{tag} step {k}: batch {j} iteration {g} != un-padded runs"
        got += [o.cpu() for o in pipe.flush()]
        assert len(got) == N_BATCHES
        for k in range(N_BATCHES):
            assert torch.equal(got[k], pad_ids[k]), f"{tag} batch {k}: ids differ from the padded engine's"
            assert torch.equal(got[k], one_ids[k]), f"{tag} batch {k} (lengths {batches[k][3]}): ids differ from the un-padded runs'"


@pytest.mark.parametrize("B,split", [(2, False), (3, True)])
def test_padded_pipeline_short_run_drains(dev, B, split):
    """Three submissions, then flush(): exactly those three batches, finished by each slot's own padded plans."""
    w, batches, pad_ids, _, one_ids, _ = _reference(dev, B)
    pipe = _pipe(w, B, split, dev, batches, graphs=False)
    for ids, pv, mask, _ in batches[:3]:
        pipe.step(ids.to(dev), pv.to(dev), mask.to(dev))
    outs = pipe.flush()
    assert len(outs) == 3
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), pad_ids[k]) and torch.equal(o.cpu(), one_ids[k]), f"short run batch {k}"


def test_padded_pipeline_errors(dev):
    from bridgelang_amd.pipeline import StaggeredDecodePipeline
    w, batches, *_ = _reference(dev, 2)
    with pytest.raises(ValueError):
        StaggeredDecodePipeline(w, 2, L, padded=True, fp8=True)
    plain = StaggeredDecodePipeline(w, 2, L)
    ids, pv, mask, _ = batches[0]
    with pytest.raises(ValueError):
        plain.step(ids.to(dev), pv.to(dev), mask.to(dev))
