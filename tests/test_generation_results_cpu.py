"""The host-side pieces every generation call shares (no GPU): `engine.present`, the one formatter of the public returns,
and the copy-batching helpers of `sample_actions` / `score_actions` (modeling_prismatic.copy_runs, tile_sampling,
tap_kwargs, stack_runs, stack_values, stack_attention) against the expressions they replaced, written out here."""
import itertools

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd.attention_taps import ActionAttention
from bridgelang_amd.engine import EngineResult, present
from bridgelang_amd.extern.hf import modeling_prismatic as M

BATCHES, COPIES = (1, 2, 3, 16, 17), (1, 8, 9)      # B = 17: 16 // B is 0, the max(1, …) matters; K = 9: a second run at B = 2


def test_record_fields_are_the_documented_order():
    assert EngineResult._fields == ("ids", "wt", "range_wt", "values", "attention")
    assert EngineResult(ids=0) == (0, None, None, None, None)


@pytest.mark.parametrize("pattern", list(itertools.product((False, True), repeat=4)))
def test_formatter_keeps_the_order_and_drops_what_is_absent(pattern):
    parts = [object() for _ in range(5)]                 # the first part (ids / action / logprobs) is always there
    given = [parts[0]] + [p if on else None for p, on in zip(parts[1:], pattern)]
    want = [p for p in given if p is not None]
    got = present(*given)
    if len(want) == 1:
        assert got is parts[0], "one part present: the bare element"
    else:
        assert isinstance(got, tuple) and len(got) == len(want) and all(g is w for g, w in zip(got, want))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("K", COPIES)
def test_copy_helpers_against_what_they_replace(B, K):
    runs = M.copy_runs(B, K)
    per_call = max(1, 16 // B)
    assert [j0 for j0, _ in runs] == list(range(0, K, per_call))
    assert [c for _, c in runs] == [min(per_call, K - j0) for j0 in range(0, K, per_call)] and sum(c for _, c in runs) == K
    # tiled settings: np.tile(T, c), copy j's seeds derive_seed(seed, j); a score has no seed
    T, k, p, seed = S.SamplingParams(temperature=np.linspace(0.5, 1.5, B), top_k=np.arange(B), top_p=np.linspace(0.6, 1.0, B),
                                     seed=np.arange(B) * 7 + 3).resolve(B)
    splits = torch.arange(2 * B).reshape(B, 2)
    for j0, c in runs:
        sp = M.tile_sampling(T, k, p, seed, j0, c)
        assert np.array_equal(sp.temperature, np.tile(T, c)) and np.array_equal(sp.top_k, np.tile(k, c))
        assert np.array_equal(sp.top_p, np.tile(p, c))
        assert np.array_equal(sp.seed, np.concatenate([S.derive_seed(seed, j) for j in range(j0, j0 + c)]))
        assert sp.seed.dtype == np.int64 and sp.seed.shape == (c * B,)
        assert M.tile_sampling(T, k, p, None, j0, c).seed == 0
        assert M.tap_kwargs(None, [1], splits, B, c) == {}
        kw = M.tap_kwargs("both", [1], splits, B, c)
        assert set(kw) == {"return_attention", "attention_layers", "text_splits"} and kw["return_attention"] == "both"
        assert kw["attention_layers"] == [1] and torch.equal(kw["text_splits"], splits.reshape(B, -1).repeat(c, 1))
        assert M.tap_kwargs("full", None, None, B, c)["text_splits"] is None
    # stacking [c·B, …] per run → [B, K, …]
    for tail in ((), (7,), (7, 2)):
        parts, at = [], 0
        for _, c in runs:
            size = c * B * int(np.prod(tail, dtype=np.int64))
            parts.append(np.arange(at, at + size).reshape((c * B,) + tail))
            at += size
        want = np.concatenate([x.reshape((c, B) + tail) for x, (_, c) in zip(parts, runs)], axis=0)
        want = want.transpose((1, 0) + tuple(range(2, want.ndim)))
        got = M.stack_runs(parts, B)
        assert got.shape == (B, K) + tail and got.dtype == want.dtype and np.array_equal(got, want)
        got_t = M.stack_runs([torch.from_numpy(x) for x in parts], B)
        assert got_t.is_contiguous() and torch.equal(got_t, torch.from_numpy(np.ascontiguousarray(want)))
        for j in range(K):      # copy j of sequence b is row j·B + b of the copy-major whole
            assert np.array_equal(got[:, j], np.concatenate(parts, axis=0)[j * B:(j + 1) * B])
    assert M.stack_runs([None] * len(runs), B) is None
    # values: copy 0's at level "action", every copy's at "token"
    act = [np.arange(c * B, dtype=np.float32) + 100 * i for i, (_, c) in enumerate(runs)]
    got = M.stack_values(act, B, "action")
    assert got.shape == (B,) and np.array_equal(got, act[0].reshape(-1, B)[0]) and not np.shares_memory(got, act[0])
    tok = [np.arange(c * B * 7, dtype=np.float32).reshape(c * B, 7) + 1000 * i for i, (_, c) in enumerate(runs)]
    assert np.array_equal(M.stack_values(tok, B, "token"),
                          np.concatenate([v.reshape((c, B, 7)) for v, (_, c) in zip(tok, runs)], axis=0).transpose(1, 0, 2))
    assert M.stack_values([None] * len(runs), B, "action") is None and M.stack_values([None] * len(runs), B, None) is None


@pytest.mark.parametrize("have_probs,have_segments", [(True, True), (True, False), (False, True)])
def test_attention_stacking(have_probs, have_segments):
    B, K, n, nl, H, cache, nseg = 2, 9, 3, 2, 4, 8, 5
    runs = M.copy_runs(B, K)
    g = torch.Generator().manual_seed(3)
    parts = [ActionAttention(probs=torch.rand(c * B, n, nl, H, cache, generator=g) if have_probs else None,
                             segments=torch.rand(c * B, n, nl, H, nseg, generator=g) if have_segments else None,
                             names=("bos", "image", "text", "generated", "x"), layers=(0, 1)) for _, c in runs]

    def cat(ts):        # the reshape `_stack_attention` did
        if ts[0] is None:
            return None
        return torch.cat([t.reshape((t.shape[0] // B, B) + tuple(t.shape[1:])) for t in ts], dim=0).transpose(0, 1).contiguous()
    got = M.stack_attention(parts, B)
    assert got.names == parts[0].names and got.layers == (0, 1)
    for name, shape in (("probs", (B, K, n, nl, H, cache)), ("segments", (B, K, n, nl, H, nseg))):
        want, have = cat([getattr(a, name) for a in parts]), getattr(got, name)
        if want is None:
            assert have is None
        else:
            assert tuple(have.shape) == shape and have.is_contiguous() and torch.equal(have, want)
    assert M.stack_attention([None] * len(runs), B) is None
