"""bl_beam_step_f32 and bl_beam_reorder_kv_bf16 (csrc/beam.hip) at their edges. The step is held to bridgelang_amd/beam.py
BIT FOR BIT on the fp32 (not bf16-rounded) rows of gen_edge_ref.beam_case — tokens, parents, both integers of wt and the
score bits — at the widths 4 and 8 (one and two active threads), at the sweep boundary (4096 against 4100), at three and
nine sweeps (8196, 36480: the widest row, whose all-equal row has total = 36480·2^30 > 2^45), and on both ranged forms.
The plants put the two best candidates into one thread's four columns of one row, into the same column group of two
rows, and into columns c and c + 4096 of one row (the owner's holder is ranked again across
sweeps); logits hold −inf, one beam is dead, one prompt has ALL scores −inf (its survivors are the first W flat
indices), one row is peaked (total = 2^30, lz = 0), one has total = 3·2^30 (mantissa above 1.41421354), one score is −1e30.
`assert_beam_census` is asserted before the device is touched. Outputs sit between guards; scores_in must be unchanged.

The reorder is compared bytewise, the whole cache, against a host gather: W·hd/8 = 16 (one slot), 256 (exactly the first
piece), 288 and 512 (head_dim 256: `kReorderPieces`' second piece, partly and fully used), with repeated parents and a
slot that is overwritten while it feeds others, for both forms of row0."""
import numpy as np
import pytest
import torch

import gen_edge_ref as E

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def _guarded(rows, tail, dtype, fill, dev):
    size = rows * int(np.prod(tail, dtype=np.int64))
    flat = torch.full((size + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return flat, flat[GUARD:GUARD + size].view((rows,) + tail)


@pytest.mark.parametrize("groups,W,n,vocab", E.BEAM_SHAPES, ids=["-".join(map(str, s[:3])) for s in E.BEAM_SHAPES])
def test_beam_step_equals_specification(dev, groups, W, n, vocab):
    from bridgelang_amd import ops
    case = E.beam_case(groups, W, n, vocab)
    E.assert_beam_census(groups, case)
    rows = groups * W
    buf = torch.empty(rows, n + 12)
    buf[:, 0::2], buf[:, 1::2] = float("nan"), float("inf")
    buf[:, :n] = torch.from_numpy(case.full.copy())
    logits, s_in = buf.to(dev)[:, :n], torch.from_numpy(case.s.copy()).to(dev)
    runs = []
    for _ in range(2):                                                   # the second launch: identical bits
        tok_f, tok = _guarded(rows, (), torch.int64, -7, dev)
        par_f, par = _guarded(rows, (), torch.int32, -7, dev)
        wt_f, wt = _guarded(rows, (2,), torch.int64, -7, dev)
        sc_f, sc = _guarded(rows, (), torch.float32, 123.0, dev)
        ops.beam_step(logits, W, s_in, tok, par, wt, sc, vocab=vocab)
        torch.cuda.synchronize()
        for flat, fill in ((tok_f, -7), (par_f, -7), (wt_f, -7), (sc_f, 123.0)):
            assert bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all()), "wrote outside its outputs"
        runs.append((tok.cpu().numpy(), par.cpu().numpy(), wt.cpu().numpy(), sc.cpu().numpy().view(np.uint32)))
    got_tok, got_par, got_wt, got_sc = runs[0]
    first, count = vocab if vocab is not None else (0, n)
    assert ((got_par >= 0) & (got_par < W)).all() and ((got_tok >= first) & (got_tok < first + count)).all()
    assert np.array_equal(got_par, case.par) and np.array_equal(got_tok, case.tok), (got_par, case.par, got_tok, case.tok)
    assert np.array_equal(got_wt, case.wt), (got_wt, case.wt)
    assert np.array_equal(got_sc, case.sc.view(np.uint32)), (got_sc.view(np.float32), case.sc)
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1])), "a second launch differs"
    assert np.array_equal(s_in.cpu().numpy().view(np.uint32), case.s.view(np.uint32)), "scores_in changed"


def _parents(W, groups):
    """Per prompt: the identity; every slot from the last; slot 0 feeds slots 1 and 2 and is itself overwritten by the last
    slot's rows (W >= 3); a seeded draw with repeats."""
    rng = np.random.default_rng(W)
    sets = [np.arange(W), np.full(W, W - 1), np.array([W - 1, 0, 0] + list(range(3, W)))[:W] if W >= 3 else np.zeros(W, int),
            rng.integers(0, W, W)]
    return np.concatenate(sets[:groups]).astype(np.int32)


@pytest.mark.parametrize("per_row", [False, True], ids=["row0-host", "row0-device"])
@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("W,hd", [(1, 128), (16, 128), (9, 256), (16, 256)])
def test_reorder_equals_host_gather(dev, W, hd, n_rows, per_row):
    from bridgelang_amd import ops
    H, cache_len, groups = 2, 16, 4
    rows = groups * W
    g = torch.Generator().manual_seed(1000 * W + hd + 10 * n_rows + per_row)
    caches = [torch.randn(rows, H, cache_len, hd, generator=g).to(torch.bfloat16).to(dev) for _ in range(2)]
    before = [c.cpu().clone() for c in caches]
    parents = torch.from_numpy(_parents(W, groups))
    starts = [5, 0, cache_len - n_rows, 9] if per_row else [cache_len - n_rows] * groups     # a prompt's rows share their start
    row0 = torch.tensor([s for s in starts for _ in range(W)], dtype=torch.int32)
    ops.beam_reorder_kv(ops.cache_table(caches), caches, W, parents.to(dev), row0.to(dev) if per_row else starts[0], n_rows)
    torch.cuda.synchronize()
    for c, b in zip(caches, before):
        want = b.clone()
        for e in range(groups):
            for k in range(W):
                src = e * W + int(parents[e * W + k])
                want[e * W + k, :, starts[e]:starts[e] + n_rows] = b[src, :, starts[e]:starts[e] + n_rows]
        assert torch.equal(c.cpu().view(torch.int16), want.view(torch.int16)), "moved rows differ from the gather, or bytes outside them changed"
    if W > 1:
        assert not torch.equal(caches[0].cpu().view(torch.int16), before[0].view(torch.int16))
