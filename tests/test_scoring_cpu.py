"""Scoring GIVEN tokens under the sampled policy — the specification side (bridgelang_amd/sampling.py::score_row,
score_rows, logprob, range_entropy) and the action tokenizer's encoding (`token_ids_from_actions`) on the CPU. Every
comparison is exact. The device kernel is held to `score_rows` bit for bit in tests/test_scoring_gpu.py, which takes its
rows, forced tokens and hard-class census from the helpers here."""
import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S

V = 32064
GRID = [(T, k, p) for T in (0.5, 1.0, 2.0) for k in (0, 8, 50) for p in (0.5, 0.9, 0.95, 1.0)]     # test_sampling_cpu.py's
HARD = ("boundary_kept", "boundary_dropped", "kth_kept", "below_kth", "weight_zero", "greedy_tied_not_first")


def bf16_logits(seed, n=V, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(torch.bfloat16).float().numpy()


# ---- rows, forced tokens and the census of hard classes (shared with the GPU test) -----------------------------------------
def wave_span(n):
    """Indices per wave in the kernel's walk: 16 waves, contiguous spans, a multiple of 64."""
    return ((n + 15) // 16 + 63) & ~63


def planted_rows(rows, n, seed):
    """`_rows` of test_sampling_gpu.py (planted ties at the k-th value, coarse logits, ties at the maximum, all-equal
    rows) + per-row seeds; two more plants where rows allow: a greedy row whose maximum is tied (its forced token will be
    the LAST of the ties), and a coarse top-p row."""
    from test_sampling_gpu import _rows
    l, T, k, p, seeds = _rows(rows, n, seed)
    if rows > 4:
        l[4, [n // 3, n // 2, n - 2]] = l[4].max()                  # row 4 is greedy (T[4::9] = 0)
    if rows > 2:
        l[2] = np.round(l[2])                                         # coarser still: many tokens share the boundary weight
        p[2] = 0.9
    return l, T, k, p, seeds


def _tie_set(l, T, k, p):
    """Indices that share the row's boundary value, in index order: the top-p boundary weight where top-p cuts; else the
    k-th largest logit where top-k cuts; else (and on greedy rows) the maximum."""
    n = l.shape[0]
    if not np.float32(T) > 0:
        return np.flatnonzero(l == l.max())
    if np.float32(p) < np.float32(1.0):
        after_k = S.kept_weights(l, T, int(k), 1.0)
        kept = S.kept_weights(l, T, int(k), float(p))
        return np.flatnonzero(after_k == kept[kept > 0].min())
    if 0 < k < n:
        return np.flatnonzero(l == np.sort(l)[-int(k)])
    return np.flatnonzero(l == l.max())


def forced_tokens(l, T, k, p, seeds, step):
    """One token per row, cycling: the specification's own draw, the first and the last index at the boundary value,
    argmin, argmax, an index in the last wave's span. Row 4 (greedy, tied maximum) takes the last of its ties."""
    rows, n = l.shape
    span = wave_span(n)
    last_lo = (n - 1) // span * span
    tok = np.zeros(rows, np.int64)
    for r in range(rows):
        c = (r + r // 6) % 6
        if r == 4 and rows > 4:
            c = 2
        if c == 0:
            tok[r] = S.sample_row(l[r], T[r], k[r], p[r], int(seeds[r]), step)[0]
        elif c in (1, 2):
            tok[r] = _tie_set(l[r], T[r], k[r], p[r])[0 if c == 1 else -1]
        elif c == 3:
            tok[r] = int(np.argmin(l[r]))
        elif c == 4:
            tok[r] = int(np.argmax(l[r]))
        else:
            tok[r] = last_lo + (r * 7) % (n - last_lo)
    return tok


def hard_classes(l, T, k, p, tok):
    """Census on the SPECIFICATION's output alone: class name → rows whose forced token falls in it."""
    out = {name: [] for name in HARD}
    for r in range(l.shape[0]):
        n, t = l.shape[1], int(tok[r])
        w, total = S.score_row(l[r], T[r], k[r], p[r], t)
        if not np.float32(T[r]) > 0:
            if l[r, t] == l[r].max() and t != int(np.argmax(l[r])):
                assert (w, total) == (0, 1)
                out["greedy_tied_not_first"].append(r)
            continue
        if S.weights(l[r], T[r])[t] == 0:
            assert w == 0
            out["weight_zero"].append(r)
            continue
        if 0 < k[r] < n:
            kth = np.sort(l[r])[-int(k[r])]
            if l[r, t] == kth and w > 0:
                out["kth_kept"].append(r)
            if l[r, t] < kth:
                assert w == 0
                out["below_kth"].append(r)
        if np.float32(p[r]) < np.float32(1.0):
            after_k = S.kept_weights(l[r], T[r], int(k[r]), 1.0)
            kept = S.kept_weights(l[r], T[r], int(k[r]), float(p[r]))
            wstar = kept[kept > 0].min()
            cut = bool(np.any((after_k == wstar) & (kept == 0)))    # the boundary falls AMONG equal weights
            if after_k[t] == wstar and cut:
                out["boundary_kept" if w > 0 else "boundary_dropped"].append(r)
    return out


def assert_hard_classes_present(census):
    empty = [name for name in HARD if not census[name]]
    assert not empty, f"no forced token in the classes {empty}: {({n: len(v) for n, v in census.items()})}"


# ---- the defining property ---------------------------------------------------------------------------------------------------
def test_round_trip_with_the_sampler():
    """Whatever `sample_row` draws, `score_row` of that token returns its pair: 200 rows over the grid, 3 seeds each."""
    for case in range(200):
        T, k, p = GRID[case % len(GRID)]
        l = bf16_logits(3000 + case)
        for seed in (case, -7 * case - 1, (1 << 63) - case):
            tok, w, total = S.sample_row(l, T, k, p, seed, case % 7)
            assert S.score_row(l, T, k, p, tok) == (w, total), (case, seed)
    l = bf16_logits(9, n=512)
    l[[400, 17, 300]] = l.max() + 1
    assert S.sample_row(l, 0.0, 50, 0.5, 1, 0) == (17, 1, 1) and S.score_row(l, 0.0, 50, 0.5, 17) == (1, 1)


def test_score_rows_is_kept_weights_indexed():
    rows, n = 40, 260
    l, T, k, p, seeds = planted_rows(rows, n, seed=5)
    tok = forced_tokens(l, T, k, p, seeds, step=2)
    wt, full = S.score_rows(l, T, k, p, tok, 0, n)
    part = S.score_rows(l, T, k, p, tok, 100, 37)[1]
    none = S.score_rows(l, T, k, p, tok)[1]
    assert wt.dtype == np.int64 and full.dtype == np.int32 and full.shape == (rows, n) and none.shape == (rows, 0)
    for r in range(rows):
        if T[r] > 0:
            kept = S.kept_weights(l[r], T[r], int(k[r]), float(p[r]))
        else:
            kept = np.zeros(n, np.int64)
            kept[np.flatnonzero(l[r] == l[r].max())[0]] = 1           # one-hot at the LOWEST index of the maximum
        assert wt[r].tolist() == [kept[tok[r]], kept.sum()] and np.array_equal(full[r], kept)
        assert full[r].astype(np.int64).sum() == wt[r, 1]             # Σ over the full range = total_kept
        assert np.array_equal(part[r], kept[100:137])
        assert S.score_row(l[r], T[r], k[r], p[r], tok[r]) == tuple(wt[r].tolist())
    assert (T == 0).sum() >= 4
    for bad in (dict(first=-1, count=2), dict(first=n - 1, count=2), dict(first=0, count=-1)):
        with pytest.raises(ValueError):
            S.score_rows(l, T, k, p, tok, **bad)
    with pytest.raises(ValueError):
        S.score_rows(l, T, k, p, np.full(rows, n))


@pytest.mark.parametrize("rows,n", [(256, V), (64, 260)])
def test_hard_classes_are_present(rows, n):
    """The rows the GPU test scores put a forced token into every class where the kernel could go wrong — decided on the
    specification's output alone."""
    l, T, k, p, seeds = planted_rows(rows, n, seed=rows + n)
    tok = forced_tokens(l, T, k, p, seeds, step=3)
    census = hard_classes(l, T, k, p, tok)
    print({name: len(v) for name, v in census.items()})
    assert_hard_classes_present(census)
    span = wave_span(n)
    assert np.any(tok >= (n - 1) // span * span) and span % 64 == 0


# ---- logprob, entropy ----------------------------------------------------------------------------------------------------------
def test_logprob_of_zero_weight_is_minus_inf_without_warning():
    rng = np.random.default_rng(1)
    total = rng.integers(1, 1 << 45, 5000)
    w = (total * rng.random(5000)).astype(np.int64).clip(1, None)
    wt = np.stack([w, total], axis=-1)
    with np.errstate(all="raise"):
        got = S.logprob(wt)
        assert np.array_equal(got, np.log(w.astype(np.float64) / total.astype(np.float64)))        # unchanged bit for bit
        assert np.array_equal(S.logprob(wt.reshape(50, 100, 2)), got.reshape(50, 100))
        assert S.logprob(np.array([S.WEIGHT_ONE, S.WEIGHT_ONE])) == 0.0 and S.logprob(np.array([1, 1])) == 0.0
        mixed = S.logprob(np.array([[0, 7], [3, 7], [0, 1]]))
        assert mixed[0] == -np.inf and mixed[2] == -np.inf and mixed[1] == np.log(3 / 7)
        assert S.logprob(np.array([0, 5])) == -np.inf


def test_range_entropy():
    with np.errstate(all="raise"):
        ent, mass = S.range_entropy(np.array([[1, 1, 0, 2], [0, 0, 0, 4], [1, 0, 0, 0]], np.int32), np.array([4, 4, 4]))
        assert np.array_equal(mass, [1.0, 1.0, 0.25])
        assert ent[0] == -(2 * 0.25 * np.log(0.25) + 0.5 * np.log(0.5)) and ent[1] == 0.0 and ent[2] == -0.25 * np.log(0.25)
        l = bf16_logits(4, n=260)
        wt, rw = S.score_rows(l[None], [1.0], [0], [0.9], [int(l.argmax())], 0, 260)
        ent, mass = S.range_entropy(rw, wt[:, 1])
        assert ent.dtype == np.float64 and mass[0] == 1.0 and 0 < ent[0] < np.log(260)


# ---- the action tokenizer's encoding -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"bridge_orig": {"action": {"q01": [-0.5, -0.1, -2.0, 0.0, -1.0, -0.3, 0.0], "q99": [0.7, 0.1, 3.0, 1.5, 1.0, 0.9, 1.0],
                                        "mask": [True] * 6 + [False]}}}
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device="cpu", dims=W.tiny_dims())


def test_token_ids_from_actions_inverts_actions_from_token_ids(model):
    vs = model.vocab_size
    tok = np.repeat(np.arange(vs - 255, vs)[:, None], 7, axis=1)                  # every decodable token in every dimension
    actions = model.actions_from_token_ids(tok, "bridge_orig")
    back = model.token_ids_from_actions(actions, "bridge_orig")
    assert back.dtype == np.int64 and np.array_equal(back, tok)
    assert np.array_equal(model.token_ids_from_actions(actions.reshape(5, 51, 7), "bridge_orig"), tok.reshape(5, 51, 7))
    st = model.get_action_stats("bridge_orig")
    lo, hi = np.array(st["q01"]), np.array(st["q99"])
    # masked-off dimension (the gripper): the value itself is binned, not its position between q01 and q99
    a = np.tile((lo + hi) / 2, (3, 1))
    a[:, 6] = [-1.0, 0.25, 1.0]
    got = model.token_ids_from_actions(a, "bridge_orig")[:, 6]
    assert got.tolist() == (vs - np.digitize([-1.0, 0.25, 1.0], model.bins)).tolist()
    # beyond q01 / q99: the end bins
    below, above = model.token_ids_from_actions(lo - 5.0, "bridge_orig"), model.token_ids_from_actions(hi + 5.0, "bridge_orig")
    assert np.all(below[:6] == vs - 1) and np.all(above[:6] == vs - 256)
    assert below[6] == vs - 1 and above[6] == vs - 256                            # the unmasked value is clipped to [-1, 1] too
    assert np.array_equal(model.token_ids_from_actions(lo - 1e-3, "bridge_orig")[:6], model.token_ids_from_actions(lo, "bridge_orig")[:6])
    with pytest.raises(ValueError):
        model.token_ids_from_actions(np.zeros(6), "bridge_orig")
