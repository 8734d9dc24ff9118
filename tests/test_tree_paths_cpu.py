"""What the tree attention tests reach, checked without a GPU through the host model of the kernels' tile schedule
(tests/tree_paths.py): the grid of tests/test_attention_tree_gpu.py does not reach the skip paths beyond 512 rows, every
shape of tests/test_attention_tree_long_gpu.py reaches the path it is there for, and the inputs of every fp64 check of that
file satisfy the precondition |s'| <= 64 of the error model of tests/attn_ref64.py."""
import math

import numpy as np
import pytest
import torch

import tree_paths
from tree_paths import LONG_CASES, masked_paths, paths

LONG = list(LONG_CASES)
LONG_IDS = [f"p{p}-nb{nb}-G{g}" for p, nb, g in LONG]


def test_model_cites_the_source_as_it_stands():
    """Every predicate the model restates is still on the line of attention_tree.hip it was read from."""
    got = tree_paths.cited_lines()
    wrong = {n: (got[n], want) for n, want in tree_paths.CITES.items() if got[n] != want}
    assert not wrong, f"attention_tree.hip moved under tests/tree_paths.py (line: (source, model)): {wrong}"


def test_old_grid_does_not_reach_the_new_paths():
    """If this fails because test_attention_tree_gpu.CASES grew, the old grid now reaches more: update these figures and its
    docstring, which names them as the reason test_attention_tree_long_gpu.py exists."""
    from test_attention_tree_gpu import CASES
    got = [paths(*c) for c in CASES]
    assert all(g["dq_blk_skips"] == 0 for g in got)
    assert max(g["fwd_max"] for g in got) == 1 and sum(g["fwd_skips"] for g in got) == 1
    assert paths(288, 8, 16)["fwd_skips"] == 1
    assert max(g["dkv_max_chunks"] for g in got) == 2 and max(g["dkv_max_start"] for g in got) == 256
    assert max(g["S"] for g in got) == 416
    assert max(c[1] for c in CASES) == 8                   # no branch spans a 16-row wave tile


@pytest.mark.parametrize("case", LONG, ids=LONG_IDS)
def test_new_case_reaches_its_path(case):
    got = paths(*case)
    assert {k: got[k] for k in LONG_CASES[case]} == LONG_CASES[case]


def test_new_cases_cover_what_the_old_grid_misses():
    got = {c: paths(*c) for c in LONG}
    assert min(g["S"] for g in got.values()) > 512
    assert got[(256, 8, 33)]["dq_blk_skips"] == 1                      # the smallest: chunk [256, 512) ends exactly at blk_lo
    assert tree_paths.branch_lo(512, 256, 8) == 512
    assert max(g["dq_blk_max"] for g in got.values()) == 6 and got[(1, 8, 112)]["dq_blk_max"] == 2
    assert sorted({g["dkv_max_chunks"] for g in got.values()}) == [3, 4, 8]
    assert max(g["dkv_max_start"] for g in got.values()) == 1792
    for branch, unit in ((56, tree_paths.WAVE_ROWS), (100, tree_paths.FWD_ROWS), (130, tree_paths.BLK), (300, tree_paths.KC)):
        assert any(nb == branch for _, nb, _ in LONG) and branch > unit   # a branch longer than each tile size
    # a forward skip followed by a branch that starts mid-chunk: the first visited branch chunk holds rows of another branch
    p, nb, G = 33, 7, 100
    mid = [(q0, seen) for q0, seen, skipped in tree_paths.fwd_schedule(p, nb, p + G * nb)
           if skipped and tree_paths.branch_lo(q0, p, nb) % tree_paths.KV_CHUNK]
    assert len(mid) >= 5 and all(min(k for k in seen if k >= p) < tree_paths.branch_lo(q0, p, nb) for q0, seen in mid)


@pytest.mark.parametrize("case", LONG, ids=LONG_IDS)
def test_schedule_drops_no_visible_pair(case):
    """The model's own sanity: every (query, key) pair tree_visible allows lies in a chunk / step the schedule visits, in all
    three kernels — a skip bound as restated here drops nothing. (That the kernels do as the model says is the GPU tests'.)"""
    from bridgelang_amd.training.shared_prompt import tree_visible
    prefix, branch, G = case
    vis = tree_visible(prefix, branch, prefix + G * branch)
    for kernel, seen in tree_paths.visited(prefix, branch, G).items():
        assert not bool((vis & ~seen).any()), f"{kernel}: the schedule skips a visible pair"


@pytest.mark.parametrize("case", LONG, ids=LONG_IDS)
def test_tree_visible_is_the_predicate(case):
    """tree_visible against a double-loop restatement of the predicate, under the default mask of batch element 1."""
    from bridgelang_amd.training.shared_prompt import tree_visible
    from test_attention_tree_gpu import _mask
    prefix, branch, G = case
    S = prefix + G * branch
    mask = _mask(prefix, branch, G)[1].numpy().tolist()
    got = tree_visible(prefix, branch, S, mask)
    for i in range(S):
        want = [bool(mask[j]) and j <= i and (j < prefix or (i >= prefix and (i - prefix) // branch == (j - prefix) // branch))
                for j in range(S)]
        assert got[i].tolist() == want, f"row {i}"


def _checks():
    from test_attention_tree_long_gpu import CHECKS
    return CHECKS


@pytest.mark.parametrize("name", list(_checks()))
def test_inputs_satisfy_the_error_models_precondition(name):
    """attn_ref64 derives C_O … C_DK for |s'| = |q·k|·scale·log2e <= 64 over visible pairs. A condition on the inputs, not a
    tolerance: a case that exceeds it gets another seed."""
    from test_attention_tree_gpu import HD, case_inputs
    from test_attention_tree_long_gpu import check_mask
    prefix, branch, G, _, seed = _checks()[name]
    q, k, _, vis = case_inputs(prefix, branch, G, check_mask(name), seed, name.endswith("peaked"))
    worst = 0.0
    for b in range(q.shape[0]):
        s = (q[b].double() @ k[b].double().transpose(-1, -2)).abs() * (HD ** -0.5 / math.log(2.0))
        worst = max(worst, float(s.masked_fill(~vis[b], 0.0).max()))
    print(f"{name}: max |s'| over visible pairs {worst:.1f}")
    assert 0.0 < worst <= 64.0


def test_masked_chunk_and_steps_are_reached():
    from test_attention_tree_long_gpu import check_mask
    mask = check_mask("masked-chunk-flat")
    assert masked_paths(288, 8, 32, mask[1].numpy()) == dict(fwd_chunks=1, dq_steps=4)     # chunk [192, 256); steps 160 … 287
    assert masked_paths(288, 8, 32, mask[0].numpy()) == dict(fwd_chunks=0, dq_steps=0)
    # the old grid's masks hide at most 5 prefix rows: nothing is ever fully masked
    from test_attention_tree_gpu import CASES, _mask
    for p, nb, g in CASES:
        assert masked_paths(p, nb, g, _mask(p, nb, g, hide_prefix=(2, 5))[1].numpy()) == dict(fwd_chunks=0, dq_steps=0)
    short = check_mask("short-long-branches-flat")
    assert int((short[1] == 0).sum()) == 5 + 5 * 37


def test_bounds_are_attn_ref64s():
    """Both tree test files compare with attn_ref64's comparators and constants; the values are pinned here."""
    import attn_ref64 as A
    import test_attention_tree_gpu as TG
    assert (TG.C_O, TG.C_DV, TG.C_DQ, TG.C_DK, TG.FLOOR) == (A.C_O, A.C_DV, A.C_DQ, A.C_DK, A.FLOOR) == (1.25, 1.25, 1.5, 1.5, 2.0 ** -110)
    assert A.LSE_REL == 2.0 ** -18 and A.U == 2.0 ** -8
    assert TG.assert_attn_close is A.assert_attn_close and TG.assert_lse_close is A.assert_lse_close
