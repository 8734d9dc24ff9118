"""One prefill shared by a prompt's rows, the parts that need no device: how `share_prefill=True` splits prompts and copies
over engine runs (`group_runs`, `group_sampling`, `stack_groups`), the argument errors raised before an engine exists, and
the new entry points in the header, the binding and the built library."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd.extern.hf.modeling_prismatic import group_runs, group_sampling, stack_groups

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("B", [1, 2, 3, 5, 16, 17, 40])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 15, 16, 17, 20, 32, 33])
def test_group_runs_cover_every_copy_once_within_16_rows(B, K):
    runs = group_runs(B, K)
    seen = np.zeros((B, K), dtype=np.int64)
    for b0, nb, j0, c in runs:
        assert nb >= 1 and c >= 1 and nb * c <= 16, (b0, nb, j0, c)
        seen[b0:b0 + nb, j0:j0 + c] += 1
        if K <= 16:
            assert (j0, c) == (0, K), "a group of at most 16 rows is never split"
        else:
            assert j0 % 16 == 0 and c == min(16, K - j0), "a larger one is cut into chunks of at most 16 rows"
    assert np.all(seen == 1), "every (prompt, copy) exactly once"
    if K <= 16:         # as many prompts per run as fit
        assert all(nb == min(max(1, 16 // K), B - b0) for b0, nb, _, _ in runs)
        assert len(runs) == -(-B // max(1, 16 // K))


@pytest.mark.parametrize("B,K", [(2, 8), (3, 5), (2, 20), (1, 33), (5, 4)])
def test_group_sampling_seeds_follow_the_copy_whatever_the_chunking(B, K):
    rng = np.random.default_rng(B * 100 + K)
    T, k, p = rng.uniform(0.5, 2.0, B).astype(np.float32), rng.integers(0, 50, B).astype(np.int32), rng.uniform(0.5, 1.0, B).astype(np.float32)
    seed = rng.integers(-2 ** 62, 2 ** 62, B).astype(np.int64)
    runs = group_runs(B, K)
    parts = {name: [] for name in ("T", "k", "p", "seed")}
    for b0, nb, j0, c in runs:
        sp = group_sampling(T, k, p, seed, b0, nb, j0, c)
        rT, rk, rp, rs = sp.resolve(nb * c)
        for name, a in zip(parts, (rT, rk, rp, rs)):
            parts[name].append(np.asarray(a))
        assert np.all(np.asarray(group_sampling(T, k, p, None, b0, nb, j0, c).resolve(nb * c)[3]) == 0), "a score has no seed"
    full = {name: stack_groups(v, runs, B, K) for name, v in parts.items()}
    for j in range(K):
        assert np.array_equal(full["seed"][:, j], S.derive_seed(seed, j)), f"copy {j} draws with derive_seed(seed, {j})"
        assert np.array_equal(full["T"][:, j], T) and np.array_equal(full["k"][:, j], k) and np.array_equal(full["p"][:, j], p)
    assert stack_groups([None] * len(runs), runs, B, K) is None


def test_stack_groups_puts_prompt_major_rows_in_their_place():
    B, K = 3, 20
    runs = group_runs(B, K)
    want = np.arange(B * K * 2).reshape(B, K, 2)
    parts = [want[b0:b0 + nb, j0:j0 + c].reshape(nb * c, 2) for b0, nb, j0, c in runs]
    assert np.array_equal(stack_groups(parts, runs, B, K), want)


@pytest.fixture(scope="module")
def model():
    from bridgelang_amd import weights as Wt
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    stats = {"d": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    m = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=stats), device="cpu", dims=Wt.tiny_dims())

    def no_engine(*a, **k):
        raise AssertionError("an argument error must be raised before an engine is asked for")
    m.engine = no_engine
    return m


def test_surface_refuses_what_a_shared_prefill_does_not_combine_with(model):
    ids, pv = torch.ones(2, 6, dtype=torch.int64), torch.zeros(2, 6, 224, 224)
    mask = torch.ones(2, 6, dtype=torch.int64)
    mask[1, -2:] = 0
    tok = np.full((2, 3, 7), 31800, dtype=np.int64)
    for call, word in ((lambda: model.sample_actions(ids, pv, "d", num_samples=4, attention_mask=mask, share_prefill=True), "padded"),
                       (lambda: model.sample_actions(ids, pv, "d", num_samples=4, return_attention="segments", share_prefill=True), "return_attention"),
                       (lambda: model.score_actions(ids, pv, token_ids=tok, attention_mask=mask, share_prefill=True), "padded"),
                       (lambda: model.score_actions(ids, pv, token_ids=tok, return_attention="full", share_prefill=True), "return_attention"),
                       (lambda: model.beam_actions(ids, pv, "d", num_beams=4, attention_mask=mask, share_prefill=True), "padded"),
                       (lambda: model.generate(ids, 7, pixel_values=pv, num_beams=4, attention_mask=mask, share_prefill=True), "padded"),
                       (lambda: model.generate(ids, 7, pixel_values=pv, forced_ids=torch.from_numpy(tok)), "share_prefill=True"),
                       (lambda: model.generate(ids, 7, pixel_values=pv, group=4), "share_prefill=True")):
        with pytest.raises(ValueError, match=word):
            call()
    model.fp8 = True
    try:
        for call in (lambda: model.sample_actions(ids, pv, "d", num_samples=4, share_prefill=True),
                     lambda: model.beam_actions(ids, pv, "d", num_beams=4, share_prefill=True)):
            with pytest.raises(ValueError, match="fp8"):
                call()
    finally:
        del model.fp8
    for call in (lambda: model.sample_actions(ids, pv, "d", num_samples=4, share_prefill=True),         # valid calls reach the engine
                 lambda: model.score_actions(ids, pv, token_ids=tok, share_prefill=True),
                 lambda: model.beam_actions(ids, pv, "d", num_beams=4, share_prefill=True)):
        with pytest.raises(AssertionError, match="before an engine"):
            call()


def test_engine_refuses_what_a_shared_prefill_does_not_combine_with():
    from bridgelang_amd import weights as Wt
    from bridgelang_amd.attention_taps import AttnTaps
    from bridgelang_amd.engine import OpenVLAEngine
    w = Wt.allocate(Wt.tiny_dims(), "cpu")
    for kw, word in ((dict(padded=True), "padded"), (dict(fp8=True), "e4m3"), (dict(attn_taps=AttnTaps(layers=None, full=True, segments=False)), "attn_taps"),
                     (dict(value="token"), "token"), (dict(all_rows=True), "generation plan"), (dict(vision_only=True), "generation plan"),
                     (dict(text_only=True), "generation plan"), (dict(beams=2), "beams=2"), (dict(group=3), "multiple"),
                     (dict(batch=32, group=2), "fused")):
        kw = {**dict(batch=8, group=4), **kw}
        with pytest.raises(ValueError, match=word):
            OpenVLAEngine(w, kw.pop("batch"), 8, **kw)
    for group in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="group"):
            OpenVLAEngine(w, 16, 8, group=group)


def test_entry_points_are_declared_bound_and_exported():
    from bridgelang_amd import _lib
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    declared = set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", header))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    want = {"bl_attention_decode_rope_shared_bf16": [C.POINTER(_lib.AttnDesc), vp, vp, i32, i32, i32, vp, vp, i32, vp],
            "bl_attention_decode_rope_shared_gq_bf16": [C.POINTER(_lib.AttnDesc), vp, vp, i32, i32, i32, vp, vp, i32, i32, vp],
            "bl_repeat_rows_bf16": [vp, i64, vp, i64, i64, i32, i32, vp]}
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"bl_[a-z0-9_]+", line.split()[-1])}
    lib = _lib.load()
    for name, args in want.items():
        assert name in declared and f"int {name}(" in header and name in exported and hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, args), name
    # the suggested shape of the issue: desc, cos, sin, pos, group, prefix_len, k_gen, v_gen, gen_len, stream
    proto = re.search(r"int bl_attention_decode_rope_shared_bf16\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert names == ["d", "cos_tab", "sin_tab", "pos", "group", "prefix_len", "k_gen", "v_gen", "gen_len", "stream"]
    assert declared == set(_lib.SIGNATURES) == exported, (declared ^ exported, declared ^ set(_lib.SIGNATURES))
    makefile = (ROOT / "bridgelang_amd" / "csrc" / "Makefile").read_text()
    assert "attention_decode_shared.hip" in makefile and "bl_attention_decode_rope_shared_bf16" in (ROOT / "INTEGRATION.md").read_text()
