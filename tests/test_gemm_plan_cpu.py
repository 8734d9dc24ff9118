"""The GEMM planner (csrc/gemm_plan.h) on the CPU: every shape → form statement of the repository, and plan invariants.

gemm_plan.h is plain host C++17 (no HIP header); the test compiles it with a few-line main that reads shapes and prints the
form code and the launches of each plan. The shape → form tables are imported from the tests that assert them on the GPU
(through ops.gemm_last_form()), with the workspace sizes and leading dimensions those tests use, so a moved threshold shows
here which of them went stale. The sweep covers both sides of every threshold of the planners; over it every plan must
keep to the LDS of a CU, to the workspace it was given and to the tile count of its problem, and the forms it reaches
must be the ones tests/test_gemm_ref_gpu.py has a per-element case for.
"""
import os
import re
import subprocess
from pathlib import Path

import pytest

from test_fused_decode_gpu import ROWS_FORMS, ROWS_STREAM_FORMS
from test_gemm_ref_cpu import ROWS_CASES, SKINNY_KS, TN_CASES
from test_gemm_ref_gpu import ALL_FORMS, SWIGLU_UNREACHABLE, TILE_ALL
from test_ops_gpu import MID_ROWS_FORMS, RING8_MAIN, RING8_TAILS, WORKSPACE_FORMS
from test_train_ops_gpu import TRAIN_EPI_FORMS

ROOT = Path(__file__).resolve().parents[1]
MIB = 1 << 20
LDS_PER_CU = 160 * 1024                     # CDNA4
# kernel families of gemm_plan.h (the KN_* enum)
(KN_GEMM128, KN_RING8, KN_MID, KN_MID2, KN_GEMM288S, KN_GEMM256S, KN_TILE_REDUCE, KN_SLAB_REDUCE, KN_ROWS_STREAM,
 KN_ROWS_STREAM_HALVES, KN_TREE_REDUCE, KN_SKINNY, KN_GEMM256S_FP8) = range(1, 14)

MAIN = r"""
#include "gemm_plan.h"
#include <cstdio>
#include <cstring>
int main() {   // tile | rows | skinny | fp8: M N K lda ws flag    tn: T M N lda ldw ws    (ws < 0: none)
  char what[16];
  long long v[6];
  while (scanf("%15s %lld %lld %lld %lld %lld %lld", what, v, v + 1, v + 2, v + 3, v + 4, v + 5) == 7) {
    using namespace blplan;
    const bool tn = !strcmp(what, "tn");
    const GemmShape g = tn ? GemmShape{(int)v[1], (int)v[2], (int)v[0], v[3], v[4], v[5] < 0 ? 0 : v[5], true}
                           : GemmShape{(int)v[0], (int)v[1], (int)v[2], v[3], v[2], v[4] < 0 ? 0 : v[4], v[5] != 0};
    const GemmPlan p = tn ? plan_gemm_tn(g) : what[0] == 't' ? plan_gemm(g) : what[0] == 'r' ? plan_rows(g) : what[0] == 'f' ? plan_gemm_fp8(g)
                                                                                                     : plan_skinny(g, v[5] != 0);
    printf("%d", p.form);
    for (int i = 0; i < p.n; ++i) {
      const Launch& l = p.l[i];
      printf(" | %d %d %d %d %d %d %d %d %d %d %d %d %d", kid_family(l.kernel), kid_a(l.kernel), kid_b(l.kernel), kid_c(l.kernel),
             l.grid_x, l.grid_y, l.block, l.lds, l.tiles_m, l.tiles_n, l.tail_base, l.splitk, l.ptiles);
    }
    printf("\n");
  }
  return 0;
}
"""
FIELDS = ("family", "a", "b", "c", "grid_x", "grid_y", "block", "lds", "tiles_m", "tiles_n", "tail_base", "splitk", "ptiles")


@pytest.fixture(scope="module")
def planner():
    """shapes → [(form name, launches)]: gemm_plan.h and MAIN compiled with the strict host line, no ROCm path."""
    from bridgelang_amd import ops
    tmp = Path(os.environ.get("TMPDIR", "/tmp"))
    exe = tmp / f"bl_gemm_plan_{os.getpid()}"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", str(ROOT / "bridgelang_amd" / "csrc"),
                    "-x", "c++", "-", "-o", str(exe)], input=MAIN.encode(), check=True)

    def run(shapes):
        text = "".join(" ".join(str(x) for x in s) + "\n" for s in shapes)
        out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True).stdout.decode().splitlines()
        assert len(out) == len(shapes)
        plans = []
        for line in out:
            code, *ls = line.split(" | ")
            plans.append((ops.gemm_form_name(int(code)), [dict(zip(FIELDS, map(int, l.split()))) for l in ls]))
        return plans

    yield run
    exe.unlink()


def tile(M, N, K, ws=-1, lda=None):
    return ("tile", M, N, K, lda or K, ws, 1)


def rows(M, N, K, ws=-1, stream=1, lda=None):
    return ("rows", M, N, K, lda or K, ws, stream)


def tn(T, M, N, ws=-1, lda=None, ldw=None):
    return ("tn", T, M, N, lda or M, ldw or N, ws)


def fp8(M, N, K, ws=-1, lda=None):
    """K and lda count e4m3 codes; bl_gemm_fp8 plans, as its kernel addresses, in 2-byte units."""
    return ("fp8", M, N, K // 2, (lda or K) // 2, ws, 1)


# ---- every shape → form statement of the repository -------------------------------------------------------------------------
def test_shape_to_form_tables(planner):
    want, shapes = [], []

    def expect(form, shape):
        want.append(form)
        shapes.append(shape)

    ws_ref = 128 * MIB                                           # workspace() of tests/test_gemm_ref_gpu.py; its A has lda = K + 8
    for form, M, N, K, use_ws in TILE_ALL:
        # at N and at the SwiGLU width (unsliced mid<4|5, .> exists only for N % 32 != 0: no SwiGLU case there)
        for n in {N} if form in SWIGLU_UNREACHABLE else {N, N if N % 32 == 0 else N + 16}:
            expect(form, tile(M, n, K, ws_ref if use_ws else -1, K + 8))
    for form, N, K, use_ws, row_counts in ROWS_CASES:
        for M in row_counts:
            for n in {N, N if N % 32 == 0 else N + 32 - N % 32}:
                expect(form, rows(M, n, K, ws_ref if use_ws else -1, lda=K + 8))
    for form, T, M, N, use_ws in TN_CASES:
        expect(form, tn(T, M, N, ws_ref if use_ws else -1, M + 8, N + 16))
    for K, ks in SKINNY_KS.items():
        for M, N in ((1, 16), (16, 4112)):
            expect(f"skinny<KS={ks}>", ("skinny", M, N, K, K, -1, 0))
            expect(f"skinny<KS={ks}>+norm", ("skinny", M, N, K, K, -1, 1))
    expect("none", ("skinny", 16, 4112, 640, 640, -1, 0))        # no instantiation: the caller falls back
    for (M, N, K), (form_ws, form_plain) in WORKSPACE_FORMS.items():
        expect(form_ws, tile(M, N, K, 64 * MIB))
        expect(form_plain, tile(M, N, K))
    for mnk, main in RING8_MAIN.items():
        expect(f"{main}+tail{RING8_TAILS[mnk]}", tile(*mnk))
    for mnk, form in MID_ROWS_FORMS.items():
        expect(form, tile(*mnk))
    for mnk, form in TRAIN_EPI_FORMS.items():
        expect(form, tile(*mnk))
    for (M, N, K), (form_plain, form_ws) in ROWS_FORMS.items():
        expect(form_plain, rows(M, N, K))
        expect(form_ws, rows(M, N, K, 4 * M * N * 4))
        expect(f"skinny<KS={K // 256}>", ("skinny", min(M, 16), N, K, K, -1, 0))
    for (M, N, K), forms in ROWS_STREAM_FORMS.items():
        for has_ws in (False, True):
            ws = 4 * M * N * 4 if has_ws else -1
            expect(forms[has_ws], rows(M, N, K, ws, stream=1))
            expect("rows_mid<SK=8>", rows(M, N, K, ws, stream=0))
    got = [form for form, _ in planner(shapes)]
    wrong = [(s, w, g) for s, w, g in zip(shapes, want, got) if w != g]
    assert not wrong, "\n".join(f"{s}: the table says {w}, the planner {g}" for s, w, g in wrong)
    # the 700-row calls of test_gemm_mid_rows take a tile kernel
    assert not any(form.startswith("mid") for form, _ in planner([tile(700, N, K) for _, N, K in MID_ROWS_FORMS]))


# ---- bl_gemm_fp8: one launch of gemm256s_fp8_kernel, whatever the shape -------------------------------------------
FP8_SHAPES = [(1, 16, 128), (256, 256, 256), (300, 528, 384), (2344, 512, 128), (4608, 22016, 4096)]


def test_fp8_plan_is_one_launch(planner):
    for ws in (-1, 64 * MIB):                                    # bl_gemm_fp8 takes no workspace; a size changes nothing
        plans = planner([fp8(M, N, K, ws, K + 16) for M, N, K in FP8_SHAPES])
        for (M, N, K), (form, launches) in zip(FP8_SHAPES, plans):
            tm, tn_ = (M + 255) // 256, (N + 255) // 256
            assert form == "gemm256s_fp8", (M, N, K, ws)
            assert launches == [dict(family=KN_GEMM256S_FP8, a=0, b=0, c=0, grid_x=tm * tn_, grid_y=1, block=512, lds=131072,
                                     tiles_m=tm, tiles_n=tn_, tail_base=-1, splitk=1, ptiles=0)], (M, N, K, ws)


# ---- the sweep: both sides of every threshold ---------------------------------------------------------------------------------
SWEEP_M = [1, 16, 17, 32, 33, 96, 97, 128, 129, 256, 257, 320, 321, 640, 641, 700, 2048, 2081, 2290, 4100, 4353, 4608, 8192, 8352, 18432]
SWEEP_K = [64, 448, 512, 576, 1024, 1088, 2112, 4096, 4160, 8192, 8256, 11008, 13824]
SWEEP_WS = [-1, MIB, 64 * MIB, 128 * MIB]
# N: 64·160 and 64·400 column slabs; one, two and three rounds of 256-column tiles at 16 row tiles; 256 weight tiles; 8·200
# and 6·200 tiles of the rows form — 16 below (N % 32 != 0), at and 16 above each; then the models' widths (Llama-2 7B and
# 13B, the ViT towers, the tiny model) and a few-tile N
MODEL_N = [64, 256, 512, 576, 768, 1024, 1072, 1152, 1536, 1728, 3072, 3456, 4304, 5120, 11008, 13824, 15360, 22016, 27648, 32064]
SWEEP_N = sorted({n + d for n in (64 * 160, 64 * 400, 4096, 8192, 12288, 16 * 8 * 200 - 112, 16 * 6 * 200 - 80) for d in (-16, 0, 16)}
                 | set(MODEL_N))


def table_shapes():
    t = [(M, N, K) for _, M, N, K, _ in TILE_ALL]
    for d in (WORKSPACE_FORMS, RING8_MAIN, MID_ROWS_FORMS, TRAIN_EPI_FORMS):
        t += list(d)
    r = [(M, N, K) for _, N, K, _, ms in ROWS_CASES for M in ms] + list(ROWS_FORMS) + list(ROWS_STREAM_FORMS)
    return t, r


def sweep():
    """Shape lines for the planner main (and for a differential run against another revision's launchers)."""
    t_tab, r_tab = table_shapes()
    ms = sorted(set(SWEEP_M) | {M for M, _, _ in t_tab})
    ns = sorted(set(SWEEP_N) | {N for _, N, _ in t_tab + r_tab})
    shapes = [tile(M, N, K, ws, K + pad) for M in ms for N in ns for K in SWEEP_K for pad in (0, 8) for ws in SWEEP_WS]
    shapes += [tile(M, N, K, ws, K + pad) for M, N, K in t_tab for pad in (0, 8) for ws in SWEEP_WS]
    for M in sorted({m for m in ms if m <= 128} | {M for M, _, _ in r_tab}):
        for N, K in sorted({(N, K) for N in ns for K in SWEEP_K if K % 256 == 0} | {(N, K) for _, N, K in r_tab}):
            exact = [2 * M * N * 4, 4 * M * N * 4]
            for ws in SWEEP_WS + exact + [b - 1 for b in exact]:
                shapes += [rows(M, N, K, ws, stream, K + pad) for stream in (0, 1) for pad in (0, 8)]
    # TN: the case table, the ViT weight gradients (16 and 32 images of 261 / 256 tokens) and Llama's at 16 x 288 tokens
    tn_mn = {(M, N) for _, _, M, N, _ in TN_CASES} | {(1024, 1024), (3072, 1024), (4096, 1024), (1024, 4096), (1152, 1152), (3456, 1152),
                                                      (4304, 1152), (1152, 4304), (4096, 4096), (12288, 4096), (22016, 4096), (4096, 11008),
                                                      (32064, 4096)}
    for T in (33, 1000, 8200, 4096, 4176, 4608, 8352):
        shapes += [tn(T, M, N, ws, M + pad, N + 2 * pad) for M, N in sorted(tn_mn) for ws in SWEEP_WS for pad in (0, 8)]
    # e4m3: every M and N of the sweep (the plan depends on nothing else), K a multiple of 128 codes
    shapes += [fp8(M, N, 2 * K, ws) for M in ms for N in ns for K in SWEEP_K[::4] for ws in (-1, 64 * MIB)]
    shapes += [fp8(M, N, K, ws, K + 16) for M, N, K in FP8_SHAPES for ws in SWEEP_WS]
    return shapes


@pytest.fixture(scope="module")
def swept(planner):
    shapes = sweep()
    return shapes, planner(shapes)


def _problem(shape):
    """(M, N, K-tiles, workspace bytes) of a shape line."""
    if shape[0] == "tn":
        _, T, M, N, _, _, ws = shape
        return M, N, (T + 63) // 64, max(ws, 0)
    _, M, N, K, _, ws, _ = shape
    return M, N, K // 64, max(ws, 0)


def test_plan_invariants_over_the_sweep(swept):
    shapes, plans = swept
    assert len(shapes) > 100000
    for shape, (form, launches) in zip(shapes, plans):
        M, N, nk, ws = _problem(shape)
        what = f"{shape} {form}"
        assert 1 <= len(launches) <= 3, what
        for l in launches:
            assert 0 <= l["lds"] <= LDS_PER_CU, what
            assert l["grid_x"] > 0 and l["grid_y"] > 0 and l["block"] > 0 and l["block"] % 64 == 0 and l["block"] <= 1024, what
            # the persistent forms: only with an even K-tile count (the stage parity carries over from tile to tile)
            assert l["ptiles"] == 0 or (nk % 2 == 0 and l["family"] == KN_GEMM256S and l["ptiles"] > l["grid_x"] == 256), what
        # the slab: no more bytes than the workspace, none without one
        last = launches[-1]
        need = {KN_TILE_REDUCE: (last["grid_x"] // 32) * last["splitk"] * 256 * 256 * 4,
                KN_SLAB_REDUCE: last["splitk"] * M * N * 4, KN_TREE_REDUCE: last["splitk"] * M * N * 4}.get(last["family"], 0)
        assert need <= ws, f"{what}: needs {need} bytes of workspace"
        sliced = any(l["splitk"] > 1 for l in launches)
        assert sliced == (need > 0), f"{what}: K slices without a reduce, or a reduce without slices"
        # 256 x 256 tile forms: the main and tail launches cover every big tile once
        if launches[0]["family"] == KN_GEMM256S:
            covered = 0
            for l in launches:
                if l["family"] == KN_GEMM256S:
                    tiles = l["ptiles"] or l["grid_x"]
                    assert tiles % l["splitk"] == 0, what
                    assert l["tail_base"] == (covered if l["splitk"] > 1 else -1), what
                    covered += tiles // l["splitk"]
                elif l["family"] == KN_RING8:
                    per_tile = (256 // l["a"]) * (256 // l["b"])
                    assert l["grid_x"] % per_tile == 0 and l["tail_base"] == covered, what
                    covered += l["grid_x"] // per_tile
                else:
                    assert l["family"] == KN_TILE_REDUCE and l["grid_x"] == 32 * (covered - l["tail_base"]), what
            big = ((M + 255) // 256) * ((N + 255) // 256)
            assert covered == big and launches[0]["tiles_m"] * launches[0]["tiles_n"] == big, what
        # the e4m3 form: one launch, one workgroup per big tile, nothing else for any shape
        if shape[0] == "fp8":
            big = ((M + 255) // 256) * ((N + 255) // 256)
            (l,) = launches
            assert form == "gemm256s_fp8" and l["family"] == KN_GEMM256S_FP8 and l["grid_x"] == big == l["tiles_m"] * l["tiles_n"], what
            assert (l["grid_y"], l["block"], l["lds"], l["tail_base"], l["splitk"], l["ptiles"]) == (1, 512, 131072, -1, 1, 0), what
        else:
            assert all(l["family"] != KN_GEMM256S_FP8 for l in launches), what


def test_sweep_reaches_the_forms_that_have_a_per_element_case(swept):
    """Slice counts aside, the forms the tile, rows and TN planners produce over the sweep are the ones ALL_FORMS of
    tests/test_gemm_ref_gpu.py lists (each has a per-element case there): a form without one fails here, without a GPU.
    (The e4m3 planner's one form has its per-element cases in tests/test_fp8_ref_gpu.py.)"""
    norm = lambda f: re.sub(r"\+splitk\d+", "+splitk", re.sub(r"/S\d+", "/S", f))
    reached = {norm(form) for shape, (form, _) in zip(*swept) if shape[0] != "fp8"}
    listed = {norm(f) for f in ALL_FORMS if not f.startswith("skinny")}
    assert reached == listed, f"no per-element case: {sorted(reached - listed)}; listed but never planned: {sorted(listed - reached)}"
