// gemm_plan.h — which kernels a GEMM shape gets, bf16 or e4m3: plain host C++17, no HIP. Every threshold the project has measured (tile
// sizes, K slicing, tails, 288-row tiles, the persistent form) lives here, next to its measurement. A planner (one per entry
// point) turns a GemmShape into a GemmPlan: up to three launches (main, tail, reduce), each with kernel id, grid, block, dynamic
// LDS bytes and the GemmArgs scalars it sets, plus the form code bl_gemm_last_form reports. launch_plan (gemm_common.h for the
// tile, rows, TN and e4m3 families; gemm_skinny.hip) carries a plan out and decides nothing. tests/test_gemm_plan_cpu.py compiles this header alone.
#pragma once
#include <cstdint>

namespace blplan {

constexpr int BK = 64, ROW_BYTES = 128;   // bf16 elements per K-step = 128 B per activation-tile row
constexpr int CUS = 256;   // MI355X compute units: the 256-row tile kernels run one workgroup per CU, a round is CUS tiles

// ---- kernels: id = family | a, b, c (kid), the kernel's template parameters after EPI in their order; the launchers' lists map
// an id to its instantiation. KN_TILE_REDUCE gemm_splitk_reduce_kernel (the split-K tail's slabs), KN_SLAB_REDUCE
// gemm128_splitk_reduce_kernel (the K-sliced forms' [M, N] slabs), KN_ROWS_STREAM_HALVES gemm_rows_stream_kernel<BL_EPI_NONE, …>
// (K-halves to the slab), KN_SKINNY <KS = a, GS = b, EPI, NORM = c>, KN_GEMM256S_FP8 gemm256s_fp8_kernel (gemm_fp8.hip)
enum { KN_GEMM128 = 1, KN_RING8, KN_MID, KN_MID2, KN_GEMM288S, KN_GEMM256S, KN_TILE_REDUCE, KN_SLAB_REDUCE, KN_ROWS_STREAM,
       KN_ROWS_STREAM_HALVES, KN_TREE_REDUCE, KN_SKINNY, KN_GEMM256S_FP8 };
constexpr int kid(int family, int a = 0, int b = 0, int c = 0) { return family | (a << 8) | (b << 16) | (c << 24); }
constexpr int kid_family(int k) { return k & 0xFF; }      constexpr int kid_a(int k) { return (k >> 8) & 0xFF; }
constexpr int kid_b(int k) { return (k >> 16) & 0xFF; }   constexpr int kid_c(int k) { return (k >> 24) & 0xFF; }

// ---- dynamic LDS: one function per kernel family; hipFuncSetAttribute and the launch both take lds_bytes(kernel id) ----------
constexpr int lds_gemm128() { return 2 * 256 * ROW_BYTES; }
constexpr int lds_gemm256s() { return 2 * 65536; }
constexpr int lds_gemm288s() { return 2 * 73728; }
constexpr int lds_gemm256s_fp8() { return 2 * 65536; }
// gemm_ring8_kernel<EPI, BM, BN, 4>: four ring slots of BM activation + BN weight rows, and the 1-KiB dump
constexpr int lds_ring8(int bm, int bn) { return 4 * (bm + bn) * ROW_BYTES + 1024; }
constexpr int lds_mid(int mb, int nb) { return 3 * (64 * mb * ROW_BYTES + nb * 2048); }
// gemm_mid2_kernel<EPI, NT, NST>: NST ring stages of 160 activation rows + NT 4-KiB weight pieces
constexpr int lds_mid2(int nt, int nst) { return nst * (160 * ROW_BYTES + nt * 4096); }
constexpr int lds_rows_stream() { return 4 * 2 * 6 * 16 * ROW_BYTES; }   // gemm_rows_stream_kernel: NWB chunks of 96 rows × 2 K-tiles
constexpr int lds_bytes(int k) {
  switch (kid_family(k)) {
    case KN_GEMM128: return lds_gemm128();
    case KN_RING8: return lds_ring8(kid_a(k), kid_b(k));
    case KN_MID: return lds_mid(kid_a(k), kid_b(k));
    case KN_MID2: return lds_mid2(kid_a(k), kid_b(k));
    case KN_GEMM288S: return lds_gemm288s();
    case KN_GEMM256S: return lds_gemm256s();
    case KN_ROWS_STREAM: case KN_ROWS_STREAM_HALVES: return lds_rows_stream();
    case KN_GEMM256S_FP8: return lds_gemm256s_fp8();
    default: return 0;   // the reduce kernels use none, the skinny kernel's is static
  }
}

// ---- the skinny kernel's K table: K, KS = MFMA k-steps per wave (K = 8 · KS · 32), GS = k-steps per load group. The one copy:
// plan_skinny, the launcher's instantiations and bl_rmsnorm_skinny_bf16 all expand it.
#define BL_SKINNY_TABLE(X)                                                                                               \
  X(4096, 16, 8) X(11008, 43, 8)   /* Llama-2-7B hidden, MLP */   X(5120, 20, 5) X(13824, 54, 9)   /* Llama-2-13B */     \
  X(512, 2, 1) X(1024, 4, 2) X(1536, 6, 3)   /* reduced-width test / oracle configs */

// ---- plans ---------------------------------------------------------------------------------------------------------------
struct GemmShape {
  int M, N, K;
  int64_t lda, ldw, ws_bytes;   // ws_bytes: the caller's workspace (0 = none; K slicing is opt-in: sliced sums are not slot-invariant)
  bool rows_stream;             // the BL_ROWS_STREAM switch (rows form only)
};
// the GemmArgs scalars a launch sets; the defaults are fill_gemm_args'
struct GemmOverrides { int tiles_m = 0, tiles_n = 0, tail_base = -1, splitk = 1, ptiles = 0, fold_ks = 0; };
struct Launch : GemmOverrides { int kernel = 0, grid_x = 0, grid_y = 1, block = 0, lds = 0; };
struct GemmPlan {
  int form = 0, n = 0;   // form_code() of the n launches below; n = 0: the entry point has no kernel for the shape
  Launch l[3];
};

// The form code (bl_gemm_last_form, named by ops.gemm_form_name): it takes no part in any dispatch decision.
//   bits 0-7 main kernel (GF_*), 8-11 / 12-15 its two template parameters, 16-21 its K slices (or the skinny KS),
//   22-24 tail treatment (GT_*), 25-29 the split-K tail's slice count
enum {
  GF_GEMM128 = 1, GF_RING160 = 2, GF_RING128_KSLICED = 3, GF_MID = 4, GF_MID2 = 5, GF_GEMM288S = 6, GF_GEMM256S = 7,
  GF_GEMM256S_PERSISTENT = 8, GF_ROWS_STREAM = 10, GF_ROWS_MID = 11, GF_SKINNY = 12, GF_TN = 13, GF_TN_PERSISTENT = 14,
  GF_TN_ALL_SPLIT = 15, GF_GEMM256S_FP8 = 16
};
enum { GT_NONE = 0, GT_SUB64X64 = 1, GT_SUB128X64 = 2, GT_SUB128X128 = 3, GT_SPLITK = 4 };
constexpr int pack_form(int kind, int a = 0, int b = 0, int s = 0, int tail = GT_NONE, int tail_s = 0) {
  return kind | (a << 8) | (b << 12) | (s << 16) | (tail << 22) | (tail_s << 25);
}
// Read off the launches, so it cannot disagree with them.
inline int form_code(const GemmPlan& pl) {
  if (pl.n == 0) return 0;
  const Launch& m = pl.l[0];
  const int k = m.kernel;
  switch (kid_family(k)) {
    case KN_GEMM128: return pack_form(GF_GEMM128);
    case KN_RING8: return kid_a(k) == 160 ? pack_form(GF_RING160) : pack_form(GF_RING128_KSLICED, 0, 0, m.splitk);
    case KN_MID: return kid_c(k) ? pack_form(GF_ROWS_MID, 0, kid_c(k)) : pack_form(GF_MID, kid_a(k), kid_b(k), m.splitk);
    case KN_MID2: return pack_form(GF_MID2, kid_a(k), kid_b(k) == 3 ? 0 : kid_b(k));
    case KN_GEMM288S: return pack_form(GF_GEMM288S);
    case KN_ROWS_STREAM: case KN_ROWS_STREAM_HALVES: return pack_form(GF_ROWS_STREAM, kid_a(k), kid_b(k));
    case KN_SKINNY: return pack_form(GF_SKINNY, kid_c(k), 0, kid_a(k));
    case KN_GEMM256S_FP8: return pack_form(GF_GEMM256S_FP8);
    case KN_GEMM256S: break;
    default: return 0;
  }
  // the 256 × 256 tile forms: main launch, then sub-tiles on the ring kernel or K slices + their reduce
  const bool tn = kid_a(k) != 0, all_split = m.splitk > 1;   // all_split: no whole round, the first launch is the slices'
  const int main = m.ptiles > 0 ? (tn ? GF_TN_PERSISTENT : GF_GEMM256S_PERSISTENT)
                                : tn ? (all_split ? GF_TN_ALL_SPLIT : GF_TN) : GF_GEMM256S;
  const Launch& last = pl.l[pl.n - 1];
  if (kid_family(last.kernel) == KN_TILE_REDUCE) return pack_form(main, 0, 0, 0, GT_SPLITK, last.splitk);
  if (kid_family(last.kernel) == KN_RING8)
    return pack_form(main, 0, 0, 0, kid_a(last.kernel) == 64 ? GT_SUB64X64 : kid_b(last.kernel) == 64 ? GT_SUB128X64 : GT_SUB128X128);
  return pack_form(main);
}

namespace detail {
inline int imin(int a, int b) { return a < b ? a : b; }
inline void add(GemmPlan& pl, int kernel, int grid_x, int grid_y, int block, const GemmOverrides& p) {
  Launch& l = pl.l[pl.n++];
  static_cast<GemmOverrides&>(l) = p;
  l.kernel = kernel; l.grid_x = grid_x; l.grid_y = grid_y; l.block = block; l.lds = lds_bytes(kernel);
}
// the [M, N] slab reduces (gemm128_splitk_reduce_kernel, gemm_rows_tree_reduce_kernel): 4 columns per thread, grid capped
inline void add_slab_reduce(GemmPlan& pl, int kernel, const GemmShape& g, const GemmOverrides& p) {
  const int64_t work = (int64_t)g.M * (g.N / 4), blocks = (work + 255) / 256;
  add(pl, kernel, (int)(blocks < 2048 ? blocks : 2048), 1, 256, p);
}
// tiles on gemm256s_kernel: more than one round walks persistently (one workgroup per CU) where the plan allows it
inline void add256(GemmPlan& pl, bool tn, int tiles, bool persist, GemmOverrides p) {
  if (persist && tiles > CUS) p.ptiles = tiles;
  add(pl, kid(KN_GEMM256S, tn), p.ptiles ? CUS : tiles, 1, 512, p);
}
inline GemmPlan finish(GemmPlan& pl) {
  pl.form = form_code(pl);
  return pl;
}
}  // namespace detail

// bl_gemm_skinny_rows_bf16: M <= 128 rows in the skinny kernel's summation order — gemm_rows_stream_kernel for the wide
// layers at M <= 96 (qkv, gate/up, lm_head), gemm_mid_kernel<SK> otherwise
inline GemmPlan plan_rows(const GemmShape& g) {
  using namespace detail;
  GemmPlan pl;
  GemmOverrides p;
  const bool has_ws = g.ws_bytes > 0;
  p.fold_ks = g.K / 256;                       // 8 slices of K/8 columns = K/256 MFMA k-steps each
  // Rows-stream form: slices that end on its 4-k-step chunks (K a multiple of 1024), more than 256 weight tiles (the narrow
  // layers' two launches — K split + reduce — are launch-bound and the mid kernel's are shorter: o 16.7 vs 19.5 µs, down
  // 28.3 vs 33.5). 7B at 96 rows, same box: gate/up 53.5 → 40.2 µs (6 waves × 230 workgroups), qkv 38.1 → 32.7 (8 waves ×
  // 96 column groups × 2 K-halves + the tree's last level in the reduce kernel). BL_ROWS_STREAM=0 switches it off (A/B).
  const int n_tiles = g.N / 16;
  if (g.M <= 96 && p.fold_ks % 4 == 0 && n_tiles > 256 && g.rows_stream) {
    const bool can_split = has_ws && g.ws_bytes >= 2LL * g.M * g.N * 4;
    // grid: NWV 16-row weight tiles per workgroup, 8 / SK workgroups along K
    if ((n_tiles + 7) / 8 >= 200) {                       // one round of 8-wave workgroups fills the chip (lm_head)
      add(pl, kid(KN_ROWS_STREAM, 8, 8), (n_tiles + 7) / 8, 1, 8 * 64, p);
    } else if ((n_tiles + 5) / 6 >= 200 || !can_split) {  // 6-wave workgroups do (gate/up: 230)
      add(pl, kid(KN_ROWS_STREAM, 6, 8), (n_tiles + 5) / 6, 1, 6 * 64, p);
    } else {                                              // two K-halves of 4 slices each + the last tree level
      p.splitk = 2;
      add(pl, kid(KN_ROWS_STREAM_HALVES, 8, 4), (n_tiles + 7) / 8, 2, 8 * 64, p);
      add_slab_reduce(pl, kid(KN_TREE_REDUCE), g, p);
    }
    return finish(pl);
  }
  const int slabs64 = (g.N + 63) / 64;
  // 64-column slabs, every weight byte once, all rows of A staged once per workgroup. Where that leaves most CUs without
  // a workgroup (N = 4096: 64 slabs) and the caller gave a workspace, grid.y = 4 workgroups take two K-slices each and
  // the tree is finished by the reduce kernel — the split is exact (see gemm_mid_kernel) and the same for every row.
  const bool split = slabs64 * 2 <= 256 && has_ws && g.ws_bytes >= 4LL * g.M * g.N * 4;
  p.splitk = split ? 4 : 1;
  if (split) {
    add(pl, kid(KN_MID, 2, 4, 2), slabs64, 4, 256, p);
    add_slab_reduce(pl, kid(KN_TREE_REDUCE), g, p);
  } else {
    add(pl, kid(KN_MID, 2, 4, 8), slabs64, 1, 256, p);
  }
  return finish(pl);
}

// bl_gemm_bf16: the tile GEMM
inline GemmPlan plan_gemm(const GemmShape& g) {
  using namespace detail;
  GemmPlan pl;
  GemmOverrides p;
  const bool has_ws = g.ws_bytes > 0;
  const int bm = (g.M + 255) / 256, bn = (g.N + 255) / 256, big_tiles = bm * bn;
  // one (partial) round of big tiles beats 1.5+ rounds of the 128 kernel once about half of the CUs get a tile (ViT qkv at
  // B = 16: 204 / 224 tiles, 45 → 39 µs; round 3, the narrow ViT layers at the training batch of 32 images — 132 / 160 tiles
  // for M = 8352 / 8192, N = 1024 / 1152 — where the 128 kernel needs 528 / 576 > 512 workgroup slots: 104 → 82 µs at
  // K = 4096, 35 → 30 µs at K = 1024)
  const bool big = big_tiles >= 128 && g.K >= 512;
  // M <= 320: the weight-streaming mid kernels; up to 640 rows (B = 2 prefill) the 160-row mid2 kernel still beats the
  // tile kernels (38.2 -> 36.4 ms per batch), beyond that it loses (B = 4: 42.7 vs 48.2 ms)
  const bool mid2_only = g.M > 320;
  if (g.M <= 640 && g.M > 32 && g.K >= 512 && !(mid2_only && (has_ws || (g.N % 32)))) {
    // every weight byte once: one workgroup per column slab, all rows; 64-column slabs when that already gives ≥ 160
    // workgroups, else 16-column slabs. grid.y slices K only with a workspace (opt-in).
    const int slabs64 = (g.N + 63) / 64, nkm = g.K / BK;
    bool wide = slabs64 >= 160;   // measured: 64-column slabs for N = 4096 without K slicing (64 workgroups) cost +2.2 ms at B = 1
    int S = 1;
    if (!wide && has_ws && slabs64 * 2 <= CUS) {
      // Every workgroup re-reads ALL M rows of A from L2, so the L2 traffic is (N / slab width) · M · K · 2 B: with a
      // workspace, narrow layers (N = 4096: 64 slabs of 64 columns) keep the 64-column slabs — a quarter of the activation
      // traffic of 16-column slabs — and fill the chip by slicing K instead (same slicing for every row: slot-invariant)
      int S2 = imin(8, CUS / slabs64);
      while (S2 > 1 && (nkm / S2 < 8 || g.ws_bytes < (int64_t)S2 * g.M * g.N * 4)) --S2;
      if (S2 > 1) { wide = true; S = S2; }
    }
    if (S == 1 && g.M > 128 && (g.N % 32) == 0) {
      // 160-row workgroups (gemm_mid2_kernel): narrow layers 32 columns (3-stage ring, 2 workgroups per CU); wide layers
      // 64 columns on a 2-stage ring so that two workgroups share a CU and one's LDS-DMA issue runs under the other's
      // MFMAs (qkv 59 -> 44 us, gate/up 112 -> 83 us at M = 288); the widest (lm_head) 128 columns.
      const int mb = (g.M + 159) / 160;
      if (!wide) add(pl, kid(KN_MID2, 1, 3), g.N / 32, mb, 256, p);
      else if (slabs64 >= 400) add(pl, kid(KN_MID2, 4, 3), (g.N + 127) / 128, mb, 256, p);
      else add(pl, kid(KN_MID2, 2, 2), (g.N + 63) / 64, mb, 256, p);
      return finish(pl);
    }
    const int slabs = wide ? slabs64 : (g.N + 15) / 16;
    if (S == 1 && !wide && has_ws && slabs < CUS) {
      S = imin(8, (CUS + CUS / 2 + slabs - 1) / slabs);
      while (S > 1 && (nkm / S < 8 || g.ws_bytes < (int64_t)S * g.M * g.N * 4)) --S;
    }
    p.splitk = S;
    // gemm_mid_kernel for M ≤ 64·MB rows: 64-column slabs (wide) or 16-column slabs
    add(pl, kid(KN_MID, g.M <= 128 ? 2 : g.M <= 256 ? 4 : 5, wide ? 4 : 1), slabs, S, 256, p);
    // K-sliced forms: slices write fp32 partials [M, N] to the slab, gemm128_splitk_reduce_kernel sums them in slice order
    // and applies the epilogue
    if (S > 1) add_slab_reduce(pl, kid(KN_SLAB_REDUCE), g, p);
    return finish(pl);
  }
  if (!big && g.K >= 512) {
    // one round of 160 × 128 tiles on the ring-buffered kernel when that covers the problem with ≥ 3/4 of the CUs busy
    const int t160 = ((g.M + 159) / 160) * ((g.N + 127) / 128);
    if (t160 <= CUS && t160 >= (3 * CUS) / 4) {
      p.tiles_m = (g.M + 159) / 160, p.tiles_n = (g.N + 127) / 128;
      add(pl, kid(KN_RING8, 160, 128), t160, 1, 512, p);
      return finish(pl);
    }
  }
  if (!big) {
    p.tiles_m = (g.M + 127) / 128, p.tiles_n = (g.N + 127) / 128;
    const int tiles = p.tiles_m * p.tiles_n, nk128 = g.K / BK;
    // few tiles, long K (tall-skinny): slice K over grid.y on the ring kernel (one workgroup per CU: 129 KiB of LDS) when
    // the caller gave a workspace (opt-in, as for the 256 kernel: sliced sums are not batch-slot invariant)
    int S128 = 1;
    if (has_ws && tiles <= CUS / 2) {
      S128 = imin(8, CUS / tiles);
      while (S128 > 1 && (nk128 / S128 < 8 || g.ws_bytes < (int64_t)S128 * g.M * g.N * 4)) --S128;
    }
    if (S128 > 1) {
      p.splitk = S128;
      add(pl, kid(KN_RING8, 128, 128), tiles, S128, 512, p);
      add_slab_reduce(pl, kid(KN_SLAB_REDUCE), g, p);
    } else {
      add(pl, kid(KN_GEMM128), tiles, 1, 256, p);
    }
    return finish(pl);
  }
  // 288-row tiles (one 288-token sequence per row tile) where they remove the leftover round: estimated cost in units of
  // one round of 256 × 256 tiles — 256-row tiling: full rounds + 0.45 for a ≤ 64-tile tail on sub-tiles, 1 for a larger
  // partial round; 288-row tiling: rounds × 1.12 (12.5 % more MFMA work and 6 % more staging per tile).
  if ((g.K % 128) == 0) {
    const int t256 = big_tiles, r256 = t256 % CUS;
    const float cost256 = (float)(t256 / CUS) + (r256 == 0 ? 0.f : (r256 <= 64 && t256 > CUS) ? 0.45f : 1.0f);
    const int bm288 = (g.M + 287) / 288, t288 = bm288 * bn;
    const float cost288 = 1.12f * (float)((t288 + CUS - 1) / CUS);
    if (cost288 < 0.97f * cost256) {
      p.tiles_m = bm288, p.tiles_n = bn;
      add(pl, kid(KN_GEMM288S), t288, 1, 512, p);
      return finish(pl);
    }
  }
  // Whole rounds of 256 tiles on the pipelined kernel; a partial last round would leave most CUs idle for a full tile
  // time, so its tiles are cut into sub-tiles and run by the ring kernel instead.
  p.tiles_m = bm, p.tiles_n = bn;
  // The last round of 256-tile launches is usually partial (e.g. 288 tiles = 1.125 rounds). Measured cost of the
  // leftover `tail` tiles in units of one full round T(K) (tools/bench_gemm.py, profiles/): plain partial round 1.0;
  // 128x128 quarters on the small kernel ≈ 0.65 when they fit one small round (tail ≤ 64 … 128), > 1 beyond; split-K
  // over S = 256/tail slices ≈ 1/S + 45 µs of fp32 slab traffic, i.e. ≈ 0.28 at K = 11008 but ≈ 0.7 at K = 4096.
  int main_tiles = big_tiles, tail = big_tiles % CUS;
  const int nk = g.K / BK;
  int S = tail ? CUS / tail : 1;
  if (S > 16) S = 16;
  while (S > 1 && nk / S < 4) --S;
  // more than one round of tiles: the persistent form (one workgroup per CU walks its tiles, the next tile's first K-tiles
  // land behind this tile's epilogue); needs an even number of K-tiles (stage parity carries over) and 32-bit extents
  const bool persist_ok = (nk % 2) == 0 && (int64_t)g.M * g.lda * 2 < (1LL << 32) && (int64_t)g.N * g.K * 2 < (1LL << 32);
  const bool can_split = tail && S >= 2 && g.K >= 8192 && has_ws && g.ws_bytes >= (int64_t)tail * S * 256 * 256 * 4;
  if (can_split) {
    main_tiles = big_tiles - tail;
    if (main_tiles) add256(pl, false, main_tiles, persist_ok, p);
    p.tail_base = main_tiles;
    p.splitk = S;
    add256(pl, false, tail * S, false, p);
    add(pl, kid(KN_TILE_REDUCE), tail * 32, 1, 512, p);
  } else {
    // (65 … 128 leftover tiles — Llama qkv at B = 16: 96 — as 256 × 128 half tiles instead of a quarter-filled fourth round
    // was measured at −0.6 % end to end: the half tiles stage 3/4 of a full tile's bytes for half its FLOPs)
    if (tail != 0 && tail <= 64 && main_tiles > tail) main_tiles = big_tiles - tail; else tail = 0;
    add256(pl, false, main_tiles, persist_ok, p);
    if (tail) {
      // leftover 256x256 tiles on gemm_ring8_kernel's tail mode, cut so that the sub-tiles cover (up to) every CU once
      p.tail_base = main_tiles;
      if (tail <= 16) add(pl, kid(KN_RING8, 64, 64), tail * 16, 1, 512, p);
      else if (tail <= 32) add(pl, kid(KN_RING8, 128, 64), tail * 8, 1, 512, p);
      else add(pl, kid(KN_RING8, 128, 128), tail * 4, 1, 512, p);
    }
  }
  return finish(pl);
}

// bl_gemm_tn_bf16: C[M, N] (fp32) = Aᵀ·B over K token rows, A = [K, M] and B = [K, N] row-major — the weight gradient
// dW = dyᵀ·x straight from the row-major gradient and activation buffers (no transposed copies). Whole rounds of 256 × 256
// tiles on the staggered kernel's TN form; a partial last round is split along K when the caller gave a workspace.
inline GemmPlan plan_gemm_tn(const GemmShape& g) {
  using namespace detail;
  GemmPlan pl;
  GemmOverrides p;
  p.tiles_m = (g.M + 255) / 256, p.tiles_n = (g.N + 255) / 256;
  const int tiles = p.tiles_m * p.tiles_n, nk = (g.K + BK - 1) / BK;
  // fewer tiles than half the CUs (ViT blocks: 16 … 85 tiles): every tile is K-split so the launch fills the chip
  int tail = tiles > CUS ? tiles % CUS : (2 * tiles <= CUS ? tiles : 0);
  int S = tail ? CUS / tail : 1;
  if (tiles <= CUS && S > 8) S = 8;
  if (S > 16) S = 16;
  while (S > 1 && nk / S < 4) --S;
  const bool can_split = tail && S >= 2 && (nk >= 128 || tiles <= CUS) && g.ws_bytes > 0 &&
                         g.ws_bytes >= (int64_t)tail * S * 256 * 256 * 4;
  const bool persist_ok = (nk % 2) == 0 && ((int64_t)(g.K - 1) * g.lda + g.M) * 2 < (1LL << 32) &&
                          ((int64_t)(g.K - 1) * g.ldw + g.N) * 2 < (1LL << 32);
  if (can_split) {
    if (tiles > tail) add256(pl, true, tiles - tail, persist_ok, p);
    p.tail_base = tiles - tail;
    p.splitk = S;
    add256(pl, true, tail * S, false, p);
    add(pl, kid(KN_TILE_REDUCE, 1), tail * 32, 1, 512, p);
  } else {
    add256(pl, true, tiles, persist_ok, p);
  }
  return finish(pl);
}

// bl_gemm_fp8 (g.K and g.lda in 2-byte units, as the kernel counts them): ONE launch of gemm256s_fp8_kernel for every shape,
// a 256 × 256 tile per workgroup — no tail treatment, no K slices (a workspace changes nothing), no persistent
// walk, no 288-row tiles: none of them has been measured for e4m3.
inline GemmPlan plan_gemm_fp8(const GemmShape& g) {
  GemmPlan pl;
  GemmOverrides p;
  p.tiles_m = (g.M + 255) / 256, p.tiles_n = (g.N + 255) / 256;
  detail::add(pl, kid(KN_GEMM256S_FP8), p.tiles_m * p.tiles_n, 1, 512, p);
  return detail::finish(pl);
}

// K → the skinny kernel's KS and GS (BL_SKINNY_TABLE); false = no instantiation for this K
inline bool skinny_ks(int K, int& ks, int& gs) {
  switch (K) {
#define BL_ROW(K_, KS_, GS_) case K_: ks = KS_; gs = GS_; return true;
    BL_SKINNY_TABLE(BL_ROW)
#undef BL_ROW
    default: return false;
  }
}

// bl_gemm_skinny_bf16 (M <= 16); no launch = no instantiation for this K, the caller falls back to bl_gemm_bf16
inline GemmPlan plan_skinny(const GemmShape& g, bool norm) {
  GemmPlan pl;
  int ks, gs;
  if (!skinny_ks(g.K, ks, gs)) return pl;
  const int n_tiles = g.N / 16;
  // One 8-wave workgroup per CU: every variant needs > 128 VGPRs (x fragments 4·KS, two weight buffers, the fused-norm
  // weights: 148–254), so two workgroups never co-reside; a grid of 384 (768 tiles ÷ 2) ran as 1.5 rounds of 256.
  // Balanced tiles per workgroup on 256 slots: 768 tiles → 256 × 3; 1376 → 230 × 6 (not 256 × 5 + 96 stragglers).
  const int tpw = (n_tiles + 255) / 256;
  const int grid = (n_tiles + tpw - 1) / tpw;
  detail::add(pl, kid(KN_SKINNY, ks, gs, norm ? 1 : 0), grid, 1, 8 * 64, GemmOverrides{});
  return detail::finish(pl);
}

}  // namespace blplan
