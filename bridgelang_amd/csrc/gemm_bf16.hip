// gemm_bf16.hip — bf16 NT GEMM on gfx950 MFMA with fused epilogues:  C[M,N] = epi(A[M,K] · W[N,K]^T)
//
// Design (MI355X-first):
//   * activations A[M,K] are row-major; weights are fragment-major (bl_pack_weight_bf16: one contiguous KiB per
//     16-row × 32-k MFMA operand). Tiles are staged HBM→LDS with LDS-DMA (`buffer_load_dwordx4 … lds`, 1 KiB per
//     wave-instruction). The buffer descriptor's bounds check zero-fills rows past M / weight tiles past N, so ragged M
//     (e.g. 16·261) needs no host padding.
//   * LDS-DMA writes lane-linear. Weight blocks therefore land already in ds_read_b128 order (address = block + 16·lane:
//     conflict-free, no swizzle). Activation rows (128 B per row per K-step) get the bank-conflict swizzle on the
//     per-lane SOURCE address (chunk c of row r is fetched from chunk c ^ (r & 7)) and undone on the read side.
//   * MFMA is v_mfma_f32_16x16x32_bf16 computed TRANSPOSED: the weight tile is the "A" operand and the activation
//     tile the "B" operand, so a lane ends up holding 4 consecutive output columns n of one row m → 8-byte stores
//     and vector loads of bias / LayerScale / residual in the epilogue.
//   * 1-D grid remapped so that each XCD (private L2) receives a contiguous run of tiles, walked in groups of
//     GROUP_M row-tiles so concurrently resident tiles share weight panels.
//
// Kernels (plan_gemm in gemm_plan.h picks per shape):
//   gemm256s_kernel   — 256×256×64 tile, 8 waves in two staggered groups, 1 workgroup/CU; whole rounds of big problems.
//   gemm288s_kernel   — the same on 288-row tiles (one 288-token sequence per row tile) where they remove a leftover round.
//   gemm_ring8_kernel — 4-stage LDS-DMA ring, 8 waves: the sub-tiles of a leftover round, one round of 160×128 tiles for
//                       narrow layers, K-sliced few-tile problems.
//   gemm128_kernel    — 128×128×64 tile, 4 waves, 2 workgroups/CU: the remaining small problems.
//   gemm_mid_kernel / gemm_mid2_kernel — weight streaming for M ≤ 640 rows.
#include "gemm_common.h"
#include <stdlib.h>

namespace bl_gemm_bf16_impl {
using namespace blgemm;

typedef __attribute__((ext_vector_type(4))) short s16x4_t;   // result of ds_read_b64_tr_b16

// ======================================================================================================================
// 128 × 128 tile
// ======================================================================================================================
template <int EPI>
__global__ __launch_bounds__(256) void gemm128_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)   // __amdgpu_buffer_rsrc_t does not exist in the host pass; an ill-formed host body
                                      // silently drops the kernel's host handle (undefined symbol at dlopen)
  constexpr int BM = 128, BN = 128, WN = 2, NWAVE = 4;
  constexpr int TM = 64, TN = 64, MT = 4, NT = 4;
  constexpr int A_BYTES = BM * ROW_BYTES, BUF_BYTES = A_BYTES + BN * ROW_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 × BUF_BYTES

  int tm, tn;
  tile_coords(p, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int kt32 = p.K >> 5;

  const unsigned a_bytes = (unsigned)min((long)p.M * p.lda * 2, 0xffffffffL);
  const unsigned w_bytes = (unsigned)min((long)p.N * p.K * 2, 0xffffffffL);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, w_bytes, 0x00020000);

  // activation pieces: 16 × (8 rows × 128 B); wave takes pieces j*4 + wave. lane → (row = lane>>3, chunk = lane&7)
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffA[4], voffW[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) voffA[j] = (unsigned)(((long)(m0 + (j * NWAVE + wave) * 8 + prow) * p.lda) * 2 + pchunk * 16);
  // weight blocks: 8 n-tiles × 2 k-steps; wave takes n-tiles 2*wave, 2*wave+1 (both k-steps: 2 KiB contiguous each)
#pragma unroll
  for (int j = 0; j < 4; ++j)
    voffW[j] = (unsigned)(((long)(n0 / 16 + 2 * wave + (j >> 1)) * kt32 + (j & 1)) * 1024 + lane * 16);

#define BL_STAGE(BUF, KT)                                                                                   \
  do {                                                                                                      \
    char* base__ = smem + (BUF) * BUF_BYTES;                                                                \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) BL_GLDS(rsA, base__ + (j * NWAVE + wave) * 1024, voffA[j], (KT) * 128); \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                           \
        BL_GLDS(rsW, base__ + A_BYTES + ((2 * wave + (j >> 1)) * 2 + (j & 1)) * 1024, voffW[j], (KT) * 2048); \
  } while (0)

  const int l15 = lane & 15, lg = lane >> 4;
  const int c0 = lg ^ (lane & 7);
  const int offA = (wm * TM + l15) * ROW_BYTES;
  const int offW = A_BYTES + (wn * 4) * 2048 + lane * 16;   // block (wn*4 + i)*2 + ks

  f32x4_t acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  BL_STAGE(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) BL_STAGE(cur ^ 1, kt + 1);
    const char* base = smem + cur * BUF_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cb = (c0 ^ (ks * 4)) << 4;
      bf16x8_t wf[NT], af[MT];
#pragma unroll
      for (int i = 0; i < NT; ++i) wf[i] = *(const bf16x8_t*)(base + offW + i * 2048 + ks * 1024);
#pragma unroll
      for (int j = 0; j < MT; ++j) af[j] = *(const bf16x8_t*)(base + offA + j * 16 * ROW_BYTES + cb);
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], af[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#undef BL_STAGE
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j)
      epilogue_store4<EPI>(p, m0 + wm * TM + j * 16 + l15, n0 + wn * TN + i * 16 + lg * 4, acc[i][j]);
#endif
}

// ======================================================================================================================
// ring kernel: BM × BN tiles, NST-stage LDS-DMA ring behind a counted vmcnt, ONE barrier per K-step, 8 waves (two per SIMD)
// — 2 along m × 4 along n. Three uses, all with at most one workgroup per CU, where nothing else hides the HBM/L2 latency
// (a two-stage loop spent ≈ 3/4 of every K-step waiting there):
//   * tail mode (p.tail_base >= 0): 128×128, 128×64 or 64×64 sub-tiles of the big kernel's leftover 256×256 tiles;
//   * one round of 160 × 128 tiles for the narrow ViT layers at 16 images (attn.proj / mlp.fc2 / patch embed: M = 4176 or
//     4096, N = 1024 or 1152: 216 / 234 tiles; 160 divides the ragged M with 1.5–3.4 % waste where 128-row tiles need
//     264 / 288 > 256 workgroups);
//   * K-sliced (grid.y > 1): few-tile, long-K problems, partial sums to the slab.
// Two waves per SIMD (round 4, replacing a one-wave-per-SIMD form): with one wave per SIMD the wave that issues
// a ring slot's LDS-DMA pieces (≈ 60 issue cycles per 1-KiB piece) is the only one that could issue MFMAs there, so a
// K-step took pieces + fragment reads + MFMAs back to back (ISA: 9 pieces, 18 ds_read_b128, lgkmcnt(0), 40 MFMAs: ≈ 0.82 µs
// for 640 cycles of matrix work). Here every wave carries half the MFMAs and
// half the pieces of its SIMD, the pieces are spread through the wave's MFMAs (sched_barrier-pinned groups), and the
// partner wave's MFMAs issue while this wave sits in a piece's issue. The 20 activation pieces do not divide by 8 waves:
// waves 4–7 issue a third, out-of-range piece (zero-fill, no memory request) into a dump KiB behind the ring, which keeps
// the loop branch-free and the counted vmcnt the same for every wave. K order per output = every other tile kernel's.
// ======================================================================================================================
template <int EPI, int BM, int BN, int NST>
__global__ __launch_bounds__(512) void gemm_ring8_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NWAVE = 8, TM = BM / 2, TN = BN / 4, MT = TM / 16, NT = TN / 16;      // waves: 2 along m x 4 along n
  constexpr int APIECES = BM / 8, WPIECES = BN / 8;
  constexpr int APW = (APIECES + NWAVE - 1) / NWAVE, WPW = WPIECES / NWAVE, LPS = APW + WPW;
  static_assert(TM % 16 == 0 && TN % 16 == 0 && WPIECES % NWAVE == 0, "tile shape");
  constexpr int A_BYTES = BM * ROW_BYTES, BUF_BYTES = A_BYTES + BN * ROW_BYTES, DUMP = NST * BUF_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NST × BUF_BYTES + 1 KiB dump

  // workgroups go to XCDs round-robin: give each XCD (private L2) a contiguous run of tiles. In tail mode that is a run of
  // WHOLE leftover tiles — with the plain order the SUBS pieces of a tile land on SUBS different L2s and every one of them
  // fetches the same rows; otherwise the column tiles of a row panel are neighbours in `lin`, so an XCD's run re-uses its
  // activation panels from L2.
  const int nwg = gridDim.x, xcd = blockIdx.x & 7, q = nwg >> 3, r = nwg & 7;
  const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
  int m0, n0;
  if (p.tail_base >= 0) {   // tail mode: SUBS sub-tiles per leftover 256 × 256 tile, row-major within the tile
    constexpr int SUB_N = 256 / BN, SUBS = (256 / BM) * SUB_N;
    int tm, tn;
    lin_to_tile(p, p.tail_base + lin / SUBS, tm, tn);
    const int sub = lin % SUBS;
    m0 = tm * 256 + (sub / SUB_N) * BM, n0 = tn * 256 + (sub % SUB_N) * BN;
  } else {
    m0 = (lin / p.tiles_n) * BM, n0 = (lin % p.tiles_n) * BN;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int kt32 = p.K >> 5;

  const unsigned a_bytes = (unsigned)min((long)p.M * p.lda * 2, 0xffffffffL);
  const unsigned w_bytes = (unsigned)min((long)p.N * p.K * 2, 0xffffffffL);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, w_bytes, 0x00020000);

  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffA[APW], voffW[WPW];
  int ldsA[APW];                       // slot-relative LDS byte offset of this wave's j-th activation piece (wave-uniform)
#pragma unroll
  for (int j = 0; j < APW; ++j) {
    const int pi = j * NWAVE + wave;
    const bool real = pi < APIECES;
    voffA[j] = real ? (unsigned)(((long)(m0 + pi * 8 + prow) * p.lda) * 2 + pchunk * 16) : 0xfffffff0u;
    ldsA[j] = real ? pi * 1024 : -1;
  }
#pragma unroll
  for (int j = 0; j < WPW; ++j) {   // weight block b = j*NWAVE + wave: n-tile b >> 1, k-step b & 1
    const int blk = j * NWAVE + wave;
    voffW[j] = (unsigned)(((long)(n0 / 16 + (blk >> 1)) * kt32 + (blk & 1)) * 1024 + lane * 16);
  }
  // piece `pc` (0 … LPS-1) of this wave for K-tile KT into ring slot BUF
#define BL_PIECE(BUF, KT, PC)                                                                                     \
  do {                                                                                                            \
    char* base__ = smem + (BUF) * BUF_BYTES;                                                                      \
    if ((PC) < APW) {                                                                                             \
      const int ja__ = (PC) < APW ? (PC) : 0;                                                                     \
      BL_GLDS(rsA, ldsA[ja__] >= 0 ? base__ + ldsA[ja__] : smem + DUMP, voffA[ja__], (KT) * 128);                 \
    } else {                                                                                                      \
      const int jw__ = (PC) >= APW ? (PC) - APW : 0;                                                              \
      BL_GLDS(rsW, base__ + A_BYTES + (jw__ * NWAVE + wave) * 1024, voffW[jw__], (KT) * 2048);                    \
    }                                                                                                             \
  } while (0)

  const int l15 = lane & 15, lg = lane >> 4;
  const int c0 = lg ^ (lane & 7);
  const int offA = (wm * TM + l15) * ROW_BYTES;
  const int offW = A_BYTES + (wn * NT) * 2048 + lane * 16;   // block (wn*NT + i)*2 + ks

  f32x4_t acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // grid.y > 1 slices K (few-tile, long-K problems — LoRA's rank projections t = x·Aᵀ / dt = dy·(sB): 37 row tiles, N = 64 … 192,
  // K up to 22016 — which gemm128's one-stage prefetch ran at one global-load latency per K-step, ≈ 19.5 µs per call): every
  // slice writes its fp32 partial [M, N] to the slab, gemm128_splitk_reduce_kernel sums them in slice order + epilogue
  const int nk_all = p.K / BK;
  int ktb = 0, nk = nk_all;
  const bool sliced = p.splitk > 1 && p.tail_base < 0;
  if (sliced) {
    ktb = (int)(((long)blockIdx.y * nk_all) / p.splitk);
    nk = (int)(((long)(blockIdx.y + 1) * nk_all) / p.splitk) - ktb;
  }
#pragma unroll
  for (int s2 = 0; s2 < NST - 1; ++s2) {
    const int kt0 = ktb + min(s2, nk - 1);
#pragma unroll
    for (int pc = 0; pc < LPS; ++pc) BL_PIECE(s2, kt0, pc);
  }
  static_assert((NST - 2) * LPS <= 63 && NST >= 4, "counted vmcnt range / ring depth");
  constexpr int NMF = 2 * NT * MT, EVERY = NMF / LPS;          // one piece every EVERY MFMAs
  constexpr int NRD = 2 * (NT + MT), RPG = (NRD + LPS - 1) / LPS;   // fragment reads per K-tile, per group
  static_assert(EVERY >= 1, "more DMA pieces than MFMAs");
  // Two fragment register sets: the reads of K-tile kt+1 are issued among the MFMAs of K-tile kt (after the barrier that
  // says kt+1 has landed), so no wave ever waits on LDS at the head of a K-step — with one set all eight waves read their
  // 14 fragments right behind the barrier (≈ 450 LDS cycles per CU with no MFMA in flight: 0.58 µs per K-step measured).
  // The loop is unrolled by two K-steps for the set swap; an odd last K-step follows the loop.
  bf16x8_t wf[2][2][NT], af[2][2][MT];
#define BL_READ(SET, BASE, RI)                                                                                   \
  do {                                                                                                           \
    const int ks__ = (RI) / (NT + MT), e__ = (RI) % (NT + MT);                                                   \
    if (e__ < NT) wf[SET][ks__][e__ < NT ? e__ : 0] = *(const bf16x8_t*)((BASE) + offW + e__ * 2048 + ks__ * 1024);   \
    else af[SET][ks__][e__ >= NT ? e__ - NT : 0] =                                                               \
        *(const bf16x8_t*)((BASE) + offA + (e__ - NT) * 16 * ROW_BYTES + ((c0 ^ (ks__ * 4)) << 4));              \
  } while (0)
#define BL_KSTEP(CUR, NXT, KT)                                                                                   \
  do {                                                                                                           \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 3) * LPS) : "memory");   /* K-tile KT+1 landed (my pieces) */ \
    __builtin_amdgcn_s_barrier();   /* … for every wave; every wave has its fragments of K-tile KT-1 and older */ \
    const char* nb__ = smem + (((KT) + 1) % NST) * BUF_BYTES;                                                    \
    const int nslot__ = ((KT) + NST - 1) % NST;                      /* the slot of K-tile KT-1 */               \
    const int nkt__ = ktb + min((KT) + NST - 1, nk - 1);                                                         \
    _Pragma("unroll") for (int g = 0; g < LPS; ++g) {                                                            \
      BL_PIECE(nslot__, nkt__, g);                                                                               \
      _Pragma("unroll") for (int ri = g * RPG; ri < ((g + 1) * RPG < NRD ? (g + 1) * RPG : NRD); ++ri)           \
          BL_READ(NXT, nb__, ri);                                                                                \
      __builtin_amdgcn_sched_barrier(0);                                                                         \
      _Pragma("unroll") for (int idx = g * EVERY; idx < ((g + 1 < LPS) ? (g + 1) * EVERY : NMF); ++idx) {        \
        const int ks = idx / (NT * MT), i = (idx / MT) % NT, j = idx % MT;                                       \
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[CUR][ks][i], af[CUR][ks][j], acc[i][j], 0, 0, 0); \
      }                                                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                                         \
    }                                                                                                            \
  } while (0)
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPS) : "memory");   // K-tile 0 landed (this wave's pieces)
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ri = 0; ri < NRD; ++ri) BL_READ(0, smem, ri);
  for (int kt = 0; kt + 1 < nk; kt += 2) {
    BL_KSTEP(0, 1, kt);
    BL_KSTEP(1, 0, kt + 1);
  }
  if (nk & 1) BL_KSTEP(0, 1, nk - 1);    // odd K-tile count (LoRA's K + rank columns): one more step from set 0, outside the loop
#undef BL_KSTEP
#undef BL_READ
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the surplus stages must not outlive the workgroup's LDS allocation
#undef BL_PIECE
  if (sliced) {
    float* slab = p.slab + (long)blockIdx.y * p.M * p.N;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const int m = m0 + wm * TM + j * 16 + l15, n = n0 + wn * TN + i * 16 + lg * 4;
        if (m < p.M && n < p.N) *(f32x4_t*)(slab + (long)m * p.N + n) = acc[i][j];
      }
    return;
  }
  int ncol[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) ncol[i] = n0 + wn * TN + i * 16 + lg * 4;
  epilogue_tile<EPI, NT, MT>(p, m0 + wm * TM + l15, ncol, m0 + BM, n0 + BN, acc);
#endif
}

// out(m, n..n+3) = epilogue(Σ_slices slab[slice][m][n..n+3]): the K-sliced forms of gemm_ring8_kernel and gemm_mid_kernel
template <int EPI>
__global__ __launch_bounds__(256) void gemm128_splitk_reduce_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int n4 = p.N >> 2;
  const long total = (long)p.M * n4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int m = (int)(i / n4), n = (int)(i - (long)m * n4) * 4;
    f32x4_t sum = *(const f32x4_t*)(p.slab + (long)m * p.N + n);
    for (int s2 = 1; s2 < p.splitk; ++s2) sum += *(const f32x4_t*)(p.slab + ((long)s2 * p.M + m) * p.N + n);
    epilogue_store4<EPI>(p, m, n, sum);
  }
#endif
}

// out(m, n..n+3) = epilogue(tree of the S = 2 / 4 / 8 slab partials) for gemm_mid_kernel<SK>: the upper levels of the
// skinny order's balanced binary tree (each partial is already the tree value of an aligned group of 8/S slices)
template <int EPI>
__global__ __launch_bounds__(256) void gemm_rows_tree_reduce_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int n4 = p.N >> 2, S = p.splitk;
  const long total = (long)p.M * n4, stride = (long)p.M * p.N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int m = (int)(i / n4), n = (int)(i - (long)m * n4) * 4;
    const float* q = p.slab + (long)m * p.N + n;
    f32x4_t v[8];
    for (int s2 = 0; s2 < S; ++s2) v[s2] = *(const f32x4_t*)(q + s2 * stride);
    for (int w = 1; w < S; w *= 2)
      for (int s2 = 0; s2 < S; s2 += 2 * w) v[s2] = v[s2] + v[s2 + w];
    epilogue_store4<EPI>(p, m, n, v[0]);
  }
#endif
}

// ======================================================================================================================
// "mid" kernel: ALL M ≤ 64·MB rows × (16·NB) columns per workgroup (batch-1 prefill S = 288, one image's ViT tokens, the
// projector at one image): every weight byte leaves HBM exactly once per GEMM — these shapes are bound by the weight
// stream, not by MFMA — while the activation K-slabs (M × 128 B per K-step) are re-read from L2 by every workgroup.
// 4 waves, wave w owns rows [16·MB·w, 16·MB·(w+1)) × all NB column blocks; 3-stage LDS ring (≤ 144 KiB), two K-tiles of
// LDS-DMA in flight behind a counted vmcnt. NB = 4 (64-column slabs) for wide layers; NB = 1 (16-column slabs) when 64
// would leave most CUs without a workgroup (N = 4096 → 256 workgroups instead of 64). The K order of every output is the
// tile kernels' (K-tile by K-tile, two 32-steps each), so results are bit-identical to theirs — a sequence's result does
// not depend on the batch size it was run in. grid.y may slice K when the caller provides a workspace (opt-in).
// ======================================================================================================================
//
// SK > 0 ("skinny order", bl_gemm_skinny_rows_bf16): the fp32 summation order of gemm_skinny_kernel instead of the tile
// kernels' — K is cut into 8 slices of p.fold_ks MFMA k-steps; each slice is accumulated from zero in k order; the slice
// partials are combined as a balanced binary tree ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)). A workgroup walks SK consecutive
// slices (SK = 8: all of K; SK = 2 with grid.y = 4 for the narrow layers, whose 64 column slabs alone would leave 3/4 of
// the CUs idle) and folds finished slices into a binary-counter stack of held partial sums (log2 SK accumulator sets),
// so an aligned group of slices yields exactly its subtree's value; grid.y > 1 writes that value as an fp32 partial and
// gemm_rows_tree_reduce_kernel finishes the tree. Every row's result is bit-identical to what the weight-streaming
// kernel gives that row in a batch of <= 16, whatever the grid (the merged decode iteration of StaggeredDecodePipeline
// stacks 6 such batches and streams the weights once).
template <int EPI, int MB, int NB, int SK = 0>
__global__ __launch_bounds__(256, 2) void gemm_mid_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = 64 * MB, BN = 16 * NB, NWAVE = 4, NST = 3;
  constexpr int A_BYTES = BM * ROW_BYTES, BUF_BYTES = A_BYTES + NB * 2048;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NST × BUF_BYTES
  const int n0 = blockIdx.x * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt32 = p.K >> 5;

  const unsigned a_bytes = (unsigned)min((long)p.M * p.lda * 2, 0xffffffffL);
  const unsigned w_bytes = (unsigned)min((long)p.N * p.K * 2, 0xffffffffL);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, w_bytes, 0x00020000);

  // activation pieces: 8·MB × (8 rows × 128 B); wave takes pieces j*4 + wave. lane → (row = lane>>3, chunk = lane&7)
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffA[2 * MB];
#pragma unroll
  for (int j = 0; j < 2 * MB; ++j) voffA[j] = (unsigned)(((long)((j * NWAVE + wave) * 8 + prow) * p.lda) * 2 + pchunk * 16);
  // weight blocks (1 KiB each): NB n-tiles × 2 k-steps. NB = 4: wave w stages n-tile w (two pieces); NB = 1: waves 0 / 1
  // stage k-step 0 / 1 of the single n-tile, waves 2 / 3 none (their counted waits are one piece shorter)
  constexpr int WP = NB == 4 ? 2 : 1;
  const bool has_w = NB == 4 || wave < 2;
  unsigned voffW[WP];
  int ldsW[WP];
#pragma unroll
  for (int q = 0; q < WP; ++q) {
    const int nt = NB == 4 ? wave : 0, ks = NB == 4 ? q : (wave & 1);
    voffW[q] = (unsigned)(((long)(n0 / 16 + nt) * kt32 + ks) * 1024 + lane * 16);
    ldsW[q] = A_BYTES + (nt * 2 + ks) * 1024;
  }

#define BL_STAGE(BUF, KT)                                                                                   \
  do {                                                                                                      \
    char* base__ = smem + (BUF) * BUF_BYTES;                                                                \
    _Pragma("unroll") for (int j = 0; j < 2 * MB; ++j) BL_GLDS(rsA, base__ + (j * NWAVE + wave) * 1024, voffA[j], (KT) * 128); \
    if (has_w) {                                                                                            \
      _Pragma("unroll") for (int q = 0; q < WP; ++q) BL_GLDS(rsW, base__ + ldsW[q], voffW[q], (KT) * 2048); \
    }                                                                                                       \
  } while (0)
#define BL_WAIT_TILES(T)                                                                                    \
  do {                                                                                                      \
    if (has_w) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((T) * (2 * MB + WP)) : "memory");                   \
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((T) * (2 * MB)) : "memory");                              \
  } while (0)

  const int l15 = lane & 15, lg = lane >> 4;
  const int c0 = lg ^ (lane & 7);
  const int offA = (wave * 16 * MB + l15) * ROW_BYTES;
  const int offW = A_BYTES + lane * 16;                 // block i*2 + ks

  f32x4_t acc[NB][MB];
  constexpr int LV = SK >= 8 ? 3 : SK >= 4 ? 2 : SK >= 2 ? 1 : 0;   // levels of held partial sums
  f32x4_t hold[LV ? LV : 1][SK ? NB : 1][SK ? MB : 1];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  int fold_next = p.fold_ks, sl = 0;        // SK: k-step count at which the current slice ends; local slice index

  const int nk_all = p.K / BK;
  int kt0 = 0, nk = nk_all;
  if constexpr (SK > 0) {                   // slices [blockIdx.y·SK, +SK): SK even → the range starts on a K-tile
    kt0 = (int)blockIdx.y * SK * p.fold_ks / 2;
    nk = kt0 + SK * p.fold_ks / 2;
  } else if (p.splitk > 1) {
    kt0 = (int)(((long)blockIdx.y * nk_all) / p.splitk);
    nk = (int)(((long)(blockIdx.y + 1) * nk_all) / p.splitk);
  }
  BL_STAGE(0, kt0);
  if (kt0 + 1 < nk) BL_STAGE(1, kt0 + 1);
  for (int kt = kt0; kt < nk; ++kt) {
    const int it = kt - kt0;
    if (kt + 2 < nk) {                 // the ring slot read in the previous iteration (all waves are past its barrier)
      BL_STAGE((it + 2) % NST, kt + 2);
      BL_WAIT_TILES(2);
    } else if (kt + 1 < nk) {
      BL_WAIT_TILES(1);
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();      // every wave's pieces of K-tile kt have landed
    const char* base = smem + (it % NST) * BUF_BYTES;
    if constexpr (SK == 0) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int cb = (c0 ^ (ks * 4)) << 4;
        bf16x8_t wf[NB], af[MB];
#pragma unroll
        for (int i = 0; i < NB; ++i) wf[i] = *(const bf16x8_t*)(base + offW + (i * 2 + ks) * 1024);
#pragma unroll
        for (int j = 0; j < MB; ++j) af[j] = *(const bf16x8_t*)(base + offA + j * 16 * ROW_BYTES + cb);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int j = 0; j < MB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], af[j], acc[i][j], 0, 0, 0);
      }
    } else {
      // both k-steps' fragments are read before the first MFMA: the slice-boundary branch between the k-steps would
      // otherwise keep the second k-step's LDS reads from overlapping the first one's MFMAs
      bf16x8_t wf[2][NB], af[2][MB];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int cb = (c0 ^ (ks * 4)) << 4;
#pragma unroll
        for (int i = 0; i < NB; ++i) wf[ks][i] = *(const bf16x8_t*)(base + offW + (i * 2 + ks) * 1024);
#pragma unroll
        for (int j = 0; j < MB; ++j) af[ks][j] = *(const bf16x8_t*)(base + offA + j * 16 * ROW_BYTES + cb);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int j = 0; j < MB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][i], af[ks][j], acc[i][j], 0, 0, 0);
        if (it * 2 + ks + 1 == fold_next) {       // slice boundary (may fall between the two k-steps of a K-tile)
          // binary counter over the local slice index sl (wave-uniform → scalar branches): a finished slice is parked at
          // level 0 or merged upwards while the levels below are occupied; after the group's last slice acc holds the
          // tree value of the whole group
          bool parked = false;
          // opaque to the optimiser: without this hipcc speculates the level-0 add (hold + acc) on EVERY k-step, a VALU
          // read of the accumulators that drains the MFMA pipeline each time (2x slower)
#pragma unroll
          for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < MB; ++j) asm volatile("" : "+v"(acc[i][j]));
#define BL_FOLD_LEVEL(L)                                                                   \
  if constexpr (LV > L) {                                                                   \
    if (!parked) {                                                                          \
      if (!((sl >> L) & 1)) {                                                               \
        _Pragma("unroll") for (int i = 0; i < NB; ++i)                                      \
          _Pragma("unroll") for (int j = 0; j < MB; ++j) hold[L][i][j] = acc[i][j];         \
        parked = true;                                                                      \
      } else {                                                                              \
        _Pragma("unroll") for (int i = 0; i < NB; ++i)                                      \
          _Pragma("unroll") for (int j = 0; j < MB; ++j) acc[i][j] = hold[L][i][j] + acc[i][j]; \
      }                                                                                     \
    }                                                                                       \
  }
          BL_FOLD_LEVEL(0) BL_FOLD_LEVEL(1) BL_FOLD_LEVEL(2)
#undef BL_FOLD_LEVEL
          if (parked) {
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
              for (int j = 0; j < MB; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
          }
          fold_next += p.fold_ks;
          ++sl;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // all reads of this slot done before it is re-issued next iteration
  }
#undef BL_STAGE
#undef BL_WAIT_TILES
  if constexpr (SK > 0) {
    float* slab = p.slab + (long)blockIdx.y * p.M * p.N;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < MB; ++j) {
        const int m = wave * 16 * MB + j * 16 + l15, n = n0 + i * 16 + lg * 4;
        if (gridDim.y == 1) epilogue_store4<EPI>(p, m, n, acc[i][j]);
        else if (m < p.M && n < p.N) *(f32x4_t*)(slab + (long)m * p.N + n) = acc[i][j];
      }
    return;
  }
  if (p.splitk > 1) {
    float* slab = p.slab + (long)blockIdx.y * p.M * p.N;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < MB; ++j) {
        const int m = wave * 16 * MB + j * 16 + l15, n = n0 + i * 16 + lg * 4;
        if (m < p.M && n < p.N) *(f32x4_t*)(slab + (long)m * p.N + n) = acc[i][j];
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j)
      epilogue_store4<EPI>(p, wave * 16 * MB + j * 16 + l15, n0 + i * 16 + lg * 4, acc[i][j]);
#endif
}

// ======================================================================================================================
// "rows-stream" kernel: the skinny order at M ≤ 96 rows (the merged decode iteration) as a WEIGHT-STREAMING kernel for the
// wide layers. Every wave owns one 16-column weight tile and walks the workgroup's K range; weight fragments go
// HBM → VGPR with non-temporal 16-byte loads straight out of the fragment-major packing (never through LDS) into a ring
// of NWB register buffers of GS k-steps: NWB − 1 groups (12 KiB per wave) are in flight while one is consumed. The ≤ 96
// activation rows of a GS-k-step chunk are staged ONCE per workgroup by LDS-DMA (the mid kernel's swizzled 128-byte rows,
// a ring of NWB chunks) and read by every wave as 6 B-fragments per weight fragment: 0.75 – 1.0 staged bytes per weight
// byte instead of the mid kernel's 3 — what a CU can pull through its vector-memory path is capped (≈ 64 KiB of requests
// outstanding: ≈ 57 GB/s per CU out of HBM, tools/micro/hbm_stream.hip), so staged activation bytes cost weight bytes.
// One raw barrier per chunk; counted vmcnt: every wave issues exactly OPS = XP + GS vector-memory operations per chunk
// on every path (surplus chunks re-read the last one), so vmcnt(2·OPS) always leaves exactly the two younger chunks in
// flight and hipcc's own counting for the weight registers comes out the same. The refill of the slot freed by the
// previous chunk is issued a quarter at a time BEHIND each k-step's MFMAs: a load that stalls at issue because the CU's
// request queue is full then stalls under MFMAs that are already in the pipe (−5 % against issuing it in one block).
// Slices, the binary-counter fold and the grid.y split are gemm_mid_kernel<SK>'s: results are bit-identical to it and to
// gemm_skinny_kernel. fold_ks must be a multiple of GS (K a multiple of 1024: slices end on chunk boundaries, the
// slice-boundary test runs once per chunk) — the launcher sends everything else to the mid kernel.
// ======================================================================================================================
template <int EPI, int NWV, int SK>
__global__ __launch_bounds__(NWV * 64) void gemm_rows_stream_kernel(GemmArgs p, int n_tiles) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int MR = 6, GS = 4, NWB = 4;
  constexpr int KT_BYTES = MR * 16 * ROW_BYTES, XBUF = 2 * KT_BYTES;   // one K-tile (2 k-steps) of all rows; one chunk
  constexpr int XP = 24 / NWV, OPS = XP + GS;
  static_assert(24 % NWV == 0 && XP <= GS, "the chunk's 24 LDS-DMA pieces are dealt evenly to the waves, one per k-step");
  constexpr int LV = SK >= 8 ? 3 : SK >= 4 ? 2 : SK >= 2 ? 1 : 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];          // NWB × XBUF
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lg = lane >> 4;
  const int tile_raw = (int)blockIdx.x * NWV + wave;
  const bool live = tile_raw < n_tiles;
  const int tile = live ? tile_raw : n_tiles - 1;        // a surplus wave streams the last tile again and stores nothing
  const int kt32 = p.K >> 5;
  const int ks0 = (int)blockIdx.y * SK * p.fold_ks, nks = SK * p.fold_ks;   // this workgroup's k-steps [ks0, ks0 + nks)
  const int NC = (nks + GS - 1) / GS;

  const unsigned a_bytes = (unsigned)min((long)p.M * p.lda * 2, 0xffffffffL);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, a_bytes, 0x00020000);
  // activation pieces (8 rows × 128 B): piece q = j·NWV + wave → K-tile q / 12 of the chunk, row block q % 12
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffA[XP];
  int ldsA[XP];
#pragma unroll
  for (int j = 0; j < XP; ++j) {
    const int q = j * NWV + wave, kt = q / 12, rb = q - kt * 12;
    voffA[j] = (unsigned)(((long)(rb * 8 + prow) * p.lda) * 2 + kt * 128 + pchunk * 16);
    ldsA[j] = kt * KT_BYTES + rb * 1024;
  }
  const u32x4_t* wbase = (const u32x4_t*)p.W + ((long)tile * kt32 + ks0) * 64 + lane;
  u32x4_t wbuf[NWB][GS];

  // part J (of GS) of chunk C into ring slot SLOT: LDS-DMA piece J (if the wave has one) and weight fragment J. Chunk
  // and k-step indices are clamped, so every call issues the same operations whatever C is.
#define BL_RS_ISSUE_PART(SLOT, C, J)                                                                          \
  do {                                                                                                        \
    const int cc__ = min((C), NC - 1);                                                                        \
    if ((J) < XP) BL_GLDS(rsA, smem + (SLOT) * XBUF + ldsA[(J) < XP ? (J) : 0], voffA[(J) < XP ? (J) : 0], (ks0 + cc__ * GS) * 64); \
    wbuf[SLOT][J] = __builtin_nontemporal_load(wbase + (long)min(cc__ * GS + (J), nks - 1) * 64);             \
  } while (0)
#define BL_RS_READX(DST, XB, S)                                                                               \
  do {                                                                                                        \
    const char* xs__ = (XB) + ((S) >> 1) * KT_BYTES + offA + ((c0 ^ (((S) & 1) * 4)) << 4);                    \
    _Pragma("unroll") for (int j = 0; j < MR; ++j) DST[j] = *(const bf16x8_t*)(xs__ + j * 16 * ROW_BYTES);    \
  } while (0)
#define BL_RS_FOLD_LEVEL(L)                                                                \
  if constexpr (LV > L) {                                                                   \
    if (!parked) {                                                                          \
      if (!((sl >> L) & 1)) {                                                               \
        _Pragma("unroll") for (int j = 0; j < MR; ++j) hold[L][j] = acc[j];                 \
        parked = true;                                                                      \
      } else {                                                                              \
        _Pragma("unroll") for (int j = 0; j < MR; ++j) acc[j] = hold[L][j] + acc[j];        \
      }                                                                                     \
    }                                                                                       \
  }
  // one chunk: counted wait, barrier (every wave's pieces of chunk C have landed; every wave is done with chunk C − 1, whose
  // ring slot the refill below overwrites), then GS × (next k-step's fragments LDS → VGPR, 6 MFMAs, a quarter of the refill)
#define BL_RS_CHUNK(SLOT, C)                                                                                  \
  {                                                                                                           \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * OPS) : "memory");                                            \
    __builtin_amdgcn_s_barrier();                                                                             \
    const char* xb = smem + (SLOT) * XBUF;                                                                    \
    bf16x8_t xf[2][MR];                                                                                       \
    BL_RS_READX(xf[0], xb, 0);                                                                                \
    _Pragma("unroll") for (int s2 = 0; s2 < GS; ++s2) {                                                       \
      if (s2 + 1 < GS) BL_RS_READX(xf[(s2 + 1) & 1], xb, s2 + 1);                                             \
      __builtin_amdgcn_sched_barrier(0);   /* next k-step's fragments are in flight under this one's MFMAs */ \
      const int kidx = (C) * GS + s2;                                                                         \
      if (kidx < nks) {                                                                                       \
        const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, wbuf[SLOT][s2]);                                     \
        _Pragma("unroll") for (int j = 0; j < MR; ++j)                                                        \
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[s2 & 1][j], acc[j], 0, 0, 0);               \
        if (SK > 1 && s2 == GS - 1 && kidx + 1 == fold_next) {   /* slices end on chunk boundaries */        \
          bool parked = false;                                                                                \
          /* opaque to the optimiser, as in gemm_mid_kernel: no speculated VALU read of the accumulators */    \
          _Pragma("unroll") for (int j = 0; j < MR; ++j) asm volatile("" : "+v"(acc[j]));                     \
          BL_RS_FOLD_LEVEL(0) BL_RS_FOLD_LEVEL(1) BL_RS_FOLD_LEVEL(2)                                         \
          if (parked) {                                                                                       \
            _Pragma("unroll") for (int j = 0; j < MR; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};            \
          }                                                                                                   \
          fold_next += p.fold_ks;                                                                             \
          ++sl;                                                                                               \
        }                                                                                                     \
      }                                                                                                       \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
      BL_RS_ISSUE_PART(((SLOT) + NWB - 1) % NWB, (C) + NWB - 1, s2);                                          \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
    }                                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                        \
  }

  const int c0 = lg ^ (lane & 7);
  const int offA = l15 * ROW_BYTES;
  f32x4_t acc[MR], hold[LV ? LV : 1][MR];
#pragma unroll
  for (int j = 0; j < MR; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  int fold_next = p.fold_ks, sl = 0;

  // prologue: chunks 0 … NWB-2 in flight, chunk by chunk (the counted waits rely on whole chunks being issued in order)
#pragma unroll
  for (int c = 0; c < NWB - 1; ++c) {
#pragma unroll
    for (int j = 0; j < GS; ++j) BL_RS_ISSUE_PART(c, c, j);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int cb = 0; cb < NC; cb += NWB) {   // whole rounds of NWB chunks; chunks past NC only skip their MFMAs
    BL_RS_CHUNK(0, cb)
    BL_RS_CHUNK(1, cb + 1)
    BL_RS_CHUNK(2, cb + 2)
    BL_RS_CHUNK(3, cb + 3)
  }
#undef BL_RS_CHUNK
#undef BL_RS_FOLD_LEVEL
#undef BL_RS_READX
#undef BL_RS_ISSUE_PART
  if (!live) return;
  float* slab = p.slab + (long)blockIdx.y * p.M * p.N;
#pragma unroll
  for (int j = 0; j < MR; ++j) {
    const int m = j * 16 + l15, n = tile * 16 + lg * 4;
    if (gridDim.y == 1) epilogue_store4<EPI>(p, m, n, acc[j]);
    else if (m < p.M) *(f32x4_t*)(slab + (long)m * p.N + n) = acc[j];
  }
#endif
}

// ======================================================================================================================
// "mid2" kernel: 160 rows × 32 columns per workgroup, 4 waves as 2 (m) × 2 (n), 3-stage ring — the narrow layers
// (N = 4096 o / down, ViT proj / fc2) at 128 < M ≤ 320. The mid kernel's 16-column slabs re-stage ALL rows of A per
// workgroup (42 KB per K-step for 0.66 MFLOP), and the CU's global→LDS path (one 1-KiB piece per ≈ 20 cycles) is what
// bounds it; half the rows and twice the columns stage 24 KB for 0.66 MFLOP with as many workgroups. Same K order per
// output as every other kernel (bit-identical results).
// ======================================================================================================================
template <int EPI, int NT, int NST = 3>   // NT = 16-column tiles per wave: 32·NT columns per workgroup; NST ring stages
__global__ __launch_bounds__(256) void gemm_mid2_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = 160, BN = 32 * NT, MT = 5, LPS = 5 + NT;   // LPS: LDS-DMA pieces per wave and stage (5 A + NT W)
  constexpr int A_BYTES = BM * ROW_BYTES, BUF_BYTES = A_BYTES + NT * 4096;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NST × BUF_BYTES
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int kt32 = p.K >> 5;

  const unsigned a_bytes = (unsigned)min((long)p.M * p.lda * 2, 0xffffffffL);
  const unsigned w_bytes = (unsigned)min((long)p.N * p.K * 2, 0xffffffffL);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, w_bytes, 0x00020000);

  // activation pieces: 20 × (8 rows × 128 B); wave takes pieces j*4 + wave. weight blocks: (n-tile, k-step) = (wave >> 1, wave & 1)
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffA[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) voffA[j] = (unsigned)(((long)(m0 + (j * 4 + wave) * 8 + prow) * p.lda) * 2 + pchunk * 16);
  unsigned voffW[NT];                            // weight block b = j*4 + wave: n-tile b >> 1, k-step b & 1, LDS slot b
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int blk = j * 4 + wave;
    voffW[j] = (unsigned)(((long)(n0 / 16 + (blk >> 1)) * kt32 + (blk & 1)) * 1024 + lane * 16);
  }

#define BL_STAGE(BUF, KT)                                                                                   \
  do {                                                                                                      \
    char* base__ = smem + (BUF) * BUF_BYTES;                                                                \
    _Pragma("unroll") for (int j = 0; j < MT; ++j) BL_GLDS(rsA, base__ + (j * 4 + wave) * 1024, voffA[j], (KT) * 128); \
    _Pragma("unroll") for (int j = 0; j < NT; ++j) BL_GLDS(rsW, base__ + A_BYTES + (j * 4 + wave) * 1024, voffW[j], (KT) * 2048); \
  } while (0)

  const int l15 = lane & 15, lg = lane >> 4;
  const int c0 = lg ^ (lane & 7);
  const int offA = (wm * 80 + l15) * ROW_BYTES;
  const int offW = A_BYTES + (wn * NT) * 2048 + lane * 16;   // block (wn*NT + i)*2 + ks

  f32x4_t acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  static_assert(NST == 2 || NST == 3, "ring depth");
  BL_STAGE(0, 0);
  if (NST == 3 && 1 < nk) BL_STAGE(1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    // issue K-tile kt+NST-1 into the ring slot read in the previous iteration (all waves are past its barrier), then wait
    // for K-tile kt with the newer ones still in flight
    if (kt + NST - 1 < nk) BL_STAGE((kt + NST - 1) % NST, kt + NST - 1);
    const int later = min(NST - 1, nk - 1 - kt);
    if (later == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // every wave's pieces of K-tile kt have landed
    const char* base = smem + (kt % NST) * BUF_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cb = (c0 ^ (ks * 4)) << 4;
      bf16x8_t wf[NT], af[MT];
#pragma unroll
      for (int i = 0; i < NT; ++i) wf[i] = *(const bf16x8_t*)(base + offW + i * 2048 + ks * 1024);
#pragma unroll
      for (int j = 0; j < MT; ++j) af[j] = *(const bf16x8_t*)(base + offA + j * 16 * ROW_BYTES + cb);
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], af[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // all reads of this slot done before it is re-issued next iteration
  }
#undef BL_STAGE
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j)
      epilogue_store4<EPI>(p, m0 + wm * 80 + j * 16 + l15, n0 + (wn * NT + i) * 16 + lg * 4, acc[i][j]);
#endif
}

// ======================================================================================================================
// 288 × 256 tile — one 288-token sequence (S = 1 + 256 + 31) per row tile.
// At the bench shape M = 16 · 288 = 4608 the 256-row tiles come out as 18 row tiles: Llama o_proj / down_proj get 288 tiles
// = one round + a 32-tile tail on sub-tiles at a third of the efficiency (+ 45 % time for 12.5 % of the work), qkv gets
// 864 = 3.375 rounds (a quarter-filled fourth round). With 288 rows per tile the same GEMMs are exactly 256 tiles
// (o / down) and 768 = 3 rounds (qkv): no tail, no partial round.
// 8 waves as 2 (m) × 4 (n): a wave owns 144 rows × 64 columns = 9 × 4 accumulator tiles (144 VGPRs). LDS: 2 stages × 72 KiB
// (288 rows × 128 B + 4 KiB landing area for the surplus pieces + 32 KiB weights). A wave issues 9 LDS-DMA pieces per
// K-tile: 5 activation — 36 real ones over 8 waves, the 4 surplus ones hit a zero-size descriptor: no traffic — and 4
// weight. K order per output = every other kernel's (K-tile by K-tile, two 32-steps each): bit-identical results.
// Staggered wave groups (the structure of gemm256s_kernel on the 288-row tile): the two 4-wave groups that
// share each SIMD alternate roles segment by segment — one runs a 24-MFMA phase while the other reads the fragments of its
// next phase and issues LDS-DMA pieces — with one raw s_barrier per segment. Three phases per K-tile: phase q runs
// activation third q (48 of the wave's 144 rows) against all four weight column tiles, both k-steps. A single X register
// set suffices (a group's fragment reads happen while its MFMAs are not running) and the K-tile's 8 weight fragments are
// read once: 9 × 4 accumulator tiles (144 VGPRs) + 6 + 4 + 4 fragments.
// Slot q of K-tile T (before phase q; reads first, pieces second):
//   slot 0: reads X third 0 + Ya + Yb (14), issues activation pieces 0, 1 of T+1
//   slot 1: reads X third 1 (6),            issues activation pieces 2, 3, 4 of T+1
//   slot 2: reads X third 2 (6),            issues the four weight pieces of T+2, waits `vmcnt(4)`
// Segments (one barrier after each): group A runs slot q of T in segment 6T + 2q - 1, group B in segment 6T + 2q.
// LDS reuse rule, held by construction: a piece is issued into a stage only after a barrier that follows the last
// fragment read of the rows it overwrites by BOTH groups (reads are complete at the slot's lgkmcnt(0), before its barrier).
//   - slots 0 and 1 of T (segments ≥ 6T - 1) write stage T+1 = the stage of T-1, whose last read is group B's slot 2 of
//     T-1 in segment 6T - 2.
//   - slot 2 of T (segments 6T + 3 / 6T + 4) writes stage T while third 2 of it is still being read (B's slot 2 runs in
//     6T + 4, beside other waves' issues). It therefore issues only the weight pieces: the weight area of stage T is last
//     read in slot 0 (segment 6T by B). No activation piece but piece 0 lies wholly inside thirds 0 and 1.
// Landing: at slot 2 of T the wave's queue holds, oldest first, the nine pieces of T+1 (4 from slot 2 of T-1, 2 + 3 from
// slots 0, 1 of T) and the four of T+2 just issued; `vmcnt(4)` leaves only those four outstanding, so all of T+1 has
// landed when B's slot 2 ends (segment 6T + 4) and A's first read of T+1 is in segment 6T + 5, one barrier on. The DMA
// stream never drains and there is no `vmcnt(0)` in the loop. Nothing else orders a ds_read behind a pending LDS-DMA.
// ======================================================================================================================
template <int EPI>
__global__ __launch_bounds__(512) void gemm288s_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = 288, BN = 256;
  constexpr int A_BYTES = BM * ROW_BYTES, DUMMY = A_BYTES, W_OFF = A_BYTES + 4096, STAGE = W_OFF + 32768;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 × STAGE
  int tm, tn;
  tile_coords(p, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, lg = lane >> 4;
  const int kt32 = p.K >> 5, nk = p.K / BK;

  const unsigned a_bytes = (unsigned)min((long)p.M * p.lda * 2, 0xffffffffL);
  const unsigned w_bytes = (unsigned)min((long)p.N * p.K * 2, 0xffffffffL);
  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffA[5];
  int ldsA[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int pi = wave + 8 * j;
    voffA[j] = (unsigned)(((long)(m0 + pi * 8 + prow) * p.lda) * 2 + pchunk * 16);
    ldsA[j] = pi < 36 ? pi * 1024 : DUMMY + (pi - 36) * 1024;
  }
  const unsigned a4_bytes = wave < 4 ? a_bytes : 0u;      // piece wave + 32 exists for waves 0..3 only (zero-size descriptor)
  unsigned voffW[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) voffW[q] = (unsigned)((long)(n0 / 16 + 2 * wave + q) * kt32 * 1024 + lane * 16);
  const int ldsW = W_OFF + 2 * wave * 2048;
#define BL_RS(PTR, BYTES) __builtin_amdgcn_make_buffer_rsrc((void*)(PTR), 0, (BYTES), 0x00020000)
#define ISSUE_A(J, TILE)                                                                                  \
  do {                                                                                                    \
    const int t__ = (TILE);                                                                               \
    const __amdgpu_buffer_rsrc_t rs__ = BL_RS(p.A, t__ < nk ? ((J) < 4 ? a_bytes : a4_bytes) : 0u);       \
    BL_GLDS(rs__, smem + (t__ & 1) * STAGE + ldsA[J], voffA[J], t__ * 128);                               \
  } while (0)
#define ISSUE_W(Q, KS, TILE)                                                                              \
  do {                                                                                                    \
    const int t__ = (TILE);                                                                               \
    const __amdgpu_buffer_rsrc_t rs__ = BL_RS(p.W, t__ < nk ? w_bytes : 0u);                              \
    BL_GLDS(rs__, smem + (t__ & 1) * STAGE + ldsW + (Q) * 2048 + (KS) * 1024, voffW[Q] + (KS) * 1024, t__ * 2048); \
  } while (0)
  const int cb0 = (lg ^ (lane & 7)) << 4;
  const int offX = (wm * 144 + l15) * ROW_BYTES;
  const int offY = W_OFF + wn * 8192 + lane * 16;
#define READ_X(T3, SB)                                                                                    \
  _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                                         \
    X[i * 2] = *(const bf16x8_t*)((SB) + offX + (3 * (T3) + i) * 2048 + cb0);                             \
    X[i * 2 + 1] = *(const bf16x8_t*)((SB) + offX + (3 * (T3) + i) * 2048 + (cb0 ^ 64));                  \
  }
#define READ_Y(DST, NH, SB)                                                                               \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                         \
    DST[j * 2] = *(const bf16x8_t*)((SB) + offY + (2 * (NH) + j) * 2048);                                 \
    DST[j * 2 + 1] = *(const bf16x8_t*)((SB) + offY + (2 * (NH) + j) * 2048 + 1024);                      \
  }
#define MMA(YR, T3, NH)                                                                                   \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                        \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                         \
      _Pragma("unroll") for (int i = 0; i < 3; ++i)                                                       \
        acc[2 * (NH) + j][3 * (T3) + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                        \
            YR[j * 2 + ks], X[i * 2 + ks], acc[2 * (NH) + j][3 * (T3) + i], 0, 0, 0);
  // phase T3: activation third T3 against all four weight column tiles, both k-steps — 24 MFMAs
#define PHASE(T3)                                                                                         \
  do {                                                                                                    \
    __builtin_amdgcn_s_setprio(1);                                                                        \
    MMA(Ya, T3, 0)                                                                                        \
    MMA(Yb, T3, 1)                                                                                        \
    __builtin_amdgcn_s_setprio(0);                                                                        \
  } while (0)
#define BAR()                                                                                             \
  do {                                                                                                    \
    __builtin_amdgcn_s_barrier();                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                    \
  } while (0)
#define WAIT_LGKM() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define WAIT_VM4_LGKM() asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory")
  // the three slots of K-tile T (stage SC): fragment reads first, then the LDS-DMA issue
#define SLOT0(SC, T) do { READ_X(0, SC); READ_Y(Ya, 0, SC); READ_Y(Yb, 1, SC); __builtin_amdgcn_sched_barrier(0); ISSUE_A(0, (T) + 1); ISSUE_A(1, (T) + 1); WAIT_LGKM(); } while (0)
#define SLOT1(SC, T) do { READ_X(1, SC); __builtin_amdgcn_sched_barrier(0); ISSUE_A(2, (T) + 1); ISSUE_A(3, (T) + 1); ISSUE_A(4, (T) + 1); WAIT_LGKM(); } while (0)
#define SLOT2(SC, T) do { READ_X(2, SC); __builtin_amdgcn_sched_barrier(0); ISSUE_W(0, 0, (T) + 2); ISSUE_W(0, 1, (T) + 2); ISSUE_W(1, 0, (T) + 2); ISSUE_W(1, 1, (T) + 2); WAIT_VM4_LGKM(); } while (0)
#define BL_EPILOGUE()                                                                                     \
  do {                                                                                                    \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                      \
    const int ncol__[4] = {n0 + wn * 64 + lg * 4, n0 + wn * 64 + 16 + lg * 4, n0 + wn * 64 + 32 + lg * 4,      \
                           n0 + wn * 64 + 48 + lg * 4};                                                   \
    epilogue_tile<EPI, 4, 9>(p, m0 + wm * 144 + l15, ncol__, m0 + 288, n0 + 256, acc);                    \
  } while (0)

  f32x4_t acc[4][9];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  bf16x8_t X[6], Ya[4], Yb[4];
  char* const S0 = smem;
  char* const S1 = smem + STAGE;

  // prologue: all nine pieces of K-tile 0, then what slot 2 of "K-tile -1" issues (the four weight pieces of K-tile 1)
  ISSUE_A(0, 0); ISSUE_A(1, 0); ISSUE_A(2, 0); ISSUE_A(3, 0); ISSUE_A(4, 0);
  ISSUE_W(0, 0, 0); ISSUE_W(0, 1, 0); ISSUE_W(1, 0, 0); ISSUE_W(1, 1, 0);
  ISSUE_W(0, 0, 1); ISSUE_W(0, 1, 1); ISSUE_W(1, 0, 1); ISSUE_W(1, 1, 1);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  BAR();
  if (wm == 0) {
    // ======================= group A: MFMA phase first, then the slot of the NEXT phase =======================
    SLOT0(S0, 0);
    BAR();
    for (int t = 0; t < nk; t += 2) {        // nk is even (launcher: K % 128 == 0)
      PHASE(0); BAR();   SLOT1(S0, t); BAR();
      PHASE(1); BAR();   SLOT2(S0, t); BAR();
      PHASE(2); BAR();   SLOT0(S1, t + 1); BAR();
      PHASE(0); BAR();   SLOT1(S1, t + 1); BAR();
      PHASE(1); BAR();   SLOT2(S1, t + 1); BAR();
      PHASE(2); BAR();   SLOT0(S0, t + 2); BAR();
    }
    BL_EPILOGUE();
    return;
  }
  // ========================= group B: the slot of THIS phase first, then its MFMA phase =========================
  BAR();
  for (int t = 0; t < nk; t += 2) {
    SLOT0(S0, t); BAR();       PHASE(0); BAR();
    SLOT1(S0, t); BAR();       PHASE(1); BAR();
    SLOT2(S0, t); BAR();       PHASE(2); BAR();
    SLOT0(S1, t + 1); BAR();   PHASE(0); BAR();
    SLOT1(S1, t + 1); BAR();   PHASE(1); BAR();
    SLOT2(S1, t + 1); BAR();   PHASE(2); BAR();
  }
  BL_EPILOGUE();
#undef BL_RS
#undef ISSUE_A
#undef ISSUE_W
#undef READ_X
#undef READ_Y
#undef MMA
#undef PHASE
#undef BAR
#undef WAIT_LGKM
#undef WAIT_VM4_LGKM
#undef SLOT0
#undef SLOT1
#undef SLOT2
#undef BL_EPILOGUE
#endif
}

// ======================================================================================================================
// 256 × 256 tile, 8 waves (128(m) × 64(n) each), 128 KiB LDS = 2 stages, 1 workgroup per CU. Each K-tile is staged as four
// 16-KiB HALF-TILES (X0/X1 = the two 64-row halves of every wave's activation rows, Y0/Y1 = the two 32-row halves of every
// wave's weight rows) and consumed in four PHASES of 16 MFMAs (output quadrants (0,0) (0,1) (1,1) (1,0)).
// STAGGERED wave groups: waves 0-3 (group A, wm = 0) and waves 4-7 (group B, wm = 1) share each SIMD
// pairwise; running them half a phase apart lets one group's 16 MFMAs cover the other group's LDS-DMA issue and
// fragment reads, so the matrix pipe no longer idles while both waves of a SIMD load in lockstep
// (square 8k: 1328 → 1430 TFLOP/s; Llama layer GEMMs 1719 → 1594 µs).
//
//   segment 2p   : A: MMA(p)                      B: ISSUE H(p+6), READ(p)
//   segment 2p+1 : A: ISSUE H(p+6), READ(p+1)     B: MMA(p)                       (one raw s_barrier after every segment)
//
// p = global phase (4 per K-tile, quadrants (0,0)(0,1)(1,1)(1,0)); H(p) = the half-tile first read for phase p:
// X0(t), Y1(t), X1(t), Y0(t+1). Half-tiles are issued 6 phases ahead in need order; H(p+1) must be complete before
// segment 2p+1, so at the end of segment 2p group A (issued up to H(p+5)) waits vmcnt(8) and group B (up to H(p+6))
// vmcnt(10). A buffer is re-issued ≥ 2 barriers after its last read. Fragments: one activation set (X), two weight sets.
// (Tried and rejected: prefetching the next phase's fragments inside the group's own MMA segment — hipcc serialises the
// reads ahead of the MFMAs, the MMA segment grows, 1430 → 1286 TFLOP/s.)
// ======================================================================================================================
template <int EPI, bool TN = false>
__global__ __launch_bounds__(512) void gemm256s_kernel(GemmArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = 256, BN = 256;
  constexpr int STAGE = 65536, W_OFF = 32768;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int tm, tn;
  const int nk_all = TN ? (p.K + BK - 1) / BK : p.K / BK;
  int kt_begin = 0, nk = nk_all;
  // Persistent form (p.ptiles > 0, round 4): the launch has one workgroup per CU and workgroup b walks tiles b, b + grid,
  // b + 2·grid … < ptiles of the XCD-contiguous order. The K streams of consecutive tiles are FLATTENED: the loop below
  // issues its LDS-DMA half-tiles 1.5 K-tiles ahead, and what used to be zero-size loads past the end of K (K-tiles nk,
  // nk + 1) are now the first two K-tiles of the workgroup's next tile — exactly the seven half-tiles of the prologue, in
  // its order, into the stages the next tile expects (nk is even) — so the next tile starts with its operands in LDS and
  // its first fragments in registers, behind this tile's epilogue instead of behind a workgroup launch and a cold prologue.
  const int ptiles = p.splitk > 1 ? 0 : p.ptiles;
  int vb = blockIdx.x;                     // virtual block index of the current tile
  if (p.splitk > 1) {
    lin_to_tile(p, p.tail_base + blockIdx.x / p.splitk, tm, tn);
    const int slice = blockIdx.x % p.splitk;
    kt_begin = (int)(((long)slice * nk_all) / p.splitk) & ~1;
    nk = slice + 1 == p.splitk ? nk_all : ((int)(((long)(slice + 1) * nk_all) / p.splitk) & ~1);
  } else if (ptiles > 0) {
    tile_coords_v(p, vb, ptiles, tm, tn);
  } else {
    tile_coords(p, tm, tn);
  }
  int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, lg = lane >> 4;
  const int kt32 = p.K >> 5;

  // TN (C = Aᵀ·B, the weight gradient dW = dyᵀ·x read UNtransposed): A is [K tokens, M] and W is [K tokens, N], both
  // row-major; a K-tile is 64 token rows of each. The descriptors end with the last token row's last column (the exact
  // extent of a column-slice view), so K-tiles past the end and the ragged last one read zeros.
  // The per-lane offsets below are TILE-RELATIVE; the tile's origin goes into the buffer descriptor's base (uniform), and
  // its size shrinks by the same bytes, so the bounds check (zero-fill past M / N / K) sees what it saw with absolute
  // offsets. A tile's (base, size) pair is rebuilt per tile from (m0, n0): TILE_A / TILE_W.
  const long a_total = TN ? ((long)(p.K - 1) * p.lda + p.M) * 2 : (long)p.M * p.lda * 2;
  const long w_total = TN ? ((long)(p.K - 1) * p.ldw + p.N) * 2 : (long)p.N * p.K * 2;
  const int kstepX = TN ? (int)(64 * p.lda * 2) : 128, kstepY = TN ? (int)(64 * p.ldw * 2) : 2048;
#define TILE_A_OFF(M0) (TN ? (long)(M0) * 2 : (long)(M0) * p.lda * 2)
#define TILE_W_OFF(N0) (TN ? (long)(N0) * 2 : (long)((N0) / 16) * (p.K >> 5) * 1024)
  const char* Acur = (const char*)p.A + TILE_A_OFF(m0);
  const char* Wcur = (const char*)p.W + TILE_W_OFF(n0);
  unsigned a_bytes = (unsigned)min(a_total - TILE_A_OFF(m0), 0xffffffffL);
  unsigned w_bytes = (unsigned)min(w_total - TILE_W_OFF(n0), 0xffffffffL);
  // the workgroup's NEXT tile (size 0 = none: loads past the end of K write zeros, as they always did)
  const char* Anext = Acur; const char* Wnext = Wcur;
  unsigned a_bytes_next = 0u, w_bytes_next = 0u;
  int m0_next = 0, n0_next = 0;
#define BL_NEXT_TILE()                                                                      \
  do {                                                                                      \
    a_bytes_next = 0u; w_bytes_next = 0u;                                                   \
    if (ptiles > 0 && vb + (int)gridDim.x < ptiles) {                                       \
      int tm__, tn__;                                                                       \
      tile_coords_v(p, vb + (int)gridDim.x, ptiles, tm__, tn__);                            \
      m0_next = tm__ * BM; n0_next = tn__ * BN;                                             \
      Anext = (const char*)p.A + TILE_A_OFF(m0_next);                                       \
      Wnext = (const char*)p.W + TILE_W_OFF(n0_next);                                       \
      a_bytes_next = (unsigned)min(a_total - TILE_A_OFF(m0_next), 0xffffffffL);             \
      w_bytes_next = (unsigned)min(w_total - TILE_W_OFF(n0_next), 0xffffffffL);             \
    }                                                                                       \
  } while (0)
  BL_NEXT_TILE();

  const int prow = lane >> 3, pchunk = (lane & 7) ^ prow;
  unsigned voffX[2][2], voffY[2][2];
  int ldsX[2][2], ldsY[2];
  if constexpr (!TN) {
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int pi = 2 * wave + j, row0 = (pi >> 3) * 128 + mh * 64 + (pi & 7) * 8;
        voffX[mh][j] = (unsigned)(((long)(row0 + prow) * p.lda) * 2 + pchunk * 16);
        ldsX[mh][j] = row0 * ROW_BYTES;
      }
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      const int nt = (wave >> 1) * 4 + 2 * nh + (wave & 1);
      voffY[nh][0] = (unsigned)((long)nt * kt32 * 1024 + lane * 16);
      voffY[nh][1] = voffY[nh][0] + 1024;
      ldsY[nh] = W_OFF + nt * 2048;
    }
  } else {
    // LDS keeps the NT kernel's regions but token-major inside them: X block (wm', mh) = [64 tokens][64 columns = 128 B],
    // Y half nh = [64 tokens][128 columns = 256 B]. The fragments come from transposing reads (ds_read_b64_tr_b16:
    // a 32-lane half touches 8 token rows × 32 B), so 32-byte chunk PAIRS are swizzled against the token index:
    // X pair' = pair ^ ((t >> 1) & 3), Y pair' = pair ^ (t & 7) — the 8 rows then cover all 64 banks once.
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int pi = 2 * wave + j, t = (pi & 7) * 8 + prow, pos = lane & 7;
        const int c = ((((pos >> 1) ^ ((t >> 1) & 3)) << 1) | (pos & 1));
        voffX[mh][j] = (unsigned)((long)t * p.lda * 2 + (long)((pi >> 3) * 128 + mh * 64) * 2 + c * 16);
        ldsX[mh][j] = ((pi >> 3) * 128 + mh * 64 + (pi & 7) * 8) * ROW_BYTES;
      }
    // Y half nh = columns nh*128 .. +127 of the tile: [64 tokens][256 B], whole 128-byte lines per piece (4 token rows × 256 B;
    // a 64-byte-segment layout made every line travel twice: −30 %). Wave wn computes columns nh*128 + wn*32 + j*16 + (0..15).
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int t = (2 * wave + j) * 4 + (lane >> 4), pos = lane & 15;
        const int c = ((((pos >> 1) ^ (t & 7)) << 1) | (pos & 1));
        voffY[nh][j] = (unsigned)((long)t * p.ldw * 2 + (long)(nh * 128) * 2 + c * 16);
      }
      ldsY[nh] = W_OFF + nh * 16384 + wave * 2048;
    }
  }
// past the end of K the descriptor's size is 0 (the load then writes zeros): only that one dword of it varies
#define BL_RS(PTR, BYTES) __builtin_amdgcn_make_buffer_rsrc((void*)(PTR), 0, (BYTES), 0x00020000)
#define ISSUE_X(MH, TILE)                                                                   \
  do {                                                                                      \
    const int t__ = (TILE);                                                                 \
    const bool nx__ = t__ >= nk;                 /* K-tile t - nk of the next tile */        \
    const int tt__ = nx__ ? t__ - nk : t__;                                                 \
    const __amdgpu_buffer_rsrc_t rs__ = BL_RS(nx__ ? Anext : Acur, nx__ ? a_bytes_next : a_bytes); \
    char* b__ = smem + (t__ & 1) * STAGE;                                                   \
    BL_GLDS(rs__, b__ + ldsX[MH][0], voffX[MH][0], tt__ * kstepX);                             \
    BL_GLDS(rs__, b__ + ldsX[MH][1], voffX[MH][1], tt__ * kstepX);                             \
  } while (0)
#define ISSUE_Y(NH, TILE)                                                                   \
  do {                                                                                      \
    const int t__ = (TILE);                                                                 \
    const bool nx__ = t__ >= nk;                                                            \
    const int tt__ = nx__ ? t__ - nk : t__;                                                 \
    const __amdgpu_buffer_rsrc_t rs__ = BL_RS(nx__ ? Wnext : Wcur, nx__ ? w_bytes_next : w_bytes); \
    char* b__ = smem + (t__ & 1) * STAGE;                                                   \
    BL_GLDS(rs__, b__ + ldsY[NH], voffY[NH][0], tt__ * kstepY);                               \
    BL_GLDS(rs__, b__ + ldsY[NH] + 1024, voffY[NH][1], tt__ * kstepY);                        \
  } while (0)
  const int cb0 = (lg ^ (lane & 7)) << 4;
  const int offX = (wm * 128 + l15) * ROW_BYTES;
  const int offY = W_OFF + wn * 8192 + lane * 16;
  // TN: lane 4q+u of a 16-lane group addresses token row 4·lg + q, 8-byte unit u of the 16-column block and receives
  // column l15 of the four rows; the second read is 16 tokens further → slots 0-3 / 4-7 of the MFMA operand hold tokens
  // {4lg..4lg+3} and {16+4lg..}, the same for both operands.
  const int trX = (wm * 128) * ROW_BYTES + (4 * lg + (l15 >> 2)) * 128 + (l15 & 3) * 8, swX = ((lg & 1) << 1) | (l15 >> 3);
  const int trY = W_OFF + (4 * lg + (l15 >> 2)) * 256 + (l15 & 3) * 8, swY = ((lg & 1) << 2) | (l15 >> 2);
  // The transposing reads are inline asm: through the builtin, hipcc orders every one of them behind ALL outstanding LDS-DMA
  // (`s_waitcnt vmcnt(0)` before each read group — the intrinsic carries no memory operand to disambiguate), which
  // serialises the staging pipeline (−30 %). The asm results land asynchronously, so they are only touched after the
  // explicit lgkmcnt wait + barrier that precede every MMA, where BL_PIN marks them as produced.
  const unsigned ldsbase = (unsigned)(size_t)LDS_PTR(smem);
#define BL_TR(DST, ADDR, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))
#define BL_PIN(R) asm volatile("" : "+v"(R))
#define READ_X(DST, MH, SB)                                                                             \
  do {                                                                                                  \
    if constexpr (!TN) {                                                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
        DST[i * 2] = *(const bf16x8_t*)((SB) + offX + (MH) * 8192 + i * 2048 + cb0);                    \
        DST[i * 2 + 1] = *(const bf16x8_t*)((SB) + offX + (MH) * 8192 + i * 2048 + (cb0 ^ 64));        \
      }                                                                                                 \
    } else {                                                                                            \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
        const unsigned a__ = ldsbase + (unsigned)((SB) - smem) + trX + ((i ^ swX) << 5);                \
        BL_TR(DST##2[i * 4 + 0], a__, (MH) * 8192);                                                     \
        BL_TR(DST##2[i * 4 + 1], a__, (MH) * 8192 + 2048);                                              \
        BL_TR(DST##2[i * 4 + 2], a__, (MH) * 8192 + 4096);                                              \
        BL_TR(DST##2[i * 4 + 3], a__, (MH) * 8192 + 4096 + 2048);                                       \
      }                                                                                                 \
    }                                                                                                   \
  } while (0)
#define READ_Y(DST, NH, SB)                                                                             \
  do {                                                                                                  \
    if constexpr (!TN) {                                                                                \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                   \
        DST[j * 2] = *(const bf16x8_t*)((SB) + offY + (2 * (NH) + j) * 2048);                           \
        DST[j * 2 + 1] = *(const bf16x8_t*)((SB) + offY + (2 * (NH) + j) * 2048 + 1024);                \
      }                                                                                                 \
    } else {                                                                                            \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                   \
        const unsigned a__ = ldsbase + (unsigned)((SB) - smem) + trY + (((wn * 2 + j) ^ swY) << 5);     \
        BL_TR(DST##2[j * 4 + 0], a__, (NH) * 16384);                                                    \
        BL_TR(DST##2[j * 4 + 1], a__, (NH) * 16384 + 4096);                                             \
        BL_TR(DST##2[j * 4 + 2], a__, (NH) * 16384 + 8192);                                             \
        BL_TR(DST##2[j * 4 + 3], a__, (NH) * 16384 + 8192 + 4096);                                      \
      }                                                                                                 \
    }                                                                                                   \
  } while (0)
// TN fragments: DST2[f * 4 + ks * 2 + half] (8 bytes each); operand ks of fragment f = {[f*4 + 2ks], [f*4 + 2ks + 1]}
#define BL_FRAG(R2, F, KS)                                                                              \
  __builtin_bit_cast(bf16x8_t, ((u32x4_t){R2[(F) * 4 + 2 * (KS)][0], R2[(F) * 4 + 2 * (KS)][1],         \
                                          R2[(F) * 4 + 2 * (KS) + 1][0], R2[(F) * 4 + 2 * (KS) + 1][1]}))
#define MMA(XR, YR, MH, NH)                                                                             \
  do {                                                                                                  \
    if constexpr (TN) {                                                                                 \
      _Pragma("unroll") for (int q = 0; q < 16; ++q) BL_PIN(XR##2[q]);                                  \
      _Pragma("unroll") for (int q = 0; q < 8; ++q) BL_PIN(YR##2[q]);                                   \
    }                                                                                                   \
    __builtin_amdgcn_s_setprio(1);                                                                      \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                    \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                     \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                 \
          if constexpr (TN)                                                                             \
            acc[2 * (NH) + j][4 * (MH) + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                  \
                BL_FRAG(YR##2, j, ks), BL_FRAG(XR##2, i, ks), acc[2 * (NH) + j][4 * (MH) + i], 0, 0, 0); \
          else                                                                                          \
            acc[2 * (NH) + j][4 * (MH) + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                  \
                YR[j * 2 + ks], XR[i * 2 + ks], acc[2 * (NH) + j][4 * (MH) + i], 0, 0, 0);              \
        }                                                                                               \
    __builtin_amdgcn_s_setprio(0);                                                                      \
  } while (0)
// (the timing-only variants of these four macros — no barrier / no wait / no issue / no reads — are generated into a
//  patched copy of this file by tools/micro/gemm_loop_experiments.py; nothing here is conditional)
#define BAR()                                   \
  do {                                          \
    __builtin_amdgcn_s_barrier();               \
    __builtin_amdgcn_sched_barrier(0);          \
  } while (0)
#define WAIT_VM8() asm volatile("s_waitcnt vmcnt(8)" ::: "memory")
#define WAIT_VM10_LGKM() asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory")
#define WAIT_LGKM() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
  // H(p+6) for phase q of K-tile T:  q=0 → X1(T+1)   q=1 → Y0(T+2)   q=2 → X0(T+2)   q=3 → Y1(T+2)
// the fragment reads go first, the LDS-DMA issue second: the ≈ 80 cycles each piece takes to issue cover the reads' latency
// instead of preceding it (+1.5–2.3 % on every shape, same box A/B). Tried and rejected: moving one of the two pieces between
// the two k-steps of the wave's next MFMA segment (to thin out the burst of 8 pieces per segment): −3 %, the piece's issue
// time then stalls the MFMA stream itself.
#define ISSUE_READ(I, R) do { R; __builtin_amdgcn_sched_barrier(0); I; } while (0)
#define ISSUE_Q0(T) ISSUE_X(1, (T) + 1)
#define ISSUE_Q1(T) ISSUE_Y(0, (T) + 2)
#define ISSUE_Q2(T) ISSUE_X(0, (T) + 2)
#define ISSUE_Q3(T) ISSUE_Y(1, (T) + 2)
  // each group runs its own loop AND its own copy of the epilogue (a common epilogue after an if/else would force the
  // 128 accumulator registers of both loops into one assignment)
#define BL_EPILOGUE()                                                                                     \
  do {                                                                                                    \
    if (a_bytes_next == 0u && w_bytes_next == 0u)   /* last tile: zero-fill loads must not outlive the LDS */ \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                    \
    if (p.splitk > 1) {                                                                                   \
      long off__ = ((long)blockIdx.x * 32 * 512 + tid) * 4;                                               \
      asm volatile("" : "+v"(off__));   /* keeps the 32 slab addresses out of the tile loop's preheader (spills) */ \
      float* dst = p.slab + off__;                                                                        \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                       \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) *(f32x4_t*)(dst + (long)(i * 8 + j) * 512 * 4) = acc[i][j]; \
    } else {                                                                                              \
      int ncol__[4];                                                                                      \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                       \
        ncol__[i] = TN ? n0 + (i >> 1) * 128 + wn * 32 + (i & 1) * 16 + lg * 4 : n0 + wn * 64 + i * 16 + lg * 4; \
      epilogue_tile<EPI, 4, 8>(p, m0 + wm * 128 + l15, ncol__, m0 + 256, n0 + 256, acc);                  \
    }                                                                                                     \
  } while (0)

  // after a tile's epilogue: the next tile becomes the current one (its first two K-tiles are in LDS or in flight, its
  // first fragments in registers), the accumulators restart from zero
#define BL_ADVANCE()                                                                                      \
  do {                                                                                                    \
    vb += (int)gridDim.x;                                                                                 \
    m0 = m0_next; n0 = n0_next; Acur = Anext; Wcur = Wnext; a_bytes = a_bytes_next; w_bytes = w_bytes_next; \
    BL_NEXT_TILE();                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                         \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};            \
  } while (0)

  f32x4_t acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  bf16x8_t X[8], Ya[4], Yb[4];            // NT fragments (unused and eliminated in the TN form)
  u32x2_t X2[16], Ya2[8], Yb2[8];         // TN fragments, one 8-byte transposing read each
  char* const S0 = smem;
  char* const S1 = smem + STAGE;
  const int t0 = kt_begin;

  // ---- prologue: H(-1) = Y0(t0), H(0) = X0(t0), H(1) = Y1(t0), H(2) = X1(t0), H(3) = Y0(t0+1), H(4) = X0(t0+1),
  //      H(5) = Y1(t0+1); the first two must have landed before the first reads ----
  ISSUE_Y(0, t0); ISSUE_X(0, t0); ISSUE_Y(1, t0); ISSUE_X(1, t0); ISSUE_Y(0, t0 + 1); ISSUE_X(0, t0 + 1); ISSUE_Y(1, t0 + 1);
  asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  BAR();
  READ_Y(Ya, 0, S0);

  if (wm == 0) {
    // ============================== group A: MMA first, then issue + read the NEXT phase ==============================
    READ_X(X, 0, S0);
    WAIT_LGKM();
    BAR();
    for (;;) {
    for (int t = t0; t < nk; t += 2) {
      // K-tile t (stage 0): Y0 in Ya, Y1 → Yb
      MMA(X, Ya, 0, 0); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q0(t), READ_Y(Yb, 1, S0)); WAIT_LGKM(); BAR();
      MMA(X, Yb, 0, 1); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q1(t), READ_X(X, 1, S0));  WAIT_LGKM(); BAR();
      MMA(X, Yb, 1, 1); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q2(t), READ_Y(Yb, 0, S1)); WAIT_LGKM(); BAR();
      MMA(X, Ya, 1, 0); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q3(t), READ_X(X, 0, S1));  WAIT_LGKM(); BAR();
      // K-tile t+1 (stage 1): Y0 in Yb, Y1 → Ya
      MMA(X, Yb, 0, 0); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q0(t + 1), READ_Y(Ya, 1, S1)); WAIT_LGKM(); BAR();
      MMA(X, Ya, 0, 1); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q1(t + 1), READ_X(X, 1, S1));  WAIT_LGKM(); BAR();
      MMA(X, Ya, 1, 1); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q2(t + 1), READ_Y(Ya, 0, S0)); WAIT_LGKM(); BAR();
      MMA(X, Yb, 1, 0); WAIT_VM8(); BAR();   ISSUE_READ(ISSUE_Q3(t + 1), READ_X(X, 0, S0));  WAIT_LGKM(); BAR();
    }
    const bool more = a_bytes_next != 0u;
    BL_EPILOGUE();
    if (!more) break;
    BL_ADVANCE();
    }
    return;
  }
  // ============================== group B: issue + read THIS phase, then MMA ==============================
  WAIT_LGKM();
  BAR();
  for (;;) {
  for (int t = t0; t < nk; t += 2) {
    ISSUE_READ(ISSUE_Q0(t), READ_X(X, 0, S0));  WAIT_VM10_LGKM(); BAR();   MMA(X, Ya, 0, 0); BAR();
    ISSUE_READ(ISSUE_Q1(t), READ_Y(Yb, 1, S0)); WAIT_VM10_LGKM(); BAR();   MMA(X, Yb, 0, 1); BAR();
    ISSUE_READ(ISSUE_Q2(t), READ_X(X, 1, S0));  WAIT_VM10_LGKM(); BAR();   MMA(X, Yb, 1, 1); BAR();
    ISSUE_READ(ISSUE_Q3(t), READ_Y(Yb, 0, S1)); WAIT_VM10_LGKM(); BAR();   MMA(X, Ya, 1, 0); BAR();
    ISSUE_READ(ISSUE_Q0(t + 1), READ_X(X, 0, S1));  WAIT_VM10_LGKM(); BAR();   MMA(X, Yb, 0, 0); BAR();
    ISSUE_READ(ISSUE_Q1(t + 1), READ_Y(Ya, 1, S1)); WAIT_VM10_LGKM(); BAR();   MMA(X, Ya, 0, 1); BAR();
    ISSUE_READ(ISSUE_Q2(t + 1), READ_X(X, 1, S1));  WAIT_VM10_LGKM(); BAR();   MMA(X, Ya, 1, 1); BAR();
    ISSUE_READ(ISSUE_Q3(t + 1), READ_Y(Ya, 0, S0)); WAIT_VM10_LGKM(); BAR();   MMA(X, Yb, 1, 0); BAR();
  }
  const bool more = a_bytes_next != 0u;
  BL_EPILOGUE();
  if (!more) break;
  BL_ADVANCE();
  }
#undef BL_EPILOGUE
#undef BL_ADVANCE
#undef BL_NEXT_TILE
#undef TILE_A_OFF
#undef TILE_W_OFF
#undef ISSUE_X
#undef ISSUE_Y
#undef READ_X
#undef READ_Y
#undef BL_TR
#undef BL_PIN
#undef BL_FRAG
#undef MMA
#undef BAR
#undef WAIT_VM8
#undef WAIT_VM10_LGKM
#undef WAIT_LGKM
#undef ISSUE_READ
#undef ISSUE_Q0
#undef ISSUE_Q1
#undef ISSUE_Q2
#undef ISSUE_Q3
#endif
}

// Sum the split-K slabs of the leftover tiles and apply the fused epilogue. Same thread → (m, n) map as the 256x256
// kernels; grid = leftover tiles × 32: one block per accumulator vector (i, j) of a tile, so the slab reads are spread
// over ≥ 1024 workgroups instead of 128.
template <int EPI, bool TN = false>
__global__ __launch_bounds__(512) void gemm_splitk_reduce_kernel(GemmArgs p) {
  int tm, tn;
  const int tile_local = blockIdx.x >> 5, idx = blockIdx.x & 31, i = idx >> 3, j = idx & 7;
  lin_to_tile(p, p.tail_base + tile_local, tm, tn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3, l15 = lane & 15, lg = lane >> 4;
  f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.splitk; ++s)
    sum += *(const f32x4_t*)(p.slab + (((long)(tile_local * p.splitk + s) * 32 + idx) * 512 + tid) * 4);
  epilogue_store4<EPI>(p, tm * 256 + wm * 128 + j * 16 + l15,
                       TN ? tn * 256 + (i >> 1) * 128 + wn * 32 + (i & 1) * 16 + lg * 4 : tn * 256 + wn * 64 + i * 16 + lg * 4, sum);
}

// kernel id (gemm_plan.h) → instantiation, per entry point. The LDS attributes and the launcher's switch both walk these
// lists, and both take the LDS bytes from lds_bytes(id). The template parameters are written once, for the id and the kernel.
#define BL_RING8(X, EPI, BM, BN) X(kid(KN_RING8, BM, BN), (gemm_ring8_kernel<EPI, BM, BN, 4>))
#define BL_MID(X, EPI, MB, NB, SK) X(kid(KN_MID, MB, NB, SK), (gemm_mid_kernel<EPI, MB, NB, SK>))
#define BL_MID2(X, EPI, NT, NST) X(kid(KN_MID2, NT, NST), (gemm_mid2_kernel<EPI, NT, NST>))
#define BL_ROWS_STREAM(X, ID, EPI, NWV, SK) X(kid(ID, NWV, SK), (gemm_rows_stream_kernel<EPI, NWV, SK>))
#define BL_TILE_KERNELS(X, EPI)                                                                                       \
  X(kid(KN_GEMM128), (gemm128_kernel<EPI>)) X(kid(KN_GEMM288S), (gemm288s_kernel<EPI>))                               \
  X(kid(KN_GEMM256S), (gemm256s_kernel<EPI>)) X(kid(KN_TILE_REDUCE), (gemm_splitk_reduce_kernel<EPI>))                \
  X(kid(KN_SLAB_REDUCE), (gemm128_splitk_reduce_kernel<EPI>))                                                         \
  BL_RING8(X, EPI, 160, 128) BL_RING8(X, EPI, 128, 128) BL_RING8(X, EPI, 128, 64) BL_RING8(X, EPI, 64, 64)            \
  BL_MID(X, EPI, 2, 4, 0) BL_MID(X, EPI, 4, 4, 0) BL_MID(X, EPI, 5, 4, 0) BL_MID(X, EPI, 2, 1, 0) BL_MID(X, EPI, 4, 1, 0) \
  BL_MID(X, EPI, 5, 1, 0) BL_MID2(X, EPI, 1, 3) BL_MID2(X, EPI, 4, 3) BL_MID2(X, EPI, 2, 2)
#define BL_ROWS_KERNELS(X, EPI)                                                                                       \
  BL_ROWS_STREAM(X, KN_ROWS_STREAM, EPI, 8, 8) BL_ROWS_STREAM(X, KN_ROWS_STREAM, EPI, 6, 8)                           \
  BL_ROWS_STREAM(X, KN_ROWS_STREAM_HALVES, BL_EPI_NONE, 8, 4) BL_MID(X, EPI, 2, 4, 8) BL_MID(X, EPI, 2, 4, 2)         \
  X(kid(KN_TREE_REDUCE), (gemm_rows_tree_reduce_kernel<EPI>))
#define BL_TN_KERNELS(X, EPI) \
  X(kid(KN_GEMM256S, 1), (gemm256s_kernel<BL_EPI_F32, true>)) X(kid(KN_TILE_REDUCE, 1), (gemm_splitk_reduce_kernel<BL_EPI_F32, true>))

// bl_gemm_bf16, bl_gemm_skinny_rows_bf16, bl_gemm_tn_bf16: launch_plan (gemm_common.h) carries their plans out on these
BL_KERNEL_FAMILY(TileKernels, BL_TILE_KERNELS)
BL_KERNEL_FAMILY(RowsKernels, BL_ROWS_KERNELS)
BL_KERNEL_FAMILY(TnKernels, BL_TN_KERNELS)

}  // namespace bl_gemm_bf16_impl
using namespace bl_gemm_bf16_impl;

extern "C" int bl_gemm_last_form(void) { return gemm_last_form(); }

extern "C" int bl_gemm_bf16(const bl_gemm_desc* d, void* stream) {
  gemm_last_form() = 0;
  GemmArgs a;
  const int rc = fill_gemm_args(d, a);
  if (rc != BL_OK) return rc;
  if (d->a_norm_weight) return BL_E_ARG;   // the fused A-operand RMSNorm exists only in the skinny kernel
  const GemmPlan plan = plan_gemm(gemm_shape(a));
  return with_epilogue<ALL_EPIS>(d->epilogue, [&](auto epi) {
    return launch_plan<TileKernels<decltype(epi)::value>>(plan, a, (hipStream_t)stream);
  });
}

extern "C" int bl_gemm_skinny_rows_bf16(const bl_gemm_desc* d, void* stream) {
  gemm_last_form() = 0;
  GemmArgs a;
  const int rc = fill_gemm_args(d, a);
  if (rc != BL_OK) return rc;
  if (d->M > 128 || (d->K % 256) || d->a_norm_weight) return BL_E_SHAPE;   // the norm is its own launch: bl_rmsnorm_skinny_bf16
  if (d->out_group) return BL_E_ARG;
  const char* e_on = getenv("BL_ROWS_STREAM");   // read per call: BL_ROWS_STREAM=0 switches the rows-stream form off (A/B)
  const GemmPlan plan = plan_rows(gemm_shape(a, e_on ? atoi(e_on) != 0 : true));
  return with_epilogue<SKINNY_EPIS>(d->epilogue, [&](auto epi) {
    return launch_plan<RowsKernels<decltype(epi)::value>>(plan, a, (hipStream_t)stream);
  });
}

extern "C" int bl_gemm_tn_bf16(const bl_gemm_desc* d, void* stream) {
  gemm_last_form() = 0;
  if (!d || !d->A || !d->W || !d->C) return BL_E_ARG;
  if (d->epilogue != BL_EPI_F32 || d->out_group || d->a_norm_weight) return BL_E_ARG;
  if (d->M <= 0 || d->N <= 0 || d->K <= 0 || (d->M % 8) || (d->N % 8)) return BL_E_SHAPE;
  if ((d->lda % 8) || (d->ldw % 8) || (d->ldc % 4) || d->lda < d->M || d->ldw < d->N || d->ldc < d->N) return BL_E_ALIGN;
  if (!bl_aligned16(d->A) || !bl_aligned16(d->W) || (((uintptr_t)d->C) & 15)) return BL_E_ALIGN;
  // byte offsets inside the kernel are 32-bit (buffer addressing)
  if ((long)d->K * d->lda * 2 >= (1L << 31) || (long)d->K * d->ldw * 2 >= (1L << 31)) return BL_E_SHAPE;
  GemmArgs a = {};
  a.A = d->A; a.W = d->W; a.C = d->C;
  a.lda = d->lda; a.ldw = d->ldw; a.ldc = d->ldc;
  a.M = d->M; a.N = d->N; a.K = d->K;
  a.tail_base = -1;
  a.slab = (float*)d->workspace; a.slab_bytes = d->workspace_bytes; a.splitk = 1;
  return launch_plan<TnKernels<BL_EPI_F32>>(plan_gemm_tn(gemm_shape(a)), a, (hipStream_t)stream);
}
