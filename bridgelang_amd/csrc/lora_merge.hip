// lora_merge.hip — merge LoRA adapters into a packed GEMM weight on the device (PEFT `merge_and_unload()`,
// vla-scripts/finetune.py:331-341):   W'[n, k] = bf16(W[n, k] + Σ_r bf16(s·B[n, r]) · A[r, k])
// read from and written to the fragment-major layout [n/16, k/32, 64, 8] of bl_pack_weight_bf16 (training/lora.py::
// merged_reference is the definition). HBM-bound: every weight byte is read once and written once.
//
// Mapping. A fragment (nt, ks) is 16 rows x 32 columns; lane l owns row n = 16·nt + (l & 15) and the eight consecutive
// columns k = 32·ks + 8·(l >> 4) + e. Δᵀ is what the MFMA computes: D[i][n] = Σ_r Aᵀ[i][r] · sB[n][r], so the accumulator's
// column (lane & 15) is the lane's own n and its rows 4·(l >> 4) + reg are k indices. Two MFMAs per 32 adapter ranks cover
// the fragment's 32 columns, and WHICH k sits behind MFMA row i is chosen so that no value has to change lane:
//     MFMA #1, row i  ->  k offset 8·(i >> 2) + (i & 3)          (lane group g, reg j: offset 8g + j)
//     MFMA #2, row i  ->  k offset 8·(i >> 2) + 4 + (i & 3)      (lane group g, reg j: offset 8g + 4 + j)
// The B operand of both is lane l's own 16 bytes of bf16(s·B)'s row n (ranks 8·(l >> 4) …). The A operand is a column of A
// (eight ranks of one k): A is transposed once per work item through LDS.
//
// Work item = four adjacent k-strips (one per wave) x up to LM_NTB consecutive 16-row tiles. The workgroup stages Aᵀ of its
// 128 columns in LDS and every wave takes its strip's A operands into registers. The same LDS then carries bf16(s·B) of
// LM_TB row tiles at a time — read from global memory once per workgroup in whole rows, scaled once, shared by the four
// waves (each lane's own B operand straight from global memory is a 16-row gather: 64 cache lines per wave load, which
// held the first version of this kernel at 0.57 x the copy rate). Per tile: one 16-byte load of W, requested one block
// ahead together with that block's B rows, 2 MFMAs per 32 ranks, one 16-byte store. A fused group whose
// members' rows are stacked (q ‖ k ‖ v) visits only the member's own rank block: the off-block entries of B are zeros by
// construction (bl_lora_block_mask_f32), and adding exact zeros changes no bit. No atomics, no workspace.
#include "bl_common.h"

namespace {

constexpr int LM_NTB = 16;         // 16-row tiles per work item
constexpr int LM_TB_MAX = 4;       // row tiles per B block (2 beyond 64 ranks, where the A operands take 32 registers); two blocks'
                                   // loads are held in registers: the next one is in flight
constexpr int LM_MAX_R = 128;      // widest rank span of one row: its A operands stay in registers (two interleaved members of rank 64)
constexpr int LM_GRID = 768;       // 256 CUs x 3 workgroups (LDS-limited) of the grid-stride loop

struct LoraMergeEntry {            // one adapter; mirrors _lib.LoraMergeDesc
  const uint16_t* w;
  const uint16_t* A;
  const uint16_t* B;
  uint16_t* out;
  float scale;
  int32_t n, k, R, rp, members, interleave, n_items;
  int64_t first_item;
};

struct LmShape { int quads, meff, tpm, bpm, span; };

// The decomposition shared by host and device (train_ops.lora_merge_items restates it for the batched table).
__host__ __device__ inline LmShape lm_shape(int n, int k, int R, int rp, int members, int interleave) {
  LmShape s;
  const int tiles = n >> 4;
  const bool skip = !interleave && members > 1 && (n % (16 * members)) == 0;   // stacked members, whole tiles each
  s.meff = skip ? members : 1;
  s.span = skip ? rp : R;
  s.tpm = tiles / s.meff;
  s.bpm = (s.tpm + LM_NTB - 1) / LM_NTB;
  s.quads = ((k >> 5) + 3) >> 2;
  return s;
}

template <int NCH>
__device__ __forceinline__ void lm_item(const LoraMergeEntry& e, const LmShape& sh, int item, uint16_t* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int SPAN = NCH * 32, PR = SPAN + 8;                  // LDS row pitch in elements (16-byte multiple)
  constexpr int LM_TB = NCH <= 2 ? LM_TB_MAX : LM_TB_MAX / 2;
  constexpr int CPR = SPAN / 8;                                  // 16-byte chunks per row of the B tile
  constexpr int BPT = (LM_TB * 16 * CPR + 255) / 256;            // B chunks per thread and tile block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int KS = e.k >> 5;
  const int q = item % sh.quads, blk = item / sh.quads, mj = blk / sh.bpm, b = blk - mj * sh.bpm;
  const int nt0 = mj * sh.tpm + b * LM_NTB, nt1 = min(nt0 + LM_NTB, (mj + 1) * sh.tpm);
  const int r0 = sh.meff > 1 ? mj * e.rp : 0;
  const int ks = q * 4 + wave;
  const bool active = ks < KS;                                   // a ragged last quad: the wave still stages and syncs

  // one tile block's global loads: the wave's weight fragments and the thread's share of the block's B rows
  auto request = [&](int nt, u32x4_t* wv, u32x4_t* bv) {
    const int tiles = min(LM_TB, nt1 - nt);
    if (active) {
#pragma unroll
      for (int u = 0; u < LM_TB; ++u)
        if (u < tiles) wv[u] = *(const u32x4_t*)(e.w + (((long)(nt + u) * KS + ks) * 64 + lane) * 8);
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int p = tid + 256 * u, row = p / CPR, ch = p - row * CPR;
      if (row < tiles * 16) bv[u] = *(const u32x4_t*)(e.B + (long)(nt * 16 + row) * e.R + r0 + ch * 8);
    }
  };
  u32x4_t wv[LM_TB], bv[BPT], wn[LM_TB], bn[BPT];
  request(nt0, wv, bv);                                          // in flight while Aᵀ is staged

  __syncthreads();                                               // the previous item's operand reads are done
  // Aᵀ of columns [128q, 128q + 128) ∩ [0, k): 16 lanes take 16 ranks of one 8-column chunk (their 2-byte LDS stores share
  // dwords and spread over the banks), the four lane groups four chunks of a row's 64 contiguous bytes
  for (int p = tid; p < SPAN * 16; p += 256) {
    const int grp = p >> 6, r = (grp % (SPAN / 16)) * 16 + l15, c = (grp / (SPAN / 16)) * 4 + g, kcol = q * 128 + c * 8;
    if (kcol < e.k) {
      const u32x4_t v = *(const u32x4_t*)(e.A + (long)(r0 + r) * e.k + kcol);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lds[(c * 8 + 2 * i) * PR + r] = (uint16_t)(v[i] & 0xffffu);
        lds[(c * 8 + 2 * i + 1) * PR + r] = (uint16_t)(v[i] >> 16);
      }
    }
  }
  __syncthreads();

  bf16x8_t a1[NCH], a2[NCH];
  if (active) {
    const int koff = 8 * (l15 >> 2) + (l15 & 3);
    const uint16_t* row1 = lds + (wave * 32 + koff) * PR + 8 * g;
    const uint16_t* row2 = row1 + 4 * PR;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      a1[c] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(row1 + 32 * c));
      a2[c] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(row2 + 32 * c));
    }
  }
  const float s = e.scale;
  for (int nt = nt0; nt < nt1; nt += LM_TB) {                    // LM_TB row tiles at a time: bf16(s·B) of their rows through LDS
    const int tiles = min(LM_TB, nt1 - nt);
    __syncthreads();                                             // A operands are in registers / the previous block is consumed
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int p = tid + 256 * u, row = p / CPR, ch = p - row * CPR;
      if (row < tiles * 16) {
        u32x4_t sb;
#pragma unroll
        for (int i = 0; i < 4; ++i) sb[i] = pack2bf(bflo(bv[u][i]) * s, bfhi(bv[u][i]) * s);   // bf16(s·B), as be_pack(scale = s)
        *(u32x4_t*)(lds + row * PR + ch * 8) = sb;
      }
    }
    __syncthreads();
    const bool more = nt + LM_TB < nt1;
    if (more) request(nt + LM_TB, wn, bn);                       // the next block's loads fly during this block's MFMAs and stores
    if (active) {
#pragma unroll
      for (int u = 0; u < LM_TB; ++u) {
        if (u >= tiles) break;
        const uint16_t* brow = lds + (u * 16 + l15) * PR + 8 * g;
        f32x4_t d1 = {0.f, 0.f, 0.f, 0.f}, d2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(brow + 32 * c));
          d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[c], bf, d1, 0, 0, 0);
          d2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2[c], bf, d2, 0, 0, 0);
        }
        const float d[8] = {d1[0], d1[1], d1[2], d1[3], d2[0], d2[1], d2[2], d2[3]};
        u32x4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t wi = wv[u][i];
          const uint32_t m = pack2bf(bflo(wi) + d[2 * i], bfhi(wi) + d[2 * i + 1]);
          // an element whose update is exactly zero keeps its bits (−0 stays −0): B = 0 or s = 0 is the identity bit for bit
          const uint32_t lo = d[2 * i] == 0.f ? (wi & 0xffffu) : (m & 0xffffu);
          const uint32_t hi = d[2 * i + 1] == 0.f ? (wi & 0xffff0000u) : (m & 0xffff0000u);
          o[i] = lo | hi;
        }
        *(u32x4_t*)(e.out + (((long)(nt + u) * KS + ks) * 64 + lane) * 8) = o;
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < LM_TB; ++u) wv[u] = wn[u];
#pragma unroll
      for (int u = 0; u < BPT; ++u) bv[u] = bn[u];
    }
  }
#endif
}

// table != nullptr: the batched form (each workgroup finds the group of its item by binary search over first_item);
// table == nullptr: `one` is the only group. Same device code, same accumulation order: bit-identical results.
__global__ __launch_bounds__(256, 3) void lora_merge_kernel(const LoraMergeEntry* table, int n_groups, LoraMergeEntry one) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[128 * (LM_MAX_R + 8)];
  const long total = table ? table[n_groups - 1].first_item + table[n_groups - 1].n_items : (long)one.n_items;
  for (long it = blockIdx.x; it < total; it += gridDim.x) {
    LoraMergeEntry e = one;
    if (table) {
      int lo = 0, hi = n_groups - 1;                             // last group whose first item is <= it
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_item <= it) lo = mid; else hi = mid - 1;
      }
      e = table[lo];
    }
    const LmShape sh = lm_shape(e.n, e.k, e.R, e.rp, e.members, e.interleave);
    const int item = (int)(it - e.first_item);
    switch (sh.span >> 5) {
      case 1: lm_item<1>(e, sh, item, lds); break;
      case 2: lm_item<2>(e, sh, item, lds); break;
      case 3: lm_item<3>(e, sh, item, lds); break;
      case 4: lm_item<4>(e, sh, item, lds); break;
      default: break;
    }
  }
}

}  // namespace

extern "C" int bl_lora_merge_bf16(const bl_bf16* w_packed, const bl_bf16* A, const bl_bf16* B, float scale, bl_bf16* out_packed,
                                  int64_t n, int64_t k, int32_t R, int32_t rp, int32_t members, int32_t interleave, void* stream) {
  if (!w_packed || !A || !B || !out_packed) return BL_E_ARG;
  if (n <= 0 || k <= 0 || R <= 0 || rp <= 0 || members <= 0 || (n % 16) || (k % 32) || (R % 32) || (rp % 32) || R != rp * members ||
      (n % members) || n > (1 << 24) || k > (1 << 24))
    return BL_E_SHAPE;
  const LmShape sh = lm_shape((int)n, (int)k, R, rp, members, interleave);
  if (sh.span > LM_MAX_R) return BL_E_SHAPE;
  if (!bl_aligned16(w_packed) || !bl_aligned16(A) || !bl_aligned16(B) || !bl_aligned16(out_packed)) return BL_E_ALIGN;
  const uintptr_t wb = (uintptr_t)w_packed, ob = (uintptr_t)out_packed, bytes = (uintptr_t)n * (uintptr_t)k * 2u;
  if (wb < ob + bytes && ob < wb + bytes) return BL_E_ARG;      // every fragment is read after others were written: no aliasing
  const long items = (long)sh.quads * sh.meff * sh.bpm;
  if (items > 0x7fffffffL) return BL_E_SHAPE;
  LoraMergeEntry e = {w_packed, A, B, out_packed, scale, (int32_t)n, (int32_t)k, R, rp, members, interleave ? 1 : 0, (int32_t)items, 0};
  const int grid = (int)(items < LM_GRID ? items : LM_GRID);
  hipLaunchKernelGGL(lora_merge_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const LoraMergeEntry*)nullptr, 0, e);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_lora_merge_batched_bf16(const void* table, int32_t n_groups, void* stream) {
  if (!table) return BL_E_ARG;
  if (n_groups <= 0) return BL_E_SHAPE;
  if (((uintptr_t)table) & 7u) return BL_E_ALIGN;
  LoraMergeEntry none = {};
  hipLaunchKernelGGL(lora_merge_kernel, dim3(LM_GRID), dim3(256), 0, (hipStream_t)stream, (const LoraMergeEntry*)table, n_groups, none);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
