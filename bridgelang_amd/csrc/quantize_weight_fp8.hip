// quantize_weight_fp8.hip — packed bf16 GEMM weight → packed e4m3 weight + per-channel scales, on the device and in place of
// what the output buffers held: the W8 operand of bl_gemm_fp8 derived from the fragment-major image [n/16, k/32, 64, 8] that
// bl_pack_weight_bf16 (and bl_lora_merge_bf16) writes, without a row-major copy. Runs with every refresh of LoRA-adapted
// weights (training/lora.py::LoraAdapters.enable_fp8). HBM-bound: 2 bytes read and 1 byte written per weight.
//
// Arithmetic: the quantiser specification above FP8_AMAX_MIN in gemm_fp8.hip (tests/fp8_ref64.py::quantize_spec), per output
// channel n: amax = max |w|; live = amax >= 2^-100; scale = amax / 448 and inv = 448 / amax (__fdiv_rn) when live, else
// scale = inv = 1; code = e4m3_rne_sat(fl32(w·inv)) through v_cvt_pk_fp8_f32, as quantize_rows_fp8_kernel.
//
// Layout. A bf16 fragment (nt, ks) is 16 rows x 32 columns: lane l holds row 16·nt + (l & 15), columns 32·ks + 8·(l >> 4) + 0…7.
// An e4m3 fragment (nt, ks8) is 16 rows x 64 columns: lane L holds row 16·nt + (L & 15), columns 64·ks8 + 16·(L >> 4) + 0…15.
// Those sixteen columns are the 16 bytes of bf16 fragment (nt, 2·ks8 + (L >> 5)), lane (L & 15) + 32·((L >> 4) & 1), followed
// by the 16 bytes of the lane 16 above it: one task = two 16-byte loads, eight conversions, one 16-byte store, and no value
// changes lane.
//
// Work item = one 16-row tile: 32·k contiguous bytes of bf16, k tasks, taken by one workgroup of 512 threads (task t = tid +
// 512·j; 512 is a multiple of 64, so a thread's tasks all belong to ONE row, 16·nt + (tid & 15)). The first WQ_RES tasks of a
// thread stay in registers between the amax pass and the conversion (k <= 4096: the whole tile, which then crosses the memory
// system once); the tasks beyond them are read again in the conversion pass, from L2 / the memory-side cache the workgroup has
// just pulled them through. A row's amax is the maximum over the lanes that share l & 15 (two shuffles) and over the eight
// waves (LDS): a maximum is the same in any order. Two workgroups per CU: one's loads fly during the other's conversion.
// No atomics, no workspace, every output byte of the n·k codes and n scales is written.
#include "bl_common.h"

namespace {

constexpr int WQ_THREADS = 512;
constexpr int WQ_RES = 8;          // resident tasks per thread (8 VGPRs each): k <= 4096 entirely
constexpr int WQ_GRID = 512;       // 256 CUs x 2 workgroups of the grid-stride loop
constexpr float WQ_AMAX_MIN = 0x1p-100f;   // FP8_AMAX_MIN of gemm_fp8.hip

struct WeightQuantEntry {          // one weight; mirrors _lib.WeightQuantDesc
  const uint16_t* w;               // packed bf16 [n/16, k/32, 64, 8]
  uint8_t* w8;                     // packed e4m3 [n/16, k/64, 64, 16]
  float* scale;                    // [n]
  int32_t n, k, n_items, pad;      // n_items = n / 16 (train_ops.quantize_packed_items)
  int64_t first_item;
};

__device__ __forceinline__ float wq_amax(const u32x4_t& v, float m) {
#pragma unroll
  for (int i = 0; i < 4; ++i) m = fmaxf(m, fmaxf(fabsf(bflo(v[i])), fabsf(bfhi(v[i]))));
  return m;
}

__device__ __forceinline__ u32x4_t wq_convert(const u32x4_t& a, const u32x4_t& b, float inv) {
  u32x4_t o;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(a[2 * i]) * inv, bfhi(a[2 * i]) * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(a[2 * i + 1]) * inv, bfhi(a[2 * i + 1]) * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(b[2 * i]) * inv, bfhi(b[2 * i]) * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(b[2 * i + 1]) * inv, bfhi(b[2 * i + 1]) * inv, hi, true);
    o[i] = (uint32_t)lo;
    o[2 + i] = (uint32_t)hi;
  }
  return o;
}

__device__ __forceinline__ void wq_tile(const WeightQuantEntry& e, int nt, float* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int tid = threadIdx.x, L = tid & 63, wave = tid >> 6, l15 = tid & 15;
  const int k = e.k;
  // task t: e4m3 fragment ks8 = t >> 6, lane L. Its bf16 source: fragment 2·ks8 + (L >> 5), lanes src and src + 16
  const int src = l15 + 32 * ((L >> 4) & 1);
  const uint16_t* wt = e.w + (long)nt * k * 16 + ((L >> 5) * 64 + src) * 8;      // + ks8 · 1024 elements per task
  uint8_t* ot = e.w8 + (long)nt * k * 16 + L * 16;                                // + ks8 · 1024 bytes per task

  u32x4_t ra[WQ_RES], rb[WQ_RES];
#pragma unroll
  for (int j = 0; j < WQ_RES; ++j) {
    const int t = tid + WQ_THREADS * j;
    ra[j] = (u32x4_t){0u, 0u, 0u, 0u};
    rb[j] = (u32x4_t){0u, 0u, 0u, 0u};
    if (t < k) {
      const uint16_t* p = wt + (long)(t >> 6) * 1024;
      ra[j] = *(const u32x4_t*)p;
      rb[j] = *(const u32x4_t*)(p + 128);
    }
  }
  float amax = 0.f;
#pragma unroll 2
  for (int t = tid + WQ_THREADS * WQ_RES; t < k; t += WQ_THREADS) {               // beyond the resident part: amax only
    const uint16_t* p = wt + (long)(t >> 6) * 1024;
    const u32x4_t a = *(const u32x4_t*)p, b = *(const u32x4_t*)(p + 128);
    amax = wq_amax(b, wq_amax(a, amax));
  }
#pragma unroll
  for (int j = 0; j < WQ_RES; ++j) amax = wq_amax(rb[j], wq_amax(ra[j], amax));
  amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
  __syncthreads();                                               // the previous tile's reads of lds are done
  if (L < 16) lds[wave * 16 + L] = amax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WQ_THREADS / 64; ++w) amax = fmaxf(amax, lds[w * 16 + l15]);
  const bool live = amax >= WQ_AMAX_MIN;
  const float inv = live ? __fdiv_rn(448.0f, amax) : 1.0f;
  if (tid < 16) e.scale[nt * 16 + tid] = live ? __fdiv_rn(amax, 448.0f) : 1.0f;

#pragma unroll
  for (int j = 0; j < WQ_RES; ++j)    // keep the tile PACKED between the passes (as quantize_rows_fp8_resident_kernel)
    asm volatile("" : "+v"(ra[j][0]), "+v"(ra[j][1]), "+v"(ra[j][2]), "+v"(ra[j][3]), "+v"(rb[j][0]), "+v"(rb[j][1]), "+v"(rb[j][2]),
                 "+v"(rb[j][3]));
#pragma unroll
  for (int j = 0; j < WQ_RES; ++j) {
    const int t = tid + WQ_THREADS * j;
    if (t < k) *(u32x4_t*)(ot + (long)(t >> 6) * 1024) = wq_convert(ra[j], rb[j], inv);
  }
#pragma unroll 2
  for (int t = tid + WQ_THREADS * WQ_RES; t < k; t += WQ_THREADS) {
    const uint16_t* p = wt + (long)(t >> 6) * 1024;
    const u32x4_t a = *(const u32x4_t*)p, b = *(const u32x4_t*)(p + 128);
    *(u32x4_t*)(ot + (long)(t >> 6) * 1024) = wq_convert(a, b, inv);
  }
#endif
}

// table != nullptr: the batched form (each workgroup finds the entry of its item by binary search over first_item);
// table == nullptr: `one` is the only entry. Same device code: bit-identical results.
__global__ __launch_bounds__(WQ_THREADS, 4) void quantize_weight_fp8_packed_kernel(const WeightQuantEntry* table, int n_entries,
                                                                                   WeightQuantEntry one) {
  __shared__ float lds[(WQ_THREADS / 64) * 16];
  const long total = table ? table[n_entries - 1].first_item + table[n_entries - 1].n_items : (long)one.n_items;
  for (long it = blockIdx.x; it < total; it += gridDim.x) {
    WeightQuantEntry e = one;
    if (table) {
      int lo = 0, hi = n_entries - 1;                            // last entry whose first item is <= it
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_item <= it) lo = mid; else hi = mid - 1;
      }
      e = table[lo];
    }
    wq_tile(e, (int)(it - e.first_item), lds);
  }
}

}  // namespace

extern "C" int bl_quantize_weight_fp8_packed(const bl_bf16* w_packed, int64_t n, int64_t k, void* w8_packed, float* scale, void* stream) {
  if (!w_packed || !w8_packed || !scale) return BL_E_ARG;
  if (n <= 0 || k <= 0 || (n % 16) || (k % 128) || n > (1 << 24) || k > (1 << 24)) return BL_E_SHAPE;
  if (!bl_aligned16(w_packed) || !bl_aligned16(w8_packed) || !bl_aligned16(scale)) return BL_E_ALIGN;
  const uintptr_t wb = (uintptr_t)w_packed, wn = (uintptr_t)n * (uintptr_t)k * 2u, ob = (uintptr_t)w8_packed, on = wn / 2u,
                  sb = (uintptr_t)scale, sn = (uintptr_t)n * 4u;
  if ((wb < ob + on && ob < wb + wn) || (wb < sb + sn && sb < wb + wn) || (ob < sb + sn && sb < ob + on))
    return BL_E_ARG;                                             // a tile is read again after others were written: no aliasing
  const int items = (int)(n >> 4);
  WeightQuantEntry e = {w_packed, (uint8_t*)w8_packed, scale, (int32_t)n, (int32_t)k, items, 0, 0};
  const int grid = items < WQ_GRID ? items : WQ_GRID;
  hipLaunchKernelGGL(quantize_weight_fp8_packed_kernel, dim3(grid), dim3(WQ_THREADS), 0, (hipStream_t)stream,
                     (const WeightQuantEntry*)nullptr, 0, e);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_quantize_weight_fp8_packed_batched(const void* table, int32_t n_entries, void* stream) {
  if (!table) return BL_E_ARG;
  if (n_entries <= 0) return BL_E_SHAPE;
  if (((uintptr_t)table) & 7u) return BL_E_ALIGN;
  WeightQuantEntry none = {};
  hipLaunchKernelGGL(quantize_weight_fp8_packed_kernel, dim3(WQ_GRID), dim3(WQ_THREADS), 0, (hipStream_t)stream,
                     (const WeightQuantEntry*)table, n_entries, none);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
