// beam.hip — the two device steps of beam search over the action tokens (bridgelang_amd/beam.py is the specification).
//
// bl_beam_step_f32: for every prompt (a group of W consecutive logits rows, W <= 16) the W best of its W × n candidate
// continuations in the total order "score descending, flat index j·n + i ascending", bit-identical to beam.py::beam_step:
// tokens, parents, both integers of the weight pair and the fp32 score. Two launches of 1024-thread workgroups:
//   1. one workgroup per ROW j (all rows of all prompts side by side: this is where the 32 064 exponentials are): the
//      maximum m_j (bl_argmax_f32's order), then total_j = Σ rint(exp_spec(l − m_j)·2^30) — the sampler's own exp_spec /
//      weight_of (sample_spec.h), exact integers — left in the row's wt pair for the second launch
//   then one workgroup per PROMPT: lz_j = log_spec(fp32(total_j)·2^-30), and
//   2. every candidate's score c = ((s_j + (l − m_j)) − lz_j), each operation rounded alone, as an integer key; thread t
//      owns the columns 4t … 4t+3 (+ 4096·k) of all W rows (16-byte loads) and keeps the best of them
//   3. W rounds: a block-wide arg-best over the threads' holders is the next survivor; only the owner's candidates have
//      to be ranked again ("strictly after the pick"), which the whole block does — one 16-byte load per thread — and
//      hands the owner its new holder. Nothing is sorted and nothing is staged: the rows stay in L2.
// A holder starts as (INT_MIN, INT_MAX) and no float has the key INT_MIN, so with W <= n every round picks a real
// candidate: parents are in [0, W) and tokens in the range by construction, whatever the logits hold (NaN included).
//
// bl_beam_reorder_kv_bf16: beam slot k of every prompt takes the generated cache rows of slot parents[k] of the same
// prompt, in place, in every cache of a device table of base pointers (the K and V caches of all layers: ONE launch per
// decode step). A parent may have no child, several, or be overwritten by another slot's child, so a workgroup owns ALL
// W slots of its (cache, prompt, head, cache row): it loads them, barriers, then stores. 16-byte loads and stores only.
#include "bl_common.h"
#include "sample_spec.h"

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / BL_WAVE;
constexpr int kMaxBeams = 16;
constexpr int kColsPerSweep = kThreads * 4;                       // columns one sweep of 16-byte loads covers
constexpr int kSweeps = (kSpecMaxN + kColsPerSweep - 1) / kColsPerSweep;      // sweeps the widest row takes
static_assert(kMaxBeams * kSweeps <= kThreads, "step 3 ranks an owner's candidates with one 16-byte load per thread");

typedef unsigned long long u64;

// ln x for x >= 1: beam.py::log_spec operation for operation (contraction off: every multiply and add rounds alone)
__device__ __forceinline__ float log_spec(float x) {
#pragma clang fp contract(off)
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  int e = (int)(b >> 23) - 127;
  float m = __builtin_bit_cast(float, (b & 0x007fffffu) | 0x3f800000u);
  const bool big = m > 1.41421354f;
  m = big ? m * 0.5f : m;
  e += big;
  const float ef = (float)e;
  const float f = m - 1.0f;
  const float d = f + 2.0f;
  const float s = f / d;
  const float z = s * s;
  float p = (float)(1.0 / 9);
  p = p * z; p = p + (float)(1.0 / 7);
  p = p * z; p = p + (float)(1.0 / 5);
  p = p * z; p = p + (float)(1.0 / 3);
  p = p * z;
  const float t = p * s;
  const float r = t + s;
  const float lm = r + r;
  const float lo = ef * -2.12194440e-4f;
  const float a = lo + lm;
  const float hi = ef * 0.693359375f;
  return hi + a;
}

// the score of candidate l on a row with (s, m, lz), and its key in bl_argmax_f32's order
__device__ __forceinline__ float cand_score(float l, float s, float m, float lz) {
#pragma clang fp contract(off)
  const float d = l - m;
  const float c = s + d;
  return c - lz;
}

// the best (key, index) of the block, returned to every thread; sk / si: kWaves slots of LDS; safe to call back to back
__device__ __forceinline__ void block_best(int& bk, int& bi, int* sk, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) argmax_take(__shfl_xor(bk, o, 64), __shfl_xor(bi, o, 64), bk, bi);
  __syncthreads();                                                // earlier readers of sk / si are done
  if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = bk; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bk = sk[0]; bi = si[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) argmax_take(sk[w], si[w], bk, bi);
}

// 1. One workgroup per ROW: its maximum and integer total, left in the row's own wt pair as (total, bits of the maximum)
// for the step kernel of the same call, which reads all W pairs of its prompt before it writes any.
__global__ __launch_bounds__(kThreads) void beam_rows_kernel(const float* logits, long ld, int n, int base, int64_t* wt) {
  __shared__ int sk[kWaves], si[kWaves];
  __shared__ u64 red[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (long)blockIdx.x * ld + base;
  f32x4_t q[kSweeps];                                             // the thread's columns 4t … 4t+3 (+ 4096·k): read once
  int bk = (int)0x80000000, bi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < kSweeps; ++k) {
    const int i = tid * 4 + k * kColsPerSweep;
    if (i < n) {                                                  // n % 4 == 0 (host check): never past column n
      q[k] = *(const f32x4_t*)(row + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) argmax_take_next(argmax_key(q[k][e]), i + e, bk, bi);
    }
  }
  block_best(bk, bi, sk, si);
  const float mx = argmax_value(bk);                              // either zero as +0: l − mx is the same
  u64 part = 0;
#pragma unroll
  for (int k = 0; k < kSweeps; ++k)
    if (tid * 4 + k * kColsPerSweep < n) {
#pragma unroll
      for (int e = 0; e < 4; ++e) part += weight_of(q[k][e], mx, 1.0f);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += (u64)__shfl_xor((long long)part, o, 64);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (tid == 0) {
    u64 total = 0;
    for (int w = 0; w < kWaves; ++w) total += red[w];
    wt[2 * (long)blockIdx.x] = (int64_t)total;
    wt[2 * (long)blockIdx.x + 1] = (int64_t)__builtin_bit_cast(uint32_t, mx);
  }
}

__global__ __launch_bounds__(kThreads) void beam_step_kernel(const float* logits, long ld, int W, int n, int base,
                                                             const float* scores_in, int64_t* tokens, int32_t* parents,
                                                             int64_t* wt, float* scores_out) {
  __shared__ int sk[kWaves], si[kWaves];
  __shared__ float s_s[kMaxBeams], s_m[kMaxBeams], s_lz[kMaxBeams];
  __shared__ u64 s_total[kMaxBeams];
  __shared__ int s_pick[kMaxBeams];

  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * W;
  const float* src = logits + row0 * ld + base;                   // row j of the prompt: src + j·ld, n columns

  // the rows' totals and maxima (beam_rows_kernel) → lz; every input of the prompt is read before any output is written
  if (tid < W) {
    const u64 total = (u64)wt[2 * (row0 + tid)];
    s_total[tid] = total;
    s_m[tid] = __builtin_bit_cast(float, (uint32_t)wt[2 * (row0 + tid) + 1]);
    s_lz[tid] = log_spec((float)total * 9.31322574615478515625e-10f);      // · 2^-30: exact
    s_s[tid] = scores_in[row0 + tid];
  }
  __syncthreads();

  // 2. every thread's best candidate among its columns of all W rows; it walks them in ascending flat index
  int hk = (int)0x80000000, hi = 0x7fffffff;
  for (int j = 0; j < W; ++j) {
    const float* row = src + (long)j * ld;
    const float s = s_s[j], m = s_m[j], lz = s_lz[j];
    for (int i = tid * 4; i < n; i += kColsPerSweep) {
      const f32x4_t q = *(const f32x4_t*)(row + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) argmax_take_next(argmax_key(cand_score(q[e], s, m, lz)), j * n + i + e, hk, hi);
    }
  }

  // 3. W rounds of "the best holder of the block"; the owner's candidates behind the pick are ranked again by the block
  const int sweeps = (n + kColsPerSweep - 1) / kColsPerSweep;
  for (int k = 0; k < W; ++k) {
    int pk = hk, pi = hi;
    block_best(pk, pi, sk, si);
    if (tid == 0) s_pick[k] = pi;
    if (k + 1 == W) break;
    const int owner = ((pi % n) % kColsPerSweep) >> 2;            // the thread whose columns hold the pick
    int rk = (int)0x80000000, ri = 0x7fffffff;
    if (tid < W * sweeps) {
      const int j = tid / sweeps, i = owner * 4 + (tid % sweeps) * kColsPerSweep;
      if (i < n) {
        const f32x4_t q = *(const f32x4_t*)(src + (long)j * ld + i);
        const float s = s_s[j], m = s_m[j], lz = s_lz[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ck = argmax_key(cand_score(q[e], s, m, lz)), ci = j * n + i + e;
          const bool after = (ck < pk) | ((ck == pk) & (ci > pi));
          if (after) argmax_take_next(ck, ci, rk, ri);
        }
      }
    }
    block_best(rk, ri, sk, si);
    if (tid == owner) { hk = rk; hi = ri; }
  }
  __syncthreads();

  // the survivors: W <= n keeps every pick a real candidate; the clamp holds the indices in range even if it were not
  if (tid < W) {
    int p = s_pick[tid];
    p = p < 0 ? 0 : (p >= W * n ? W * n - 1 : p);
    const int j = p / n, i = p % n;
    const float l = src[(long)j * ld + i];
    tokens[row0 + tid] = (int64_t)base + i;
    parents[row0 + tid] = j;
    wt[2 * (row0 + tid)] = (int64_t)weight_of(l, s_m[j], 1.0f);
    wt[2 * (row0 + tid) + 1] = (int64_t)s_total[j];
    scores_out[row0 + tid] = cand_score(l, s_s[j], s_m[j], s_lz[j]);
  }
}

// One workgroup: cache blockIdx.z, prompt blockIdx.y, (head, cache row) blockIdx.x; its W slots × hd8 16-byte pieces.
constexpr int kReorderThreads = 256, kReorderPieces = 2;          // 512 pieces: 16 slots of head_dim 256

__global__ __launch_bounds__(kReorderThreads) void beam_reorder_kernel(bl_bf16* const* caches, int W, int H, int cache_len,
                                                                        int hd8, const int32_t* parents, int row0,
                                                                        const int32_t* row0_dev, int n_rows) {
  bl_bf16* cache = caches[blockIdx.z];
  const int g = blockIdx.y, h = blockIdx.x / n_rows, r = blockIdx.x % n_rows;
  u32x4_t held[kReorderPieces];
  long dst[kReorderPieces];
#pragma unroll
  for (int it = 0; it < kReorderPieces; ++it) {
    const int piece = threadIdx.x + it * kReorderThreads;
    dst[it] = -1;
    if (piece >= W * hd8) continue;
    const int k = piece / hd8, c = piece % hd8;
    int p = parents[g * W + k];
    p = (unsigned)p < (unsigned)W ? p : k;                        // a parent outside the prompt's slots: the slot keeps its rows
    const int to = (row0_dev ? row0_dev[g * W + k] : row0) + r, from = (row0_dev ? row0_dev[g * W + p] : row0) + r;
    if (to < 0 || to >= cache_len || from < 0 || from >= cache_len) continue;      // rows outside the cache: nothing moves
    held[it] = *(const u32x4_t*)(cache + ((((long)(g * W + p) * H + h) * cache_len + from) * hd8 + c) * 8);
    dst[it] = ((((long)(g * W + k) * H + h) * cache_len + to) * hd8 + c) * 8;
  }
  __syncthreads();                                                // every slot of this set is in registers
#pragma unroll
  for (int it = 0; it < kReorderPieces; ++it)
    if (dst[it] >= 0) *(u32x4_t*)(cache + dst[it]) = held[it];
}

}  // namespace

extern "C" int bl_beam_step_f32(const float* logits, int64_t ld, int32_t groups, int32_t W, int32_t n, const float* scores_in,
                                int64_t* tokens, int32_t* parents, int64_t* wt, float* scores_out, int32_t vocab_first,
                                int32_t vocab_count, void* stream) {
  if (!logits || !scores_in || !tokens || !parents || !wt || !scores_out) return BL_E_ARG;
  if (groups <= 0 || W < 1 || W > kMaxBeams || n <= 0 || (ld % 4) || ld < n || vocab_first < 0 || vocab_count <= 0 ||
      (vocab_first % 4) || (vocab_count % 4) || (int64_t)vocab_first + vocab_count > n || vocab_count > kSpecMaxN ||
      W > vocab_count)
    return BL_E_SHAPE;
  if (!bl_aligned16(logits) || (((uintptr_t)tokens | (uintptr_t)wt) & 7) ||
      (((uintptr_t)scores_in | (uintptr_t)scores_out | (uintptr_t)parents) & 3))
    return BL_E_ALIGN;
  hipLaunchKernelGGL(beam_rows_kernel, dim3(groups * W), dim3(kThreads), 0, (hipStream_t)stream, logits, (long)ld, vocab_count,
                     vocab_first, wt);
  BL_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_step_kernel, dim3(groups), dim3(kThreads), 0, (hipStream_t)stream, logits, (long)ld, W, vocab_count,
                     vocab_first, scores_in, tokens, parents, wt, scores_out);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_beam_reorder_kv_bf16(bl_bf16* const* caches, int32_t n_caches, int32_t rows, int32_t W, int32_t H,
                                       int32_t cache_len, int32_t head_dim, const int32_t* parents, int32_t row0,
                                       const int32_t* row0_dev, int32_t n_rows, void* stream) {
  if (!caches || !parents) return BL_E_ARG;
  if (n_caches <= 0 || n_caches > 65535 || rows <= 0 || W < 1 || W > kMaxBeams || (rows % W) || rows / W > 65535 || H <= 0 ||
      cache_len <= 0 || head_dim <= 0 || (head_dim % 8) || W * (head_dim / 8) > kReorderThreads * kReorderPieces || n_rows <= 0 ||
      n_rows > cache_len || (int64_t)H * n_rows > 0x7fffffff)
    return BL_E_SHAPE;
  if (!row0_dev && (row0 < 0 || (int64_t)row0 + n_rows > cache_len)) return BL_E_SHAPE;
  if ((((uintptr_t)caches) & 7) || (((uintptr_t)parents | (uintptr_t)row0_dev) & 3)) return BL_E_ALIGN;
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(H * n_rows, rows / W, n_caches), dim3(kReorderThreads), 0, (hipStream_t)stream,
                     caches, W, H, cache_len, head_dim / 8, parents, row0, row0_dev, n_rows);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
