// value.hip — the critic of the policy training step: a linear value head on the final-norm output (bf16 rows) and PPO's
// clipped value loss, forward + statistics (bl_value_head_f32) and backward (bl_value_head_backward_f32).
// bridgelang_amd/training/value_loss.py is the fp64 definition; these kernels are its fp32 twin to a tolerance.
//
// Conventions of policy.hip: wave64, 16-byte loads, targets[row] = token of the NEXT position, deterministic reductions in
// a fixed order, no float atomics, int return codes. The traffic is a few hundred rows of 8 KB at 7B: nothing here is tuned,
// everything is exact to the definition, the same bits on every launch, and free of host-side knowledge of the labels — the
// VALUE ROWS (level 0 "token": every valid row; level 1 "action": the first valid row of each run of group_rows rows) are
// found on the device, so a captured graph serves any labels.
//
// Forward, four launches on the stream:
//   value_mark_kernel     index[i] = candidate row or −1 (token: i = row; action: i = sequence, one wave scans its rows and
//                         takes the lowest valid one), and zeros value_rows for every row
//   value_compact_kernel  ONE workgroup packs the candidates to the front of index in ascending order (ballot prefix per
//                         wave, the four waves in order, chunks of 256 in order), −1 behind them, and writes count
//   value_rows_kernel     one wave per list entry: v = Σ_k hn[r,k]·w[k] + b. Lane L takes the 8 columns [512·s + 8·L, + 8)
//                         of step s = 0, 1, …: ONE chain acc = fma(h, w, acc) in ascending k per lane (a bf16·bf16
//                         product is exact in fp32, so only the additions round), then wave_sum (6 xor-butterfly levels),
//                         then + b. Then the loss terms of the row into value_rows[r] = (v, l, clipped, dv).
//   value_stats_kernel    ONE workgroup, two passes over the list: thread t sums entries t, t + 256, … in ascending order,
//                         wave_sum, the four waves in order → the means; then Σ(e − ē)² and Σ(R − R̄)² the same way.
// A row that is not a value row is never loaded (hn, returns, old_values alike).
//
// Backward, two launches:
//   value_wgrad_kernel    a thread owns 8 columns and walks the list in ascending order: dw[k] = fma(dv_r, hn[r,k], dw[k]);
//                         one more workgroup sums db (lane L takes entries L, L + 64, … ascending, then wave_sum).
//   value_dgrad_kernel    one wave per list entry: dh[r,k] = bf16(float(dh[r,k]) + dv_r·w[k]); skipped when dh is NULL.
//
// Inference, one launch (bl_value_predict_f32):
//   value_predict_kernel  one wave per residual row: the final RMSNorm of norm.hip and value_rows_kernel's v, the row held in
//                         registers in between — the bits of the two ops in sequence, one fp32 per row out.
#include "bl_common.h"
#include <limits.h>
#include <math.h>

namespace bl_value_impl {

enum { VR_VALUE = 0, VR_LOSS, VR_CLIPPED, VR_DV };

__device__ __forceinline__ void unpack8(const u32x4_t q, float* v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = bflo(q[i]);
    v[2 * i + 1] = bfhi(q[i]);
  }
}

// token level (action == 0): thread i ↔ row i. action level: wave i ↔ sequence i, the lowest valid row by a
// min-reduction over the lanes' own lowest. Both zero value_rows of the rows they visit (every row exactly once).
__global__ __launch_bounds__(256) void value_mark_kernel(const int64_t* targets, long ignore_index, int rows, int group_rows,
                                                         int action, int32_t* index, float* value_rows) {
  if (!action) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    index[r] = targets[r] != ignore_index ? r : -1;
    *(f32x4_t*)(value_rows + (long)r * 4) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    return;
  }
  const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (seq >= rows / group_rows) return;      // uniform per wave
  const long r0 = (long)seq * group_rows;
  int first = INT_MAX;
  for (int k = lane; k < group_rows; k += 64) {
    const long r = r0 + k;
    if (targets[r] != ignore_index && first == INT_MAX) first = (int)r;
    *(f32x4_t*)(value_rows + r * 4) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if (lane == 0) index[seq] = first == INT_MAX ? -1 : first;
}

// in place: an entry moves to a position at or below its own, and every entry of a chunk is read before the barrier that
// precedes the chunk's writes
__global__ __launch_bounds__(256) void value_compact_kernel(int32_t* index, int cap, int32_t* count) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int c0 = 0; c0 < cap; c0 += 256) {
    const int i = c0 + threadIdx.x;
    const int v = i < cap ? index[i] : -1;
    const unsigned long long bal = __ballot(v >= 0);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int k = 0; k < wave; ++k) off += wcnt[k];
    if (v >= 0) index[off + __popcll(bal & ((1ull << lane) - 1ull))] = v;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  for (int i = base + threadIdx.x; i < cap; i += 256) index[i] = -1;
  if (threadIdx.x == 0) count[0] = base;
}

// one wave per list entry, four per workgroup, no barrier. clip < 0: unclipped (old_values is not read).
__global__ __launch_bounds__(256) void value_rows_kernel(const uint16_t* hn, long ld, int dim, const uint16_t* w, const uint16_t* b,
                                                         const float* returns, const float* old_values, float coef, float clip,
                                                         const int32_t* index, const int32_t* count, int cap, int rows,
                                                         float* value_rows) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = count[0];
  if (j >= cap || j >= n) return;            // uniform per wave
  const int r = index[j];
  if (r < 0 || r >= rows) return;            // never with a list the kernels above wrote: nothing is indexed unchecked
  const uint16_t* hr = hn + (long)r * ld;
  float acc = 0.f;
  for (int k = lane * 8; k < dim; k += 512) {
    float h[8], ww[8];
    unpack8(*(const u32x4_t*)(hr + k), h);
    unpack8(*(const u32x4_t*)(w + k), ww);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(h[e], ww[e], acc);
  }
  acc = wave_sum(acc);
  if (lane != 0) return;
  const float v = acc + bf2f(b[0]);
  const float R = returns[r];
  const float e = v - R;
  float ec = e;
  if (clip >= 0.f) {
    const float vo = old_values[r];
    const float d = v - vo;                  // inside the range vc IS v: ec = e exactly, not vo + (v − vo) − R with its rounding,
    if (fabsf(d) > clip) ec = (vo + copysignf(clip, d)) - R;      // which could break the tie towards "clipped"
  }
  const float e2 = e * e, ec2 = ec * ec;
  const bool unclipped = e2 >= ec2;
  *(f32x4_t*)(value_rows + (long)r * 4) =
      (f32x4_t){v, 0.5f * fmaxf(e2, ec2), unclipped ? 0.f : 1.f, unclipped ? (coef * e) / (float)n : 0.f};
}

// Σ over the 256 threads of K per-thread sums: wave_sum, then the four waves in order. Every thread gets the totals.
template <int K>
__device__ __forceinline__ void block_sums(float* a, float (*red)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = wave_sum(a[k]);
  __syncthreads();                            // a previous use of `red` has been read
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// stats = (value_loss, n, clip_frac, mean v, mean R, explained variance, mean |e|, total); total adds policy_stats[0]
__global__ __launch_bounds__(256) void value_stats_kernel(const float* value_rows, const float* returns, const int32_t* index,
                                                          const int32_t* count, int cap, int rows, float coef,
                                                          const float* policy_stats, float* out) {
  __shared__ float red[4][6], red2[4][2];
  const int n = min(count[0], cap);
  float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // Σ l, Σ clipped, Σ v, Σ R, Σ |e|, Σ e
  for (int j = threadIdx.x; j < n; j += 256) {
    const int r = index[j];
    if (r < 0 || r >= rows) continue;
    const f32x4_t q = *(const f32x4_t*)(value_rows + (long)r * 4);
    const float R = returns[r], e = q[VR_VALUE] - R;
    a[0] += q[VR_LOSS];
    a[1] += q[VR_CLIPPED];
    a[2] += q[VR_VALUE];
    a[3] += R;
    a[4] += fabsf(e);
    a[5] += e;
  }
  block_sums<6>(a, red);
  const float inv = n > 0 ? 1.0f / (float)n : 0.f;
  const float e_mean = a[5] * inv, r_mean = a[3] * inv;
  float s[2] = {0.f, 0.f};                          // Σ (e − ē)², Σ (R − R̄)²
  for (int j = threadIdx.x; j < n; j += 256) {
    const int r = index[j];
    if (r < 0 || r >= rows) continue;
    const float R = returns[r], e = value_rows[(long)r * 4 + VR_VALUE] - R;
    s[0] += (e - e_mean) * (e - e_mean);
    s[1] += (R - r_mean) * (R - r_mean);
  }
  block_sums<2>(s, red2);
  if (threadIdx.x == 0) {
    const float vl = a[0] * inv;
    out[0] = vl;
    out[1] = (float)n;
    out[2] = a[1] * inv;
    out[3] = a[2] * inv;
    out[4] = r_mean;
    out[5] = s[1] > 0.f ? 1.0f - s[0] / s[1] : 0.f;
    out[6] = a[4] * inv;
    out[7] = (policy_stats ? policy_stats[0] : 0.f) + coef * vl;
  }
}

// workgroups [0, gridDim.x − 1): thread ↔ 8 columns of dw. The last workgroup: db by its one wave.
__global__ __launch_bounds__(64) void value_wgrad_kernel(const uint16_t* hn, long ld, int dim, const float* value_rows,
                                                         const int32_t* index, const int32_t* count, int cap, int rows,
                                                         float inv_world, float* dw, float* db) {
  const int n = min(count[0], cap);
  if (blockIdx.x == gridDim.x - 1) {
    float s = 0.f;
    for (int j = threadIdx.x; j < n; j += 64) {
      const int r = index[j];
      if (r >= 0 && r < rows) s += value_rows[(long)r * 4 + VR_DV] * inv_world;
    }
    s = wave_sum(s);
    if (threadIdx.x == 0) db[0] = s;
    return;
  }
  const int k = (blockIdx.x * 64 + threadIdx.x) * 8;
  if (k >= dim) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < n; ++j) {
    const int r = index[j];
    if (r < 0 || r >= rows) continue;
    const float dv = value_rows[(long)r * 4 + VR_DV] * inv_world;
    float h[8];
    unpack8(*(const u32x4_t*)(hn + (long)r * ld + k), h);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(dv, h[e], acc[e]);
  }
  *(f32x4_t*)(dw + k) = (f32x4_t){acc[0], acc[1], acc[2], acc[3]};
  *(f32x4_t*)(dw + k + 4) = (f32x4_t){acc[4], acc[5], acc[6], acc[7]};
}

__global__ __launch_bounds__(256) void value_dgrad_kernel(const uint16_t* w, int dim, const float* value_rows, const int32_t* index,
                                                          const int32_t* count, int cap, int rows, float inv_world, uint16_t* dh,
                                                          long lddh) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= cap || j >= count[0]) return;     // uniform per wave
  const int r = index[j];
  if (r < 0 || r >= rows) return;
  const float dv = value_rows[(long)r * 4 + VR_DV] * inv_world;
  uint16_t* dr = dh + (long)r * lddh;
  for (int k = lane * 8; k < dim; k += 512) {
    float d[8], ww[8];
    unpack8(*(const u32x4_t*)(dr + k), d);
    unpack8(*(const u32x4_t*)(w + k), ww);
    u32x4_t q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = pack2bf(fmaf(dv, ww[2 * i], d[2 * i]), fmaf(dv, ww[2 * i + 1], d[2 * i + 1]));
    *(u32x4_t*)(dr + k) = q;
  }
}

// Inference: V(s) straight from the residual rows — the final RMSNorm and the head in one launch (bl_value_predict_f32).
// Defined by composition: the bits of bl_rmsnorm_bf16 (norm.hip, norm_rows_kernel<NCH, true>) followed by
// value_rows_kernel's v. Both give lane L the columns [512·c + 8·L, + 8) of chunk c, so the row never leaves the
// registers: the sum of squares in norm_rows_kernel's expression and order, hn = bf16(norm_w · bf16(x · rstd)) through the
// same rbf / pack2bf, then value_rows_kernel's one fmaf chain per lane in ascending k, wave_sum, + b on lane 0.
// One wave per row, four per workgroup, no LDS, no barrier; a row at or beyond `rows` and a column at or beyond `dim` are
// never loaded; the only store is out[row · out_stride].
template <int NCH>
__global__ __launch_bounds__(256) void value_predict_kernel(const uint16_t* __restrict__ x, long ldx, int rows, int dim,
                                                            const uint16_t* __restrict__ nw, float eps,
                                                            const uint16_t* __restrict__ w, const uint16_t* __restrict__ b,
                                                            float* __restrict__ out, long out_stride) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // whole wave exits together
  const int nchunk = dim >> 3;
  const uint16_t* xr = x + (long)row * ldx;
  float v[NCH][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = c * 64 + lane;
    u32x4_t q = {0u, 0u, 0u, 0u};
    if (ch < nchunk) q = *(const u32x4_t*)(xr + ch * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[c][2 * i] = bflo(q[i]); v[c][2 * i + 1] = bfhi(q[i]); }
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[c][i] * v[c][i];
  }
  s = wave_sum(s);
  const float inv_n = 1.0f / (float)dim;
  const float rstd = 1.0f / sqrtf(s * inv_n + eps);
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = c * 64 + lane;
    if (ch >= nchunk) continue;
    const u32x4_t nq = *(const u32x4_t*)(nw + ch * 8);
    u32x4_t hq;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      hq[i] = pack2bf(bflo(nq[i]) * rbf(v[c][2 * i] * rstd), bfhi(nq[i]) * rbf(v[c][2 * i + 1] * rstd));
    float h[8], ww[8];
    unpack8(hq, h);
    unpack8(*(const u32x4_t*)(w + ch * 8), ww);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(h[e], ww[e], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) out[(long)row * out_stride] = acc + bf2f(b[0]);
}

}  // namespace bl_value_impl
using namespace bl_value_impl;

// the capacity of the index list: one slot per row (token level) or per sequence (action level); < 0 for a bad shape
static int64_t value_cap(int32_t rows, int32_t group_rows, int32_t level) {
  if (rows <= 0 || (level != 0 && level != 1)) return -1;
  if (level == 0) return rows;
  if (group_rows <= 0 || (rows % group_rows)) return -1;
  return rows / group_rows;
}

extern "C" int bl_value_head_f32(const bl_bf16* hn, int64_t ld, int32_t rows, int32_t dim, const int64_t* targets,
                                 int64_t ignore_index, int32_t group_rows, int32_t level, const bl_bf16* w, const bl_bf16* b,
                                 const float* returns, const float* old_values, float coef, float clip,
                                 const float* policy_stats, int32_t* index, int32_t* count, float* value_rows, float* stats,
                                 void* stream) {
  if (!hn || !targets || !w || !b || !returns || !index || !count || !value_rows || !stats) return BL_E_ARG;
  if (!(coef >= 0.f) || clip != clip || (clip >= 0.f && !old_values)) return BL_E_ARG;
  const int64_t cap = value_cap(rows, group_rows, level);
  if (cap < 0 || dim <= 0 || (dim % 8) || (ld % 8) || ld < dim) return BL_E_SHAPE;
  if (!bl_aligned16(hn) || !bl_aligned16(w) || !bl_aligned16(value_rows)) return BL_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int mark_blocks = level == 0 ? (rows + 255) / 256 : (int)((cap + 3) / 4);
  hipLaunchKernelGGL(value_mark_kernel, dim3(mark_blocks), dim3(256), 0, s, targets, (long)ignore_index, rows, group_rows, level,
                     index, value_rows);
  hipLaunchKernelGGL(value_compact_kernel, dim3(1), dim3(256), 0, s, index, (int)cap, count);
  hipLaunchKernelGGL(value_rows_kernel, dim3((int)((cap + 3) / 4)), dim3(256), 0, s, (const uint16_t*)hn, (long)ld, dim,
                     (const uint16_t*)w, (const uint16_t*)b, returns, old_values, coef, clip, index, count, (int)cap, rows, value_rows);
  hipLaunchKernelGGL(value_stats_kernel, dim3(1), dim3(256), 0, s, value_rows, returns, index, count, (int)cap, rows, coef,
                     policy_stats, stats);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_value_head_backward_f32(const bl_bf16* hn, int64_t ld, int32_t rows, int32_t dim, int32_t group_rows,
                                          int32_t level, const bl_bf16* w, const float* value_rows, const int32_t* index,
                                          const int32_t* count, float inv_world, float* dw, float* db, bl_bf16* dh, int64_t lddh,
                                          void* stream) {
  if (!hn || !w || !value_rows || !index || !count || !dw || !db) return BL_E_ARG;
  if (!(inv_world > 0.f)) return BL_E_ARG;
  const int64_t cap = value_cap(rows, group_rows, level);
  if (cap < 0 || dim <= 0 || (dim % 8) || (ld % 8) || ld < dim) return BL_E_SHAPE;
  if (dh && ((lddh % 8) || lddh < dim)) return BL_E_SHAPE;
  if (!bl_aligned16(hn) || !bl_aligned16(w) || !bl_aligned16(value_rows) || !bl_aligned16(dw) || (dh && !bl_aligned16(dh)))
    return BL_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(value_wgrad_kernel, dim3((dim / 8 + 63) / 64 + 1), dim3(64), 0, s, (const uint16_t*)hn, (long)ld, dim,
                     value_rows, index, count, (int)cap, rows, inv_world, dw, db);
  if (dh)
    hipLaunchKernelGGL(value_dgrad_kernel, dim3((int)((cap + 3) / 4)), dim3(256), 0, s, (const uint16_t*)w, dim, value_rows, index,
                       count, (int)cap, rows, inv_world, (uint16_t*)dh, (long)lddh);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_value_predict_f32(const bl_bf16* x, int64_t ldx, int32_t rows, int32_t dim, const bl_bf16* norm_w, float eps,
                                    const bl_bf16* w, const bl_bf16* b, float* out, int64_t out_stride, void* stream) {
  if (!x || !norm_w || !w || !b || !out) return BL_E_ARG;
  if (rows <= 0 || dim <= 0 || (dim % 8) || dim > 64 * 8 * 10 || out_stride < 1) return BL_E_SHAPE;
  if ((ldx % 8) || !bl_aligned16(x) || !bl_aligned16(norm_w) || !bl_aligned16(w)) return BL_E_ALIGN;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define BL_VP_CASE(N)                                                                                                  \
  case N:                                                                                                              \
    hipLaunchKernelGGL((value_predict_kernel<N>), grid, block, 0, s, (const uint16_t*)x, (long)ldx, rows, dim,         \
                       (const uint16_t*)norm_w, eps, (const uint16_t*)w, (const uint16_t*)b, out, (long)out_stride);   \
    break;
  switch ((dim / 8 + 63) / 64) {
    BL_VP_CASE(1) BL_VP_CASE(2) BL_VP_CASE(3) BL_VP_CASE(4) BL_VP_CASE(5)
    BL_VP_CASE(6) BL_VP_CASE(7) BL_VP_CASE(8) BL_VP_CASE(9) BL_VP_CASE(10)
    default: return BL_E_SHAPE;
  }
#undef BL_VP_CASE
  BL_CHECK_LAUNCH();
  return BL_OK;
}
