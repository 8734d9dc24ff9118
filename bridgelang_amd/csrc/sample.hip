// sample.hip — bl_sample_f32: seeded sampling of one token per row of fp32 logits (temperature, top-k, top-p), the
// device twin of bridgelang_amd/sampling.py::sample_rows. Token id and both integers of the weight pair are bit-identical
// to that specification: the exponential is a fixed sequence of individually rounded fp32 operations, and everything
// behind it is integer arithmetic (weights <= 2^30, sums < 2^45).
// bl_score_f32 (twin of sampling.py::score_rows) is the same kernel in its other mode: it READS a token per row where
// the sampler writes one, and reports that token's kept weight — and, on request, the kept weights of an index range —
// under the same warped distribution. Stages 1–4 and the first walk of stage 5 are one body of code for both.
//
// One 1024-thread workgroup per row. The row is read from HBM once (16-byte loads) into ONE uint32 image in LDS
// (n·4 bytes: 128 256 B for the 32 064-token vocabulary, beside a 16.5 KB histogram inside the CU's 160 KB):
//   1. load: order-preserving integer key of every logit → LDS; row maximum and its lowest index (the greedy answer)
//   2. top-k: radix selection of the k-th largest key (11 + 11 + 10 bits, count histograms) — no sort
//   3. keys → weights in place: w = rint(exp_spec((l − max)/T)·2^30), 0 for what top-k drops; total = Σ w
//   4. top-p: radix selection on the weight with weight-SUM histograms: the threshold weight w* is the smallest weight
//      whose strictly-heavier mass is below the bound; of the tokens AT w*, the first m in index order stay
//   5. kept mass per wave (each wave owns a contiguous index range; ranks among the w* ties by ballot), the Philox
//      draw → target, then the one wave that holds the target walks its range with a wave prefix sum
//      (scoring: no draw and no second walk — during the first walk the lane that owns the given token keeps its kept
//      weight and the lanes inside the requested range store theirs)
// Histogram bins are 64-bit LDS atomics; one wave turns a histogram into the selected bin.
//
// bl_sample_range_f32 / bl_score_range_f32 restrict the policy to the columns [vocab_first, vocab_first + vocab_count) of
// every row: the same kernel with a column base. The LDS image holds vocab_count entries read from logits + row·ld +
// vocab_first, ids are reported as vocab_first + i, the scored token and the report range are taken relative to the
// base, and no column outside the range is loaded. The unranged entry points are the base-0, count-n case.
#include "bl_common.h"
#include "sample_spec.h"

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / BL_WAVE;
constexpr int kBins = 2048;
constexpr int kHistSlots = kBins + kBins / 32;                    // one pad slot per 32 bins: see hb()
constexpr int kLdsBytes = 160 * 1024;
constexpr int kFixedBytes = kHistSlots * 8;
constexpr int kMaxN = (kLdsBytes - kFixedBytes - 1024) / 4;       // 1 KB left for the static reduction scratch below
static_assert(kMaxN == kSpecMaxN, "sample_spec.h states this kernel's row limit");

typedef unsigned long long u64;

// lane L of the selecting wave walks bins 32L … 32L+31: the pad puts the lanes of a half-wave on different banks
__device__ __forceinline__ int hb(int bin) { return bin + (bin >> 5); }

__device__ __forceinline__ uint32_t key_of(float v) {
  if (v == 0.0f) v = 0.0f;                                        // −0 and +0 compare equal: one key
  const uint32_t b = __builtin_bit_cast(uint32_t, v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float logit_of(uint32_t k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// exp_spec and weight_of (sampling.py's exponential and integer weight) live in sample_spec.h: beam.hip shares them

// Philox4x32-10, counter (t, 0, 0, 0), key = the seed's two words → x0 << 32 | x1
__device__ __forceinline__ u64 philox_u64(u64 seed, uint32_t t) {
  uint32_t c0 = t, c1 = 0, c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
  }
  return ((u64)c0 << 32) | c1;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((long long)v, o, 64);
  return v;
}

// Σ v over the block, returned to every thread. red: kWaves slots of LDS; safe to call back to back.
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* red) {
  v = wave_sum_u64(v);
  __syncthreads();                                                // earlier readers of red are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 s = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += red[w];
  return s;
}

// hist[bin] += v for every lane with `on`. The lanes that share the first active lane's bin are summed in registers and
// added once: a softmax row puts most of its weights into one bin (and most logits share an exponent), which as plain
// atomics would queue up on one LDS address.
__device__ __forceinline__ void hist_add(u64* hist, bool on, int bin, u64 v) {
  const u64 active = __ballot(on);
  if (active == 0) return;                                        // wave-uniform
  const int lead = __ffsll((long long)active) - 1;
  const int lead_bin = __shfl(bin, lead, 64);
  const bool same = on && bin == lead_bin;
  const u64 s = wave_sum_u64(same ? v : 0);
  if ((int)(threadIdx.x & 63) == lead) atomicAdd(&hist[hb(lead_bin)], s);
  else if (on && !same) atomicAdd(&hist[hb(bin)], v);
}

// One wave turns the histogram into a bin. Walking the bins from the top, `excl` = the sum of all higher bins:
//   BY_COUNT: the bin that holds the need-th largest element (excl < need <= excl + hist[bin])
//   else    : the LOWEST non-empty bin with base + excl < need
// sel[0] = bin, sel[1] = its excl. Exactly one lane writes (the rows this kernel is given always have such a bin).
template <bool BY_COUNT>
__device__ __forceinline__ void select_bin(const u64* hist, u64 base, u64 need, u64* sel) {
  const int lane = threadIdx.x & 63;
  u64 mine = 0;
#pragma unroll 4
  for (int j = 0; j < 32; ++j) mine += hist[hb(lane * 32 + j)];
  u64 incl = mine;                                                // suffix sum over the lanes above (they hold higher bins)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = (u64)__shfl_down((long long)incl, o, 64);
    if (lane + o < 64) incl += up;
  }
  u64 excl = incl - mine;
  int found = -1;
  u64 found_excl = 0;
  for (int j = 31; j >= 0; --j) {
    const int bin = lane * 32 + j;
    const u64 h = hist[hb(bin)];
    const bool hit = BY_COUNT ? (excl < need && need <= excl + h) : (h != 0 && base + excl < need);
    if (hit) { found = bin; found_excl = excl; }                  // descending walk: the last hit is the lane's lowest
    excl += h;
  }
  int lowest = found < 0 ? 0x7fffffff : found;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, __shfl_xor(lowest, o, 64));
  if (found >= 0 && found == lowest) { sel[0] = (u64)found; sel[1] = found_excl; }
}

// Radix selection over the LDS image, digits of 11, 11 and 10 bits from the top. BY_COUNT: the `need`-th largest value
// (count histograms). Otherwise: the smallest non-zero value whose strictly-larger values sum below `need` (sum
// histograms; zeros are skipped). Returns the value; `above` = count / sum of the strictly larger values.
template <bool BY_COUNT>
__device__ __forceinline__ uint32_t radix_select(const uint32_t* img, int n, u64 need, u64* hist, u64* sel, u64& above) {
  uint32_t prefix = 0, known = 0;                                 // `known`: mask of the bits decided so far
  u64 base = 0;
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t dmask = pass == 2 ? 1023u : 2047u;
    for (int b = threadIdx.x; b < kHistSlots; b += kThreads) hist[b] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kThreads) {                    // whole waves stay in the loop: hist_add uses shuffles
      const int i = i0 + threadIdx.x;
      const uint32_t v = i < n ? img[i] : 0;
      const bool on = i < n && (v & known) == prefix && (BY_COUNT || v != 0);
      hist_add(hist, on, (int)((v >> shift) & dmask), BY_COUNT ? 1ull : (u64)v);
    }
    __syncthreads();
    if (threadIdx.x < 64) select_bin<BY_COUNT>(hist, base, BY_COUNT ? need - base : need, sel);
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    known |= dmask << shift;
    base += sel[1];
    __syncthreads();                                              // sel is read before the next pass rewrites it
  }
  above = base;
  return prefix;
}

// SCORE = false: the draw (seed, step → ids, wt). SCORE = true: the score of tokens[row] (→ wt, and range_wt[row][j] = the
// kept weight of token range_first + j when range_wt is given); seed, step and ids are unused there, and the reverse.
// The row is the n columns from column `base` on; range_first is relative to base, tokens and ids are not.
template <bool SCORE>
__global__ __launch_bounds__(kThreads) void sample_kernel(const float* logits, long ld, int n, const float* temperature,
                                                          const int* top_k, const float* top_p, const int64_t* seed,
                                                          uint32_t step, int64_t* ids, const int64_t* tokens, int64_t* wt,
                                                          int range_first, int range_count, int32_t* range_wt, int base) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* hist = (u64*)smem;                                         // kHistSlots
  uint32_t* img = (uint32_t*)(smem + kFixedBytes);                // n: keys, then weights
  __shared__ u64 red[kWaves];
  __shared__ u64 sel[2];
  __shared__ int s_best[kWaves];
  __shared__ int s_arg[kWaves];

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* src = logits + (long)row * ld + base;
  const float T = temperature[row];
  const float P = top_p[row];
  const int K = top_k[row];

  // 1. the row → keys in LDS; maximum and its lowest index in bl_argmax_f32's order (argmax_key: the first NaN, else the
  // first maximum), so a greedy row's id is in [0, n) whatever the row holds; rows with T > 0 need NaN-free logits
  int bk = (int)0x80000000, bi = 0x7fffffff;
  for (int i = tid * 4; i < n; i += kThreads * 4) {               // n % 4 == 0 (host check): never past column n
    const f32x4_t q = *(const f32x4_t*)(src + i);
    u32x4_t k;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      argmax_take_next(argmax_key(q[e]), i + e, bk, bi);          // i + e only grows in a thread
      k[e] = key_of(q[e]);
    }
    *(u32x4_t*)(img + i) = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) argmax_take(__shfl_xor(bk, o, 64), __shfl_xor(bi, o, 64), bk, bi);
  if (lane == 0) { s_best[wave] = bk; s_arg[wave] = bi; }
  __syncthreads();
  bk = s_best[0]; bi = s_arg[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) argmax_take(s_best[w], s_arg[w], bk, bi);
  const float best = argmax_value(bk);                            // the row maximum (either zero as +0: l − best is the same)

  int64_t tok = -1;                                               // SCORE: the token to score, relative to base; outside [0, n) it owns no lane
  int32_t* rw = nullptr;                                          // SCORE: this row of range_wt
  if constexpr (SCORE) {
    tok = tokens[row] - base;                                     // a token below the base is negative: no lane either
    if (range_wt) rw = range_wt + (long)row * range_count;
  }

  if (!(T > 0.0f)) {                                              // greedy row (block-uniform)
    if constexpr (SCORE) {                                        // one-hot at the argmax
      if (tid == 0) { wt[2 * row] = tok == (int64_t)bi; wt[2 * row + 1] = 1; }
      if (rw)
        for (int j = tid; j < range_count; j += kThreads) rw[j] = range_first + j == bi;
    } else {
      if (tid == 0) { ids[row] = (int64_t)base + bi; wt[2 * row] = 1; wt[2 * row + 1] = 1; }
    }
    return;
  }

  // 2. top-k threshold: the k-th largest key; every key >= it stays (ties included)
  uint32_t kth = 0;
  if (K > 0 && K < n) {
    u64 above;
    kth = radix_select<true>(img, n, (u64)K, hist, sel, above);
  }

  // 3. keys → weights, in place; total mass
  u64 part = 0;
  for (int i = tid; i < n; i += kThreads) {
    const uint32_t k = img[i];
    const uint32_t w = k >= kth ? weight_of(logit_of(k), best, T) : 0u;
    img[i] = w;
    part += w;
  }
  const u64 total = block_sum_u64(part, red);                     // its barriers also publish the weights

  // 4. top-p: keep the ranking's prefix whose `before` mass is below ceil(P24·total / 2^24)
  uint32_t wstar = 0;                                             // keep w > wstar, and the first m tokens with w == wstar
  u64 m = 0;
  if (P < 1.0f) {
    const u64 p24 = (u64)rintf(P * 16777216.0f);
    const u64 lo = p24 * total + 0xFFFFFFull;                     // (p24·total + 2^24 − 1) >> 24 on the 70-bit product
    const u64 hi = __umul64hi(p24, total) + (lo < 0xFFFFFFull);   // (the low word wrapped iff it ended below the addend)
    u64 bound = (hi << 40) | (lo >> 24);                          // before·2^24 < p24·total  ⇔  before < bound
    if (bound == 0) bound = 1;                                    // the first-ranked token always stays
    u64 above;
    wstar = radix_select<false>(img, n, bound, hist, sel, above);
    m = (bound - above + wstar - 1) / wstar;                      // tie j stays iff above + j·wstar < bound
  }

  // 5. kept mass in index order. Wave w owns indices [w·span, (w+1)·span), 64 per round.
  const int span = ((n + kWaves - 1) / kWaves + 63) & ~63;
  const int lo = wave * span, hi = min(n, lo + span);
  u64 ties = 0;                                                   // tokens at wstar in the waves before this one
  if (m != 0) {
    u64 mine = 0;
    for (int i = lo + lane; i < hi; i += 64) mine += img[i] == wstar;
    mine = wave_sum_u64(mine);
    __syncthreads();
    if (lane == 0) red[wave] = mine;
    __syncthreads();
    for (int w = 0; w < wave; ++w) ties += red[w];
  }
  const u64 lanes_below = (1ull << lane) - 1;
  auto kept = [&](int i, u64& seen) -> u64 {                      // whole wave calls it; `seen` = ties before this round
    const uint32_t w = i < hi ? img[i] : 0u;
    const bool tie = m != 0 && i < hi && w == wstar;
    const u64 tb = __ballot(tie);
    const u64 rank = seen + (u64)__popcll(tb & lanes_below);
    seen += (u64)__popcll(tb);
    return (w > wstar || (tie && rank < m)) ? (u64)w : 0ull;
  };
  u64 seen = ties, acc = 0, tokw = 0;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const int i = i0 + lane;
    const u64 w = kept(i, seen);
    acc += w;
    if constexpr (SCORE) {
      if ((int64_t)i == tok) tokw = w;                            // i >= hi: kept() gave 0
      if (rw && i < hi && i >= range_first && i - range_first < range_count) rw[i - range_first] = (int32_t)w;
    }
  }
  acc = wave_sum_u64(acc);
  __syncthreads();
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  u64 before = 0, total_kept = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) before += red[w];
    total_kept += red[w];
  }
  if constexpr (SCORE) {
    tokw = block_sum_u64(tokw, red);                              // at most one lane of the block holds a non-zero
    if (tid == 0) { wt[2 * row] = (int64_t)tokw; wt[2 * row + 1] = (int64_t)total_kept; }
    return;
  }
  const u64 target = __umul64hi(philox_u64((u64)seed[row], step), total_kept);
  if (target < before || target >= before + acc) return;          // wave-uniform: one wave holds the target

  seen = ties;
  u64 run = before;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const u64 w = kept(i0 + lane, seen);
    u64 incl = w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 dn = (u64)__shfl_up((long long)incl, o, 64);
      if (lane >= o) incl += dn;
    }
    const u64 past = __ballot(run + incl > target);
    if (past) {
      if (lane == __ffsll((long long)past) - 1) {
        ids[row] = (int64_t)base + (i0 + lane);
        wt[2 * row] = (int64_t)w;
        wt[2 * row + 1] = (int64_t)total_kept;
      }
      return;
    }
    run += __shfl((long long)incl, 63, 64);
  }
}

}  // namespace

// the 160 KB LDS layout needs the attribute once per kernel instantiation
template <bool SCORE>
static int allow_full_lds() {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<SCORE>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes - 1024) != hipSuccess)
      return BL_E_LAUNCH;
    attr_set = true;
  }
  return BL_OK;
}

// n here is the number of columns a row has in memory; the policy is columns [vfirst, vfirst + vcount) of it
static bool bad_vocab(int32_t n, int64_t ld, int32_t vfirst, int32_t vcount) {
  return n <= 0 || (ld % 4) || ld < n || vfirst < 0 || vcount <= 0 || (vfirst % 4) || (vcount % 4) ||
         (int64_t)vfirst + vcount > n || vcount > kMaxN;
}

extern "C" int bl_sample_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                                   const int32_t* top_k, const float* top_p, const int64_t* seed, int32_t step,
                                   int64_t* ids, int64_t* wt, int32_t vocab_first, int32_t vocab_count, void* stream) {
  if (!logits || !temperature || !top_k || !top_p || !seed || !ids || !wt) return BL_E_ARG;
  if (rows <= 0 || bad_vocab(n, ld, vocab_first, vocab_count) || step < 0) return BL_E_SHAPE;
  if (!bl_aligned16(logits) || (((uintptr_t)seed | (uintptr_t)ids | (uintptr_t)wt) & 7) ||
      (((uintptr_t)temperature | (uintptr_t)top_k | (uintptr_t)top_p) & 3))
    return BL_E_ALIGN;
  if (const int rc = allow_full_lds<false>()) return rc;
  const size_t lds = (size_t)kFixedBytes + (size_t)vocab_count * 4;
  hipLaunchKernelGGL(sample_kernel<false>, dim3(rows), dim3(kThreads), lds, (hipStream_t)stream, logits, (long)ld,
                     vocab_count, temperature, top_k, top_p, seed, (uint32_t)step, ids, (const int64_t*)nullptr, wt, 0, 0,
                     (int32_t*)nullptr, vocab_first);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_score_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                                  const int32_t* top_k, const float* top_p, const int64_t* tokens, int64_t* wt,
                                  int32_t range_first, int32_t range_count, int32_t* range_wt, int32_t vocab_first,
                                  int32_t vocab_count, void* stream) {
  if (!logits || !temperature || !top_k || !top_p || !tokens || !wt || (range_count > 0 && !range_wt)) return BL_E_ARG;
  if (rows <= 0 || bad_vocab(n, ld, vocab_first, vocab_count)) return BL_E_SHAPE;
  if (range_count < 0 || (range_count > 0 && (range_first < vocab_first ||
                                              (int64_t)range_first + range_count > (int64_t)vocab_first + vocab_count)))
    return BL_E_SHAPE;
  if (!bl_aligned16(logits) || (((uintptr_t)tokens | (uintptr_t)wt) & 7) ||
      (((uintptr_t)temperature | (uintptr_t)top_k | (uintptr_t)top_p) & 3) || (range_count > 0 && ((uintptr_t)range_wt & 3)))
    return BL_E_ALIGN;
  if (const int rc = allow_full_lds<true>()) return rc;
  const size_t lds = (size_t)kFixedBytes + (size_t)vocab_count * 4;
  hipLaunchKernelGGL(sample_kernel<true>, dim3(rows), dim3(kThreads), lds, (hipStream_t)stream, logits, (long)ld,
                     vocab_count, temperature, top_k, top_p, (const int64_t*)nullptr, 0u, (int64_t*)nullptr, tokens, wt,
                     range_count > 0 ? range_first - vocab_first : 0, range_count,
                     range_count > 0 ? range_wt : (int32_t*)nullptr, vocab_first);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_sample_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                             const int32_t* top_k, const float* top_p, const int64_t* seed, int32_t step, int64_t* ids,
                             int64_t* wt, void* stream) {
  return bl_sample_range_f32(logits, ld, rows, n, temperature, top_k, top_p, seed, step, ids, wt, 0, n, stream);
}

extern "C" int bl_score_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                            const int32_t* top_k, const float* top_p, const int64_t* tokens, int64_t* wt,
                            int32_t range_first, int32_t range_count, int32_t* range_wt, void* stream) {
  return bl_score_range_f32(logits, ld, rows, n, temperature, top_k, top_p, tokens, wt, range_first, range_count, range_wt,
                            0, n, stream);
}
