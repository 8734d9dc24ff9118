// policy.hip — the clipped-surrogate policy-gradient loss (PPO / GRPO form) over fp32 logits rows, with an entropy bonus
// and a k3 KL penalty against a reference policy: the second loss the training step can plan, beside the shifted
// cross-entropy (glue.hip / train.hip). bridgelang_amd/training/policy_loss.py is the fp64 definition; these kernels are
// its fp32 twin to a tolerance (expf / logf, as the cross-entropy kernels).
//
// Same conventions as cross-entropy: one workgroup per row, targets[row] = token of the NEXT position, ignore_index rows
// contribute nothing (and their logits are never read), 16-byte accesses, deterministic reductions, no float atomics.
// HBM-bound: the forward reads a valid row twice, the backward once (m, log S, H and g are saved per row), and the bf16
// zero fill of the ignored rows' dlogits is most of the traffic at training shapes.
//
// bl_policy_loss_range_f32 / bl_policy_loss_backward_range_f32 take the policy over the columns [first, first + count) of
// every row (the 256 action bins of the 32 064-row vocabulary): m, S, H, logp and p_i are over the range, no logit
// outside it is read, and dlogits is 0 there. The forward is row_forward over the range, by a whole workgroup for a long
// range and by ONE WAVE for a range of at most 256 columns (a float4 per lane: four rows per workgroup, no barrier and
// no idle wave); both call the same finish_row → row_terms. The backward is the one kernel with a column window. The
// unranged entry points are the (0, n) case of the workgroup kernels.
//
// bl_policy_loss_grouped_f32 takes the importance ratio per ACTION, not per token: the valid rows of each run of group_rows
// consecutive rows (one sequence) share ratio_G = exp(c·Σ (logp − q)), c = 1 or 1 / n_G. It is the row pass above, then
// policy_group_kernel (one wave per sequence; it overwrites ratio, row_loss, clipped and g of the valid rows with the
// group-level values and writes group_stats), then the statistics with the log-ratio read from group_stats. m, log S, H
// and g stay where the backward kernel reads them, so the backward entry points serve both levels.
//
// bl_policy_loss_is_f32 is either level with the rollout correction: a truncated importance weight w = min(exp(q − μ), cap),
// 0 outside a trust band, between the proximal policy q (given, or this forward's own logp) and the behaviour policy μ that
// drew the tokens, as a constant factor of the surrogate. The same kernels in their IS instantiation: is_terms is the one
// definition of (λ, ρ, w), (λ, w) per row go to is_rows and six more means to is_stats. g still holds ∂row_loss/∂logp, so
// the backward entry points serve it too.
//
// bl_preference_loss_f32 is the preference-pair loss (DPO family; training/preference_loss.py) on the same rows: the row
// pass without the surrogate, then preference_seq_kernel, preference_pair_kernel and preference_apply_kernel (below, with
// their own comment). It leaves g per row, and the number of pairs in stats[1], for the same backward entry points.
#include "bl_common.h"
#include <math.h>

namespace bl_policy_impl {

// per-row statistics, fp32 [rows, 8]
enum { RS_LOGP = 0, RS_H, RS_RATIO, RS_LOSS, RS_CLIPPED, RS_M, RS_LOGS, RS_G };

struct PolicyParams {
  float inv_t, clip_low, clip_high, entropy_coef, kl_coef;
};

// Everything of a row that follows from log π(a) alone. ONE definition for the row kernels, the group kernel and both step
// reductions: the clipped surrogate from a given log-ratio (a token's or a group's), then the KL term of the row.
struct RowTerms {
  float ratio, log_ratio, pg, kl, g;
  bool active;
};
__device__ __forceinline__ RowTerms surrogate_terms(float log_ratio, float A, const PolicyParams& P) {
  RowTerms t;
  t.log_ratio = log_ratio;
  t.ratio = expf(t.log_ratio);
  const float lo = 1.0f - P.clip_low, hi = 1.0f + P.clip_high;
  const float clipped = fminf(fmaxf(t.ratio, lo), hi);
  t.pg = -fminf(t.ratio * A, clipped * A);
  t.active = (A >= 0.f && t.ratio <= hi) || (A < 0.f && t.ratio >= lo);   // clamp passes its gradient at the boundary
  t.kl = 0.f;
  t.g = t.active ? -A * t.ratio : 0.f;
  return t;
}
// kl = k3 of the row, and its share of ∂row_loss/∂logp taken off g
__device__ __forceinline__ void kl_terms(float logp, const float* ref, int row, const PolicyParams& P, float& kl, float& g) {
  if (ref) {
    const float d = ref[row] - logp;
    const float em1 = expm1f(d);
    kl = em1 - d;                          // exp(d) − d − 1 (k3)
    g -= P.kl_coef * em1;                  // kl_coef·(1 − exp(d))
  }
}
__device__ __forceinline__ RowTerms row_terms(float logp, float A, float q, const float* ref, int row, const PolicyParams& P) {
  RowTerms t = surrogate_terms(logp - q, A, P);
  kl_terms(logp, ref, row, P, t.kl, t.g);
  return t;
}

// ---- the rollout correction (bl_policy_loss_is_f32): a truncated importance weight between the proximal policy q and the
// behaviour policy μ that drew the tokens. The kernels below are templates on IS: the IS = false instantiations are the
// uncorrected loss and never look at an IsArgs (they are passed an empty one); the IS = true ones read and write through it.
struct IsArgs {
  const float* mu;      // behaviour log-probability per row
  float* rows;          // fp32 [rows, 2] = (λ, w)
  float cap, lo, hi;    // w = min(ρ, cap), 0 where ρ is outside [lo, hi] (no mask: lo = 0, hi = +inf)
};
// Everything that follows from λ = q − μ (a token's, or c·Σ over a group). ONE definition for the row kernels, the group
// kernel and both reductions, as surrogate_terms is for the ratio.
struct IsTerms {
  float lambda, rho, w;
  bool masked, truncated;
};
__device__ __forceinline__ IsTerms is_terms(float lambda, const IsArgs& I) {
  IsTerms s;
  s.lambda = lambda;
  s.rho = expf(lambda);
  s.masked = s.rho < I.lo || s.rho > I.hi;
  s.truncated = !s.masked && s.rho > I.cap;
  s.w = s.masked ? 0.f : fminf(s.rho, I.cap);
  return s;
}
// w·x as a product of its own: the compiler may not contract it into the sum x goes on to, so with w = 1 every later
// result has the bits of the uncorrected loss (the empty statement only hides the product from the optimiser)
__device__ __forceinline__ float weighted(float w, float x) {
  float y = w * x;
  asm volatile("" : "+v"(y));
  return y;
}
// the weight is a constant factor of the surrogate: on pg and on the surrogate's share of g, before the KL share is taken off
__device__ __forceinline__ void weight_surrogate(RowTerms& t, float w) {
  t.pg = weighted(w, t.pg);
  t.g = weighted(w, t.g);
}
// a row's proximal log-probability: the given one, or (self-proximal) this forward's own logp as a constant
__device__ __forceinline__ float proximal(const float* old_lp, long row, float logp) { return old_lp ? old_lp[row] : logp; }

__device__ __forceinline__ float row_loss_of(const RowTerms& t, float H, const PolicyParams& P) {
  return t.pg - P.entropy_coef * H + P.kl_coef * t.kl;
}

// what thread 0 / lane 0 does once S and W of a row are known. lr points at column `first`; tgt is relative to it.
// SURR = false is the row pass of the preference loss: the same logp, H, m and log S, no surrogate (adv, old_lp and ref_lp
// are not read); ratio, row_loss, clipped and g are written as zeros for preference_apply_kernel to fill. IS (with SURR)
// is the rollout correction: q may be this row's own logp, the surrogate carries w, and (λ, w) go to I.rows.
template <bool SURR, bool IS>
__device__ __forceinline__ void finish_row(const float* lr, int n, long tgt, float m, float S, float W, const float* adv,
                                           const float* old_lp, const float* ref_lp, int row, const PolicyParams& P,
                                           const IsArgs& I, float* rs) {
  const float logS = logf(S);
  const float H = logS - W / S;                                       // −Σ p·logp, logp = (z − m) − log S
  const float za = (tgt >= 0 && tgt < n) ? lr[tgt] * P.inv_t : NAN;    // a token outside the row: NaN, never a stray read
  const float logp = za - m - logS;
  rs[RS_LOGP] = logp;
  rs[RS_H] = H;
  rs[RS_M] = m;
  rs[RS_LOGS] = logS;
  if constexpr (SURR) {
    RowTerms t;
    if constexpr (IS) {
      const float q = proximal(old_lp, row, logp);
      const IsTerms s = is_terms(q - I.mu[row], I);
      t = surrogate_terms(logp - q, adv[row], P);
      weight_surrogate(t, s.w);
      kl_terms(logp, ref_lp, row, P, t.kl, t.g);
      I.rows[2 * (long)row] = s.lambda;
      I.rows[2 * (long)row + 1] = s.w;
    } else {
      t = row_terms(logp, adv[row], old_lp[row], ref_lp, row, P);
    }
    rs[RS_RATIO] = t.ratio;
    rs[RS_LOSS] = row_loss_of(t, H, P);
    rs[RS_CLIPPED] = t.active ? 0.f : 1.f;
    rs[RS_G] = t.g;
  } else {
    rs[RS_RATIO] = 0.f;
    rs[RS_LOSS] = 0.f;
    rs[RS_CLIPPED] = 0.f;
    rs[RS_G] = 0.f;
  }
}

// one workgroup per row; the row is the n columns from column `first` on
template <bool SURR, bool IS = false>
__global__ __launch_bounds__(256) void policy_rows_kernel(const float* logits, long ld, int first, int n, const int64_t* targets,
                                                          long ignore_index, const float* adv, const float* old_lp,
                                                          const float* ref_lp, PolicyParams P, IsArgs I, float* row_stats) {
  __shared__ float red_m[4], red_s[4], red_w[4];
  const int row = blockIdx.x;
  const long tgt = targets[row];
  float* rs = row_stats + (long)row * 8;
  if (tgt == ignore_index) {          // uniform per workgroup
    if (threadIdx.x < 8) rs[threadIdx.x] = 0.f;
    if (IS && threadIdx.x < 2) I.rows[2 * (long)row + threadIdx.x] = 0.f;
    return;
  }
  const float* lr = logits + (long)row * ld + first;
  float mx = -INFINITY;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4_t q = *(const f32x4_t*)(lr + i);
    mx = fmaxf(fmaxf(mx, fmaxf(q[0], q[1])), fmaxf(q[2], q[3]));
  }
  mx = wave_max(mx);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red_m[wave] = mx;
  __syncthreads();
  // max of z = l / T is max(l) / T (T > 0); the row is scaled as it is read
  const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3])) * P.inv_t;
  float s = 0.f, w = 0.f;             // S = Σ exp(z − m), W = Σ exp(z − m)·(z − m)
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4_t q = *(const f32x4_t*)(lr + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = q[e] * P.inv_t - m;
      const float ex = expf(d);
      s += ex;
      w += ex * d;                    // exp underflows to 0 long before d overflows: 0·d = 0
    }
  }
  s = wave_sum(s);
  w = wave_sum(w);
  if ((threadIdx.x & 63) == 0) { red_s[wave] = s; red_w[wave] = w; }
  __syncthreads();
  if (threadIdx.x == 0)
    finish_row<SURR, IS>(lr, n, tgt - first, m, red_s[0] + red_s[1] + red_s[2] + red_s[3], red_w[0] + red_w[1] + red_w[2] + red_w[3],
               adv, old_lp, ref_lp, row, P, I, rs);
}

// n <= 256: one wave per row, four rows per workgroup, the lane's float4 stays in registers between the two passes. The
// order of every sum is the workgroup kernel's on such a row (there waves 1–3 hold no column and add zeros).
template <bool SURR, bool IS = false>
__global__ __launch_bounds__(256) void policy_rows_wave_kernel(const float* logits, long ld, int first, int n, int rows,
                                                               const int64_t* targets, long ignore_index, const float* adv,
                                                               const float* old_lp, const float* ref_lp, PolicyParams P,
                                                               IsArgs I, float* row_stats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;            // uniform per wave, and the kernel has no barrier
  const long tgt = targets[row];
  float* rs = row_stats + (long)row * 8;
  if (tgt == ignore_index) {
    if (lane < 8) rs[lane] = 0.f;
    if (IS && lane < 2) I.rows[2 * (long)row + lane] = 0.f;
    return;
  }
  const float* lr = logits + (long)row * ld + first;
  const bool on = lane * 4 < n;       // n % 4 == 0: a lane's four columns are inside together
  f32x4_t q = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (on) q = *(const f32x4_t*)(lr + lane * 4);
  const float m = wave_max(fmaxf(fmaxf(-INFINITY, fmaxf(q[0], q[1])), fmaxf(q[2], q[3]))) * P.inv_t;
  float s = 0.f, w = 0.f;
  if (on) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = q[e] * P.inv_t - m;
      const float ex = expf(d);
      s += ex;
      w += ex * d;
    }
  }
  s = wave_sum(s);
  w = wave_sum(w);
  if (lane == 0) finish_row<SURR, IS>(lr, n, tgt - first, m, s + 0.f + 0.f + 0.f, w + 0.f + 0.f + 0.f, adv, old_lp, ref_lp, row, P, I, rs);
}

// The action-level ratio. One wave per sequence (its group_rows consecutive rows), four sequences per workgroup, no barrier.
// The group is the sequence's valid rows; lane l takes rows l, l + 64, ... in ascending order and every sum is a wave_sum
// of those lane partials (deterministic, no float atomics). Reads what the row pass left (logp, H) and overwrites ratio,
// row_loss, clipped and g of the valid rows: ratio_G = exp(s_G), s_G = c·Σ (logp − q), and
// g_r = c·Σ_j (−A_j·ratio_G·[active_j]) − kl_coef·expm1(ref_r − logp_r). group_stats[seq] = (s_G, ratio_G, n_G, Σ logp);
// an empty group writes zeros there and touches no row. IS is the rollout correction at this level: λ_G = c·Σ (q − μ)
// over the same rows with the same c, the group's surrogate sum carries w_G, and every valid row gets (λ_G, w_G) in I.rows.
template <bool IS>
__global__ __launch_bounds__(256) void policy_group_kernel(float* row_stats, int group_rows, int groups, int by_mean,
                                                           const int64_t* targets, long ignore_index, const float* adv,
                                                           const float* old_lp, const float* ref_lp, PolicyParams P,
                                                           IsArgs I, float* group_stats) {
  const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (seq >= groups) return;          // uniform per wave
  const long r0 = (long)seq * group_rows;
  float sd = 0.f, sl = 0.f, sm = 0.f; // Σ (logp − q), Σ logp, Σ (q − μ)
  int c = 0;
  for (int k = lane; k < group_rows; k += 64) {
    const long r = r0 + k;
    if (targets[r] == ignore_index) continue;
    const float logp = row_stats[r * 8 + RS_LOGP];
    if constexpr (IS) {
      const float q = proximal(old_lp, r, logp);
      sd += logp - q;
      sm += q - I.mu[r];
    } else {
      sd += logp - old_lp[r];
    }
    sl += logp;
    ++c;
  }
  sd = wave_sum(sd);
  sl = wave_sum(sl);
  if constexpr (IS) sm = wave_sum(sm);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  float* gs = group_stats + (long)seq * 4;
  if (c == 0) {                       // uniform per wave
    if (lane < 4) gs[lane] = 0.f;
    return;
  }
  const float w = by_mean ? 1.0f / (float)c : 1.0f;
  const float s = w * sd;
  float gsum = 0.f;                   // Σ −A_j·ratio_G·[active_j]
  for (int k = lane; k < group_rows; k += 64) {
    const long r = r0 + k;
    if (targets[r] == ignore_index) continue;
    gsum += surrogate_terms(s, adv[r], P).g;
  }
  gsum = wave_sum(gsum);
  IsTerms is = {0.f, 1.f, 1.f, false, false};
  if constexpr (IS) {                 // the weight is formed at the ratio's level, with its norm; w_G·Σ_j = Σ_j w_G·
    is = is_terms(w * sm, I);
    gsum = weighted(is.w, gsum);
  }
  for (int k = lane; k < group_rows; k += 64) {
    const long r = r0 + k;
    if (targets[r] == ignore_index) continue;
    float* rs = row_stats + r * 8;
    RowTerms t = surrogate_terms(s, adv[r], P);
    t.g = w * gsum;
    if constexpr (IS) {
      t.pg = weighted(is.w, t.pg);
      I.rows[2 * r] = is.lambda;
      I.rows[2 * r + 1] = is.w;
    }
    kl_terms(rs[RS_LOGP], ref_lp, (int)r, P, t.kl, t.g);
    rs[RS_RATIO] = t.ratio;
    rs[RS_LOSS] = row_loss_of(t, rs[RS_H], P);
    rs[RS_CLIPPED] = t.active ? 0.f : 1.f;
    rs[RS_G] = t.g;
  }
  if (lane == 0) {                    // lane 0 may hold no valid row: the ratio again, from the same s
    gs[0] = s;
    gs[1] = expf(s);
    gs[2] = (float)c;
    gs[3] = sl;
  }
}

// the 8 step statistics: means over valid rows (single workgroup, fixed summation order → deterministic). The log-ratio
// of a row is its own (group_stats NULL) or its group's, as policy_group_kernel left it in group_stats. IS: λ of a row
// (its own or its group's) is read back from I.rows, pg carries w, and six more means go to is_out (w, ρ, truncated,
// masked, ρ − 1 − λ, −λ; then two zeros), summed in the same order as the other seven.
template <bool IS>
__device__ __forceinline__ void stats_body(const float* row_stats, const int64_t* targets, long ignore_index, const float* adv,
                                           const float* old_lp, const float* ref_lp, const PolicyParams& P, int rows,
                                           const float* group_stats, int group_rows, float* out, const IsArgs& I, float* is_out) {
  constexpr int NS = IS ? 13 : 7;
  __shared__ float rsum[4][NS];
  __shared__ int rc[4];
  float a[NS];                        // row_loss, pg, H, kl, clipped, approx KL, ratio; IS: then w, ρ, truncated, masked, ρ − 1 − λ, −λ
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < rows; i += 256) {
    if (targets[i] == ignore_index) continue;
    const float* rs = row_stats + (long)i * 8;
    RowTerms t;
    if (group_stats) {
      t = surrogate_terms(group_stats[(long)(i / group_rows) * 4], adv[i], P);
      kl_terms(rs[RS_LOGP], ref_lp, i, P, t.kl, t.g);
    } else if constexpr (IS) {
      t = row_terms(rs[RS_LOGP], adv[i], proximal(old_lp, i, rs[RS_LOGP]), ref_lp, i, P);
    } else {
      t = row_terms(rs[RS_LOGP], adv[i], old_lp[i], ref_lp, i, P);
    }
    if constexpr (IS) {
      const IsTerms s = is_terms(I.rows[2 * (long)i], I);
      t.pg = weighted(s.w, t.pg);
      a[7] += s.w;
      a[8] += s.rho;
      a[9] += s.truncated ? 1.f : 0.f;
      a[10] += s.masked ? 1.f : 0.f;
      a[11] += expm1f(s.lambda) - s.lambda;              // (ρ − 1) − λ
      a[12] += -s.lambda;
    }
    a[0] += rs[RS_LOSS];
    a[1] += t.pg;
    a[2] += rs[RS_H];
    a[3] += t.kl;
    a[4] += rs[RS_CLIPPED];
    a[5] += expm1f(t.log_ratio) - t.log_ratio;         // (ratio − 1) − log ratio
    a[6] += t.ratio;
    ++c;
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = wave_sum(a[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) rsum[threadIdx.x >> 6][k] = a[k];
    rc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int k = threadIdx.x;
    const int cnt = rc[0] + rc[1] + rc[2] + rc[3];
    const float mean = cnt > 0 ? (rsum[0][k] + rsum[1][k] + rsum[2][k] + rsum[3][k]) / (float)cnt : 0.f;
    if (k < 7) {
      out[k == 0 ? 0 : k + 1] = mean;
      if (k == 0) out[1] = (float)cnt;
    } else {
      is_out[k - 7] = mean;
    }
  } else if (IS && threadIdx.x < 15) {
    is_out[threadIdx.x - 7] = 0.f;    // the two spare slots
  }
}
__global__ __launch_bounds__(256) void policy_stats_kernel(const float* row_stats, const int64_t* targets, long ignore_index,
                                                           const float* adv, const float* old_lp, const float* ref_lp,
                                                           PolicyParams P, int rows, float* out) {
  stats_body<false>(row_stats, targets, ignore_index, adv, old_lp, ref_lp, P, rows, nullptr, 1, out, IsArgs{}, nullptr);
}
__global__ __launch_bounds__(256) void policy_stats_grouped_kernel(const float* row_stats, const int64_t* targets,
                                                                   long ignore_index, const float* adv, const float* ref_lp,
                                                                   PolicyParams P, int rows, const float* group_stats,
                                                                   int group_rows, float* out) {
  stats_body<false>(row_stats, targets, ignore_index, adv, nullptr, ref_lp, P, rows, group_stats, group_rows, out, IsArgs{}, nullptr);
}
// both levels of the corrected loss: group_stats NULL is the token level (old_lp NULL: self-proximal)
__global__ __launch_bounds__(256) void policy_stats_is_kernel(const float* row_stats, const int64_t* targets, long ignore_index,
                                                              const float* adv, const float* old_lp, const float* ref_lp,
                                                              PolicyParams P, int rows, const float* group_stats,
                                                              int group_rows, float* out, IsArgs I, float* is_out) {
  stats_body<true>(row_stats, targets, ignore_index, adv, old_lp, ref_lp, P, rows, group_stats, group_rows, out, I, is_out);
}

__device__ __forceinline__ u32x4_t pack8(const float* v) {
  u32x4_t q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = pack2bf(v[2 * i], v[2 * i + 1]);
  return q;
}

// dlogits_i = [ g·(δ_ia − p_i) + entropy_coef·p_i·(logp_i + H) ] / (T · n_valid): one read of the row; logp_i by arithmetic
// (z_i − m − log S), so an underflowed p_i gives 0·finite = 0, never 0·(−inf). The policy is over columns [first, first +
// count): the 8-column groups outside it (first and count are multiples of 8) are written as zeros and never read.
__global__ __launch_bounds__(256) void policy_backward_kernel(const float* logits, long ld, int n, const int64_t* targets,
                                                              long ignore_index, const float* row_stats, const float* stats,
                                                              float inv_t, float entropy_coef, uint16_t* dlogits, long ldd,
                                                              int first, int count) {
  const int row = blockIdx.x;
  const long tgt = targets[row];
  uint16_t* dr = dlogits + (long)row * ldd;
  if (tgt == ignore_index) {
    for (int i = threadIdx.x * 8; i < n; i += 2048) *(u32x4_t*)(dr + i) = (u32x4_t){0u, 0u, 0u, 0u};
    return;
  }
  const float* lr = logits + (long)row * ld;
  const float* rs = row_stats + (long)row * 8;
  const float H = rs[RS_H], g = rs[RS_G];
  const float off = rs[RS_M] + rs[RS_LOGS];
  const float scale = inv_t / stats[1];                 // 1 / (T · n_valid)
  for (int i = threadIdx.x * 8; i < n; i += 2048) {
    if (i < first || i - first >= count) {
      *(u32x4_t*)(dr + i) = (u32x4_t){0u, 0u, 0u, 0u};
      continue;
    }
    const f32x4_t a = *(const f32x4_t*)(lr + i), b = *(const f32x4_t*)(lr + i + 4);
    float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float lp = v[e] * inv_t - off;
      const float p = expf(lp);
      v[e] = (g * (((long)(i + e) == tgt ? 1.f : 0.f) - p) + entropy_coef * p * (lp + H)) * scale;
    }
    *(u32x4_t*)(dr + i) = pack8(v);
  }
}

// ---- the preference-pair loss (training/preference_loss.py): the row pass above without the surrogate, then three small
// kernels over what it left. Sequences are runs of group_rows rows as for policy_group_kernel; pair[b] = +k / −k / 0 puts
// sequence b on the chosen / rejected side of pair k or in none. g of every valid row is rewritten so that the policy
// backward kernel (entropy_coef = 0, stats[1] = P) writes this loss's dlogits.
enum { PREF_SIGMOID = 0, PREF_IPO = 1, PREF_HINGE = 2 };
struct PrefParams {
  float beta, margin, eps, alpha;
  int kind, by_mean;
};

// P: the host's count, or the device scalar's (a captured graph serves batches with another number of pairs), kept inside
// [1, cap] — cap is how many rows pair_stats has
__device__ __forceinline__ int pref_pairs(int cap, const int32_t* n_pairs_dev) {
  const int P = n_pairs_dev ? *n_pairs_dev : cap;
  return P < 1 ? 1 : (P > cap ? cap : P);
}
// the signed pair id of sequence b, 0 for an id outside ±P: nothing is indexed by an unchecked id
__device__ __forceinline__ int pref_id(const int32_t* pair, int b, int P) {
  const long v = pair[b];
  const long k = v < 0 ? -v : v;
  return (k >= 1 && k <= P) ? (int)v : 0;
}
__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// One wave per sequence, four sequences per workgroup, no barrier: n_b, δ_b = c_b·Σ (logp − ref) and Σ logp over the
// sequence's valid rows, lanes striding the rows in ascending order as policy_group_kernel. seq_stats[b] = (δ_b, n_b,
// Σ logp, 0); slot 3 is preference_apply_kernel's.
__global__ __launch_bounds__(256) void preference_seq_kernel(const float* row_stats, int group_rows, int groups, int by_mean,
                                                             const int64_t* targets, long ignore_index, const float* ref_lp,
                                                             float* seq_stats) {
  const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (seq >= groups) return;          // uniform per wave
  const long r0 = (long)seq * group_rows;
  float sd = 0.f, sl = 0.f;           // Σ (logp − ref), Σ logp
  int c = 0;
  for (int k = lane; k < group_rows; k += 64) {
    const long r = r0 + k;
    if (targets[r] == ignore_index) continue;
    const float logp = row_stats[r * 8 + RS_LOGP];
    sd += ref_lp ? logp - ref_lp[r] : logp;
    sl += logp;
    ++c;
  }
  sd = wave_sum(sd);
  sl = wave_sum(sl);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) {
    float* ss = seq_stats + (long)seq * 4;
    ss[0] = c == 0 ? 0.f : (by_mean ? 1.0f / (float)c : 1.0f) * sd;
    ss[1] = (float)c;
    ss[2] = sl;
    ss[3] = 0.f;
  }
}

// The pair level and the 8 step statistics, ONE workgroup: thread t takes pairs t, t + 256, … and walks the sequences in
// ascending b for each (Δ_k, N_k, nll_k; O(P·B / 256) steps per thread, a few hundred at training batches), writes
// pair_stats[k] = (h_k, ℓ_k, ℓ'_k, nll_k) — zeros for the rows [P, cap) — and the statistics are the means over the pairs,
// summed per thread in ascending k, then wave_sum, then the four waves in order. stats[1] = P. A pair without a chosen
// token (the host refuses it) gets nll 0, not a division by zero.
__global__ __launch_bounds__(256) void preference_pair_kernel(const float* seq_stats, const int32_t* pair, int groups, int cap,
                                                              const int32_t* n_pairs_dev, PrefParams Q, float* pair_stats,
                                                              float* out) {
  __shared__ float rsum[4][7];
  const int P = pref_pairs(cap, n_pairs_dev);
  float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // ℓ + α·nll, ℓ, [Δ > 0], β·Δ, β·chosen, β·rejected, nll
  for (int k = threadIdx.x; k < cap; k += 256) {
    float* ps = pair_stats + (long)k * 4;
    if (k >= P) {
      ps[0] = ps[1] = ps[2] = ps[3] = 0.f;
      continue;
    }
    float rc = 0.f, rr = 0.f, lp = 0.f, N = 0.f;
    for (int b = 0; b < groups; ++b) {
      const int id = pref_id(pair, b, P);
      if (id == k + 1) {
        rc += seq_stats[(long)b * 4];
        N += seq_stats[(long)b * 4 + 1];
        lp += seq_stats[(long)b * 4 + 2];
      } else if (id == -(k + 1)) {
        rr += seq_stats[(long)b * 4];
      }
    }
    const float nll = N > 0.f ? -lp / N : 0.f;
    const float delta = rc - rr;
    const float h = Q.beta * delta - Q.margin;
    float l, dl;
    if (Q.kind == PREF_SIGMOID) {
      const float e = expf(-fabsf(h));
      l = (1.0f - Q.eps) * softplusf(-h) + Q.eps * softplusf(h);
      dl = (h >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e)) - (1.0f - Q.eps);
    } else if (Q.kind == PREF_IPO) {
      const float u = h / Q.beta - 1.0f / (2.0f * Q.beta);
      l = u * u;
      dl = 2.0f * u / Q.beta;
    } else {
      l = fmaxf(0.f, 1.0f - h);
      dl = h < 1.0f ? -1.0f : 0.f;
    }
    ps[0] = h;
    ps[1] = l;
    ps[2] = dl;
    ps[3] = nll;
    a[0] += l + Q.alpha * nll;
    a[1] += l;
    a[2] += delta > 0.f ? 1.f : 0.f;
    a[3] += Q.beta * delta;
    a[4] += Q.beta * rc;
    a[5] += Q.beta * rr;
    a[6] += nll;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) a[k] = wave_sum(a[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) rsum[threadIdx.x >> 6][k] = a[k];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    out[k == 0 ? 0 : k + 1] = (rsum[0][k] + rsum[1][k] + rsum[2][k] + rsum[3][k]) / (float)P;
    if (k == 0) out[1] = (float)P;
  }
}

// One wave per sequence again: g_r = ℓ'_k·β·sign(pair[b])·c_b − [pair[b] > 0]·α / N_k into RS_G of the sequence's valid rows
// (0 for a sequence in no pair) and the first term into seq_stats[b][3]. N_k is recounted here from the n_b of the pair's
// chosen sequences: small integers in fp32, exact in any order. RS_RATIO, RS_LOSS and RS_CLIPPED stay the zeros of the row
// pass; RS_M, RS_LOGS and RS_H stay where the backward kernel reads them.
__global__ __launch_bounds__(256) void preference_apply_kernel(float* row_stats, int group_rows, int groups, int cap,
                                                               const int32_t* n_pairs_dev, const int32_t* pair,
                                                               const int64_t* targets, long ignore_index, PrefParams Q,
                                                               const float* pair_stats, float* seq_stats) {
  const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (seq >= groups) return;          // uniform per wave
  const int P = pref_pairs(cap, n_pairs_dev);
  const int id = pref_id(pair, seq, P);
  float* ss = seq_stats + (long)seq * 4;
  float g_seq = 0.f, g = 0.f;
  if (id != 0) {                      // uniform per wave
    const int k = id > 0 ? id : -id;
    const float c = ss[1];
    const float w = (Q.by_mean && c > 0.f) ? 1.0f / c : 1.0f;
    g_seq = pair_stats[(long)(k - 1) * 4 + 2] * Q.beta * (id > 0 ? 1.0f : -1.0f) * w;
    g = g_seq;
    if (id > 0 && Q.alpha != 0.f) {
      float N = 0.f;
      for (int b = lane; b < groups; b += 64)
        if (pref_id(pair, b, P) == id) N += seq_stats[(long)b * 4 + 1];
      N = wave_sum(N);
      if (N > 0.f) g -= Q.alpha / N;
    }
  }
  const long r0 = (long)seq * group_rows;
  for (int j = lane; j < group_rows; j += 64) {
    const long r = r0 + j;
    if (targets[r] == ignore_index) continue;
    row_stats[r * 8 + RS_G] = g;
  }
  if (lane == 0) ss[3] = g_seq;
}

}  // namespace bl_policy_impl
using namespace bl_policy_impl;

static bool bad_range(int32_t n, int32_t first, int32_t count) {
  return n <= 0 || (n % 8) || first < 0 || count <= 0 || (first % 8) || (count % 8) || (int64_t)first + count > n;
}

static int policy_forward_check(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                const float* advantages, const float* old_logprob, float temperature, float clip_low,
                                float clip_high, const float* row_stats, const float* stats, int32_t vocab_first,
                                int32_t vocab_count, bool need_old = true) {
  if (!logits || !targets || !advantages || (need_old && !old_logprob) || !row_stats || !stats) return BL_E_ARG;
  if (!(temperature > 0.f) || !(clip_low >= 0.f) || !(clip_high >= 0.f)) return BL_E_ARG;
  if (rows <= 0 || bad_range(n, vocab_first, vocab_count) || (ld % 4) || ld < n) return BL_E_SHAPE;
  if (!bl_aligned16(logits)) return BL_E_ALIGN;
  return BL_OK;
}

// by_wave: a range of at most 256 columns goes to the wave-per-row kernel. The unranged entry point never asks for it.
template <bool SURR = true, bool IS = false>
static void launch_rows(const float* logits, int64_t ld, int32_t rows, const int64_t* targets, int64_t ignore_index,
                        const float* advantages, const float* old_logprob, const float* ref_logprob, const PolicyParams& P,
                        float* row_stats, int32_t vocab_first, int32_t vocab_count, bool by_wave, void* stream,
                        const IsArgs& I = IsArgs{}) {
  if (by_wave && vocab_count <= 256)
    hipLaunchKernelGGL((policy_rows_wave_kernel<SURR, IS>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits,
                       (long)ld, vocab_first, vocab_count, rows, targets, (long)ignore_index, advantages, old_logprob, ref_logprob,
                       P, I, row_stats);
  else
    hipLaunchKernelGGL((policy_rows_kernel<SURR, IS>), dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld,
                       vocab_first, vocab_count, targets, (long)ignore_index, advantages, old_logprob, ref_logprob, P, I, row_stats);
}

static int policy_forward(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                          int64_t ignore_index, const float* advantages, const float* old_logprob, const float* ref_logprob,
                          float temperature, float clip_low, float clip_high, float entropy_coef, float kl_coef,
                          float* row_stats, float* stats, int32_t vocab_first, int32_t vocab_count, bool by_wave, void* stream) {
  const int bad = policy_forward_check(logits, ld, rows, n, targets, advantages, old_logprob, temperature, clip_low, clip_high,
                                       row_stats, stats, vocab_first, vocab_count);
  if (bad != BL_OK) return bad;
  const PolicyParams P = {1.0f / temperature, clip_low, clip_high, entropy_coef, ref_logprob ? kl_coef : 0.f};
  launch_rows(logits, ld, rows, targets, ignore_index, advantages, old_logprob, ref_logprob, P, row_stats, vocab_first,
              vocab_count, by_wave, stream);
  hipLaunchKernelGGL(policy_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_stats, targets, (long)ignore_index,
                     advantages, old_logprob, ref_logprob, P, rows, stats);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_policy_loss_grouped_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                          int64_t ignore_index, const float* advantages, const float* old_logprob,
                                          const float* ref_logprob, float temperature, float clip_low, float clip_high,
                                          float entropy_coef, float kl_coef, float* row_stats, float* stats,
                                          int32_t vocab_first, int32_t vocab_count, int32_t group_rows, int32_t ratio_norm,
                                          float* group_stats, void* stream) {
  const int bad = policy_forward_check(logits, ld, rows, n, targets, advantages, old_logprob, temperature, clip_low, clip_high,
                                       row_stats, stats, vocab_first, vocab_count);
  if (bad != BL_OK) return bad;
  if (!group_stats) return BL_E_ARG;
  if (group_rows <= 0 || (rows % group_rows) || (ratio_norm != 0 && ratio_norm != 1)) return BL_E_SHAPE;
  const PolicyParams P = {1.0f / temperature, clip_low, clip_high, entropy_coef, ref_logprob ? kl_coef : 0.f};
  const int groups = rows / group_rows;
  launch_rows(logits, ld, rows, targets, ignore_index, advantages, old_logprob, ref_logprob, P, row_stats, vocab_first,
              vocab_count, true, stream);
  hipLaunchKernelGGL(policy_group_kernel<false>, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, row_stats, group_rows,
                     groups, ratio_norm, targets, (long)ignore_index, advantages, old_logprob, ref_logprob, P, IsArgs{},
                     group_stats);
  hipLaunchKernelGGL(policy_stats_grouped_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_stats, targets,
                     (long)ignore_index, advantages, ref_logprob, P, rows, group_stats, group_rows, stats);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

// The corrected loss at either level: the launches of the uncorrected form of that level, each in its IS instantiation
// (rows, [groups,] statistics) — no launch more. At action level the row pass's token-level (λ, w) of the valid rows are
// overwritten by the group pass, as ratio, row_loss, clipped and g are.
extern "C" int bl_policy_loss_is_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                     int64_t ignore_index, const float* advantages, const float* old_logprob,
                                     const float* behaviour_logprob, const float* ref_logprob, float temperature, float clip_low,
                                     float clip_high, float entropy_coef, float kl_coef, float* row_stats, float* stats,
                                     int32_t vocab_first, int32_t vocab_count, int32_t group_rows, int32_t ratio_norm,
                                     float* group_stats, float is_cap, float is_mask_low, float is_mask_high, float* is_rows,
                                     float* is_stats, void* stream) {
  const int bad = policy_forward_check(logits, ld, rows, n, targets, advantages, old_logprob, temperature, clip_low, clip_high,
                                       row_stats, stats, vocab_first, vocab_count, false);
  if (bad != BL_OK) return bad;
  if (!behaviour_logprob || !is_rows || !is_stats) return BL_E_ARG;
  if (group_rows >= 0 && (group_stats != nullptr) != (group_rows > 0)) return BL_E_ARG;
  if (!(is_cap > 0.f) || !(is_mask_low >= 0.f) || !(is_mask_low < is_mask_high)) return BL_E_ARG;
  if (group_rows < 0 || (group_rows > 0 && rows % group_rows) || (ratio_norm != 0 && ratio_norm != 1)) return BL_E_SHAPE;
  const PolicyParams P = {1.0f / temperature, clip_low, clip_high, entropy_coef, ref_logprob ? kl_coef : 0.f};
  const IsArgs I = {behaviour_logprob, is_rows, is_cap, is_mask_low, is_mask_high};
  launch_rows<true, true>(logits, ld, rows, targets, ignore_index, advantages, old_logprob, ref_logprob, P, row_stats, vocab_first,
                          vocab_count, true, stream, I);
  if (group_rows > 0) {
    const int groups = rows / group_rows;
    hipLaunchKernelGGL(policy_group_kernel<true>, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, row_stats,
                       group_rows, groups, ratio_norm, targets, (long)ignore_index, advantages, old_logprob, ref_logprob, P, I,
                       group_stats);
  }
  hipLaunchKernelGGL(policy_stats_is_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_stats, targets, (long)ignore_index,
                     advantages, old_logprob, ref_logprob, P, rows, group_stats, group_rows > 0 ? group_rows : 1, stats, I, is_stats);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_policy_loss_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                        int64_t ignore_index, const float* advantages, const float* old_logprob,
                                        const float* ref_logprob, float temperature, float clip_low, float clip_high,
                                        float entropy_coef, float kl_coef, float* row_stats, float* stats,
                                        int32_t vocab_first, int32_t vocab_count, void* stream) {
  return policy_forward(logits, ld, rows, n, targets, ignore_index, advantages, old_logprob, ref_logprob, temperature, clip_low,
                        clip_high, entropy_coef, kl_coef, row_stats, stats, vocab_first, vocab_count, true, stream);
}

extern "C" int bl_policy_loss_backward_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n,
                                                 const int64_t* targets, int64_t ignore_index, const float* row_stats,
                                                 const float* stats, float temperature, float entropy_coef, bl_bf16* dlogits,
                                                 int64_t ldd, int32_t vocab_first, int32_t vocab_count, void* stream) {
  if (!logits || !targets || !row_stats || !stats || !dlogits) return BL_E_ARG;
  if (!(temperature > 0.f)) return BL_E_ARG;
  if (rows <= 0 || bad_range(n, vocab_first, vocab_count) || (ld % 4) || (ldd % 8) || ld < n || ldd < n) return BL_E_SHAPE;
  if (!bl_aligned16(logits) || !bl_aligned16(dlogits)) return BL_E_ALIGN;
  hipLaunchKernelGGL(policy_backward_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, n, targets,
                     (long)ignore_index, row_stats, stats, 1.0f / temperature, entropy_coef, dlogits, (long)ldd, vocab_first,
                     vocab_count);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_policy_loss_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                  int64_t ignore_index, const float* advantages, const float* old_logprob,
                                  const float* ref_logprob, float temperature, float clip_low, float clip_high,
                                  float entropy_coef, float kl_coef, float* row_stats, float* stats, void* stream) {
  return policy_forward(logits, ld, rows, n, targets, ignore_index, advantages, old_logprob, ref_logprob, temperature, clip_low,
                        clip_high, entropy_coef, kl_coef, row_stats, stats, 0, n, false, stream);
}

extern "C" int bl_policy_loss_backward_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                           int64_t ignore_index, const float* row_stats, const float* stats,
                                           float temperature, float entropy_coef, bl_bf16* dlogits, int64_t ldd,
                                           void* stream) {
  return bl_policy_loss_backward_range_f32(logits, ld, rows, n, targets, ignore_index, row_stats, stats, temperature,
                                           entropy_coef, dlogits, ldd, 0, n, stream);
}

extern "C" int bl_preference_loss_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                      int64_t ignore_index, const int32_t* pair, const float* ref_logprob, int32_t n_pairs,
                                      const int32_t* n_pairs_dev, int32_t group_rows, int32_t kind, int32_t seq_norm,
                                      float beta, float label_smoothing, float margin, float sft_coef, float temperature,
                                      float* row_stats, float* stats, float* pair_stats, float* seq_stats,
                                      int32_t vocab_first, int32_t vocab_count, void* stream) {
  if (!logits || !targets || !pair || !row_stats || !stats || !pair_stats || !seq_stats) return BL_E_ARG;
  if (!(temperature > 0.f) || !(beta > 0.f) || !(label_smoothing >= 0.f && label_smoothing < 0.5f) || !(margin >= 0.f) ||
      !(sft_coef >= 0.f) || n_pairs < 1)
    return BL_E_ARG;
  if (rows <= 0 || bad_range(n, vocab_first, vocab_count) || (ld % 4) || ld < n) return BL_E_SHAPE;
  if (group_rows <= 0 || (rows % group_rows) || (seq_norm != 0 && seq_norm != 1)) return BL_E_SHAPE;
  if (kind != PREF_SIGMOID && kind != PREF_IPO && kind != PREF_HINGE) return BL_E_SHAPE;
  if (!bl_aligned16(logits)) return BL_E_ALIGN;
  const PolicyParams P = {1.0f / temperature, 0.f, 0.f, 0.f, 0.f};
  const PrefParams Q = {beta, margin, label_smoothing, sft_coef, kind, seq_norm};
  const int groups = rows / group_rows;
  launch_rows<false>(logits, ld, rows, targets, ignore_index, nullptr, nullptr, nullptr, P, row_stats, vocab_first, vocab_count,
                     true, stream);
  hipLaunchKernelGGL(preference_seq_kernel, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, row_stats, group_rows,
                     groups, seq_norm, targets, (long)ignore_index, ref_logprob, seq_stats);
  hipLaunchKernelGGL(preference_pair_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seq_stats, pair, groups, n_pairs,
                     n_pairs_dev, Q, pair_stats, stats);
  hipLaunchKernelGGL(preference_apply_kernel, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, row_stats, group_rows,
                     groups, n_pairs, n_pairs_dev, pair, targets, (long)ignore_index, Q, pair_stats, seq_stats);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
