// distill.hip — the distribution-matching (distillation) loss over fp32 logits rows: forward KL, reverse KL or the
// generalised Jensen-Shannon divergence between the student's softmax over a token range and a TEACHER ROW of the same
// width (the 256 action bins of an OpenVLA token), plus sft_coef times the target's negative log-likelihood. The fourth
// loss the training step can plan, beside the cross-entropy (glue.hip / train.hip) and the policy and preference losses
// (policy.hip). bridgelang_amd/training/distill_loss.py is the fp64 definition; these kernels are its fp32 twin to a
// tolerance (expf / logf). tests/distill_ref64.py derives the per-element bounds from the chains written down here.
//
// Conventions are policy.hip's: targets[row] = token of the NEXT position, ignore_index rows contribute nothing and
// neither their logits nor their teacher row are read, 16-byte accesses, deterministic reductions, no float atomics. The
// teacher is fp32 [rows, count] in ROW layout (row r of the step holds its own teacher row, column j is token first + j):
// the kernels index it with the row they already have, no gather, and a captured graph serves any labelling.
//
// Forward, launch 1: the row pass. One workgroup per row (distill_rows_kernel), or for a range of at most 256 columns ONE
// WAVE per row, four rows per workgroup, no barrier (distill_rows_wave_kernel: the lane's float4 of logits and float4 of
// the teacher stay in registers across the passes). Thread t owns the float4s at columns 4t + 1024k, k ascending, and
// inside a float4 the elements ascending; every sum below is accumulated in that order per thread, then wave_sum (xor
// butterfly), then the four waves' LDS slots folded 0 + 1 + 2 + 3. In the wave form waves 1-3 do not exist and their
// slots are literal + 0.f: up to 256 columns both forms add the same numbers in the same order.
//   pass 1   max(l); m = max·inv_t                                               (policy.hip to the letter)
//   pass 2   d = l·inv_t − m, ex = expf(d): S += ex, W += ex·d                    (policy.hip to the letter)
//            Q += q, E += q·logf(q) [q > 0], IQ += i·q, the first argmax of q and of l (integer keys, bl_common.h)
//   then     log S = logf(S) (every thread computes it from the same folded S)
//   pass 3   ONE MORE PASS over the same columns with log S known (registers in the wave form, a re-read in the
//            workgroup form): lp = d − log S, p = expf(lp), IP += i·p and
//              forward_kl   A += q·(logf(q) − lp) [q > 0]                         D = A            c = Q
//              reverse_kl   A += p·(lp − logf(q))                                 D = A            c = A
//              jsd          mi = β·q + (1 − β)·p, lm = logf(mi)
//                           A += q·(logf(q) − lm) [q > 0],  C += p·((1 − β)·(lp − lm)) [p > 0]
//                                                                                 D = β·A + C      c = C
//   The sums are NOT expanded algebraically (Σ p·u as (Σ ex·u) / S and so on): the third pass keeps every term the
//   definition's own, so a row whose teacher equals its student gives terms that vanish one by one.
//   finish   thread 0: H = log S − W / S, logp = z_a − m − log S (policy.hip's finish_row), D, c, agree, and between the
//            two launches −E (the teacher's entropy) in the row_loss slot and |IP − IQ| (the bin gap) in the agree slot,
//            carrying agree as its sign bit.
// Forward, launch 2: distill_stats_kernel, one workgroup. Thread t takes rows t, t + 256, … ascending: it reads the two
// stashed values, writes row_loss = D + sft_coef·(−logp) and agree = 0 / 1 in their place, and accumulates the seven means
// (wave_sum, four slots, one division). Every row ignored: every statistic is exactly 0. After the two launches every
// element of row_stats and stats has been written.
//
// Backward: distill_backward_kernel, one workgroup per row with a column window as policy_backward_kernel. It reads the
// row's logits and its teacher row once, m, log S and c from row_stats and n_valid from stats[1], and writes the whole
// [rows, n] bf16 row through pack8: +0 outside the range and on ignored rows.
//
// A target outside the range gives NaN in that row's logp (never a stray read); a teacher zero under reverse_kl gives inf
// or NaN in that row. Both are caller errors the host front end refuses.
#include "bl_common.h"
#include <math.h>

namespace bl_distill_impl {

// per-row statistics, fp32 [rows, 8]; logp, m and log S where policy.hip has them
enum { RS_LOGP = 0, RS_H, RS_DIV, RS_LOSS, RS_AGREE, RS_M, RS_LOGS, RS_C };
enum { KIND_FORWARD = 0, KIND_REVERSE = 1, KIND_JSD = 2 };

struct DistillParams {
  float inv_t, beta, omb, sft_coef;   // omb = 1 − β
  int kind;
};

// the per-thread partial sums of pass 2 that belong to the teacher, and the two argmax holders
struct TeacherAcc {
  float Q, E, IQ;
  int qk, qi, lk, li;
};
__device__ __forceinline__ TeacherAcc teacher_acc_init() { return {0.f, 0.f, 0.f, (int)0x80000000, 0x7fffffff, (int)0x80000000, 0x7fffffff}; }

// pass 2 on one column i (relative to the range) with logit l and teacher q
__device__ __forceinline__ void pass2_col(int i, float l, float q, TeacherAcc& t) {
  t.Q += q;
  if (q > 0.f) t.E += q * logf(q);
  t.IQ += (float)i * q;
  argmax_take_next(argmax_key(q), i, t.qk, t.qi);
  argmax_take_next(argmax_key(l), i, t.lk, t.li);
}

// pass 3 on one column: d = z − m as pass 2 formed it
__device__ __forceinline__ void pass3_col(int i, float d, float q, float logS, const DistillParams& P, float& A, float& C, float& IP) {
  const float lp = d - logS;
  const float p = expf(lp);
  IP += (float)i * p;
  if (P.kind == KIND_FORWARD) {
    if (q > 0.f) A += q * (logf(q) - lp);
  } else if (P.kind == KIND_REVERSE) {
    A += p * (lp - logf(q));             // p = 0 (underflow) times a finite u is 0
  } else {
    const float mi = P.beta * q + P.omb * p;
    const float lm = logf(mi);
    if (q > 0.f) A += q * (logf(q) - lm);
    if (p > 0.f) C += p * (P.omb * (lp - lm));
  }
}

// the first argmax across the lanes of a wave: the larger key, among equal keys the lower index
__device__ __forceinline__ void wave_argmax(int& k, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ok = __shfl_xor(k, o, 64), oi = __shfl_xor(i, o, 64);
    argmax_take(ok, oi, k, i);
  }
}

// what thread 0 / lane 0 does once every sum of a row is known. lr points at column `first`; tgt is relative to it.
__device__ __forceinline__ void finish_row(const float* lr, int n, long tgt, float m, float S, float W, float logS, float Q,
                                           float E, float IQ, float IP, float A, float C, bool agree, const DistillParams& P,
                                           float* rs) {
  const float H = logS - W / S;                                       // −Σ p·logp, logp = (z − m) − log S
  const float za = (tgt >= 0 && tgt < n) ? lr[tgt] * P.inv_t : NAN;    // a token outside the row: NaN, never a stray read
  float D = A, c = Q;
  if (P.kind == KIND_REVERSE) c = A;
  if (P.kind == KIND_JSD) {
    D = P.beta * A + C;
    c = C;
  }
  rs[RS_LOGP] = za - m - logS;
  rs[RS_H] = H;
  rs[RS_DIV] = D;
  rs[RS_LOSS] = -E;                                                   // until the statistics kernel: the teacher's entropy
  rs[RS_AGREE] = copysignf(fabsf(IP - IQ), agree ? 1.f : -1.f);       // until the statistics kernel: the bin gap, agree in its sign
  rs[RS_M] = m;
  rs[RS_LOGS] = logS;
  rs[RS_C] = c;
}

// one workgroup per row; the row is the n columns from column `first` on
__global__ __launch_bounds__(256) void distill_rows_kernel(const float* logits, long ld, int first, int n, const int64_t* targets,
                                                           long ignore_index, const float* teacher, long ldt, DistillParams P,
                                                           float* row_stats) {
  __shared__ float red_m[4], red_s[4], red_w[4], red_q[4], red_e[4], red_iq[4], red_ip[4], red_a[4], red_c[4];
  __shared__ int red_k[4][4];
  const int row = blockIdx.x;
  const long tgt = targets[row];
  float* rs = row_stats + (long)row * 8;
  if (tgt == ignore_index) {          // uniform per workgroup
    if (threadIdx.x < 8) rs[threadIdx.x] = 0.f;
    return;
  }
  const float* lr = logits + (long)row * ld + first;
  const float* tr = teacher + (long)row * ldt;
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
  TeacherAcc t = teacher_acc_init();
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4_t l = *(const f32x4_t*)(lr + i);
    const f32x4_t q = *(const f32x4_t*)(tr + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = l[e] * P.inv_t - m;
      const float ex = expf(d);
      s += ex;
      w += ex * d;                    // exp underflows to 0 long before d overflows: 0·d = 0
      pass2_col(i + e, l[e], q[e], t);
    }
  }
  s = wave_sum(s);
  w = wave_sum(w);
  t.Q = wave_sum(t.Q);
  t.E = wave_sum(t.E);
  t.IQ = wave_sum(t.IQ);
  wave_argmax(t.qk, t.qi);
  wave_argmax(t.lk, t.li);
  if ((threadIdx.x & 63) == 0) {
    red_s[wave] = s; red_w[wave] = w; red_q[wave] = t.Q; red_e[wave] = t.E; red_iq[wave] = t.IQ;
    red_k[wave][0] = t.qk; red_k[wave][1] = t.qi; red_k[wave][2] = t.lk; red_k[wave][3] = t.li;
  }
  __syncthreads();
  const float S = red_s[0] + red_s[1] + red_s[2] + red_s[3];
  const float logS = logf(S);
  float A = 0.f, C = 0.f, IP = 0.f;
  for (int i = threadIdx.x * 4; i < n; i += 1024) {
    const f32x4_t l = *(const f32x4_t*)(lr + i);
    const f32x4_t q = *(const f32x4_t*)(tr + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) pass3_col(i + e, l[e] * P.inv_t - m, q[e], logS, P, A, C, IP);
  }
  A = wave_sum(A);
  C = wave_sum(C);
  IP = wave_sum(IP);
  if ((threadIdx.x & 63) == 0) { red_a[wave] = A; red_c[wave] = C; red_ip[wave] = IP; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int qk = red_k[0][0], qi = red_k[0][1], lk = red_k[0][2], li = red_k[0][3];
#pragma unroll
    for (int v = 1; v < 4; ++v) {
      argmax_take(red_k[v][0], red_k[v][1], qk, qi);
      argmax_take(red_k[v][2], red_k[v][3], lk, li);
    }
    finish_row(lr, n, tgt - first, m, S, red_w[0] + red_w[1] + red_w[2] + red_w[3], logS, red_q[0] + red_q[1] + red_q[2] + red_q[3],
               red_e[0] + red_e[1] + red_e[2] + red_e[3], red_iq[0] + red_iq[1] + red_iq[2] + red_iq[3],
               red_ip[0] + red_ip[1] + red_ip[2] + red_ip[3], red_a[0] + red_a[1] + red_a[2] + red_a[3],
               red_c[0] + red_c[1] + red_c[2] + red_c[3], qi == li, P, rs);
  }
}

// n <= 256: one wave per row, four rows per workgroup, the lane's two float4s stay in registers across the three passes.
// The order of every sum is the workgroup kernel's on such a row (there waves 1–3 hold no column and add zeros).
__global__ __launch_bounds__(256) void distill_rows_wave_kernel(const float* logits, long ld, int first, int n, int rows,
                                                                const int64_t* targets, long ignore_index, const float* teacher,
                                                                long ldt, DistillParams P, float* row_stats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;            // uniform per wave, and the kernel has no barrier
  const long tgt = targets[row];
  float* rs = row_stats + (long)row * 8;
  if (tgt == ignore_index) {
    if (lane < 8) rs[lane] = 0.f;
    return;
  }
  const float* lr = logits + (long)row * ld + first;
  const bool on = lane * 4 < n;       // n % 4 == 0: a lane's four columns are inside together
  f32x4_t l = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, q = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    l = *(const f32x4_t*)(lr + lane * 4);
    q = *(const f32x4_t*)(teacher + (long)row * ldt + lane * 4);
  }
  const float m = wave_max(fmaxf(fmaxf(-INFINITY, fmaxf(l[0], l[1])), fmaxf(l[2], l[3]))) * P.inv_t;
  float s = 0.f, w = 0.f;
  TeacherAcc t = teacher_acc_init();
  if (on) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = l[e] * P.inv_t - m;
      const float ex = expf(d);
      s += ex;
      w += ex * d;
      pass2_col(lane * 4 + e, l[e], q[e], t);
    }
  }
  s = wave_sum(s);
  w = wave_sum(w);
  t.Q = wave_sum(t.Q);
  t.E = wave_sum(t.E);
  t.IQ = wave_sum(t.IQ);
  wave_argmax(t.qk, t.qi);
  wave_argmax(t.lk, t.li);
  const float S = s + 0.f + 0.f + 0.f;
  const float logS = logf(S);
  float A = 0.f, C = 0.f, IP = 0.f;
  if (on) {
#pragma unroll
    for (int e = 0; e < 4; ++e) pass3_col(lane * 4 + e, l[e] * P.inv_t - m, q[e], logS, P, A, C, IP);
  }
  A = wave_sum(A);
  C = wave_sum(C);
  IP = wave_sum(IP);
  if (lane == 0)
    finish_row(lr, n, tgt - first, m, S, w + 0.f + 0.f + 0.f, logS, t.Q + 0.f + 0.f + 0.f, t.E + 0.f + 0.f + 0.f, t.IQ + 0.f + 0.f + 0.f,
               IP + 0.f + 0.f + 0.f, A + 0.f + 0.f + 0.f, C + 0.f + 0.f + 0.f, t.qi == t.li, P, rs);
}

// The 8 step statistics: means over valid rows (single workgroup, fixed summation order → deterministic). It also turns
// the two values the row pass stashed (the teacher's entropy, the signed bin gap) into row_loss and agree: thread t is the
// only one that touches its rows.
__global__ __launch_bounds__(256) void distill_stats_kernel(float* row_stats, const int64_t* targets, long ignore_index,
                                                            float sft_coef, int rows, float* out) {
  constexpr int NS = 7;
  __shared__ float rsum[4][NS];
  __shared__ int rc[4];
  float a[NS];                        // row_loss, D, H, teacher entropy, agree, nll, bin gap
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < rows; i += 256) {
    if (targets[i] == ignore_index) continue;
    float* rs = row_stats + (long)i * 8;
    const float te = rs[RS_LOSS], sg = rs[RS_AGREE];
    const float nll = -rs[RS_LOGP];
    const float loss = rs[RS_DIV] + sft_coef * nll;
    const float agree = __builtin_signbit(sg) ? 0.f : 1.f;
    rs[RS_LOSS] = loss;
    rs[RS_AGREE] = agree;
    a[0] += loss;
    a[1] += rs[RS_DIV];
    a[2] += rs[RS_H];
    a[3] += te;
    a[4] += agree;
    a[5] += nll;
    a[6] += fabsf(sg);
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
    out[k == 0 ? 0 : k + 1] = cnt > 0 ? (rsum[0][k] + rsum[1][k] + rsum[2][k] + rsum[3][k]) / (float)cnt : 0.f;
    if (k == 0) out[1] = (float)cnt;
  }
}

__device__ __forceinline__ u32x4_t pack8(const float* v) {
  u32x4_t q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = pack2bf(v[2 * i], v[2 * i + 1]);
  return q;
}

// dlogits_i = [ ∂D/∂z_i + sft_coef·(p_i − δ_ia) ] / (T · n_valid): one read of the row and of its teacher row; logp_i by
// arithmetic (z_i − m − log S). The 8-column groups outside [first, first + count) are written as zeros and never read.
__global__ __launch_bounds__(256) void distill_backward_kernel(const float* logits, long ld, int n, const int64_t* targets,
                                                               long ignore_index, const float* teacher, long ldt,
                                                               const float* row_stats, const float* stats, DistillParams P,
                                                               uint16_t* dlogits, long ldd, int first, int count) {
  const int row = blockIdx.x;
  const long tgt = targets[row];
  uint16_t* dr = dlogits + (long)row * ldd;
  if (tgt == ignore_index) {
    for (int i = threadIdx.x * 8; i < n; i += 2048) *(u32x4_t*)(dr + i) = (u32x4_t){0u, 0u, 0u, 0u};
    return;
  }
  const float* lr = logits + (long)row * ld;
  const float* tr = teacher + (long)row * ldt;            // column j of the teacher is column first + j of the row
  const float* rs = row_stats + (long)row * 8;
  const float c = rs[RS_C];
  const float off = rs[RS_M] + rs[RS_LOGS];
  const float scale = P.inv_t / stats[1];                 // 1 / (T · n_valid)
  for (int i = threadIdx.x * 8; i < n; i += 2048) {
    if (i < first || i - first >= count) {
      *(u32x4_t*)(dr + i) = (u32x4_t){0u, 0u, 0u, 0u};
      continue;
    }
    const f32x4_t a = *(const f32x4_t*)(lr + i), b = *(const f32x4_t*)(lr + i + 4);
    const f32x4_t qa = *(const f32x4_t*)(tr + (i - first)), qb = *(const f32x4_t*)(tr + (i - first) + 4);
    float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    const float q[8] = {qa[0], qa[1], qa[2], qa[3], qb[0], qb[1], qb[2], qb[3]};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float lp = v[e] * P.inv_t - off;
      const float p = expf(lp);
      float dz;
      if (P.kind == KIND_FORWARD) {
        dz = p * c - q[e];
      } else if (P.kind == KIND_REVERSE) {
        dz = p * ((lp - logf(q[e])) - c);
      } else {
        const float mi = P.beta * q[e] + P.omb * p;
        dz = p > 0.f ? p * (P.omb * (lp - logf(mi)) - c) : 0.f;
      }
      v[e] = (dz + P.sft_coef * (p - ((long)(i + e) == tgt ? 1.f : 0.f))) * scale;
    }
    *(u32x4_t*)(dr + i) = pack8(v);
  }
}

}  // namespace bl_distill_impl
using namespace bl_distill_impl;

static bool distill_bad_range(int32_t n, int32_t first, int32_t count) {
  return n <= 0 || (n % 8) || first < 0 || count <= 0 || (first % 8) || (count % 8) || (int64_t)first + count > n;
}

// the checks both entry points share; BL_OK, or the code of the first rule broken
static int distill_check(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets, const float* teacher,
                         int64_t ldt, const float* row_stats, const float* stats, int32_t kind, float beta, float sft_coef,
                         float temperature, int32_t vocab_first, int32_t vocab_count) {
  if (!logits || !targets || !teacher || !row_stats || !stats) return BL_E_ARG;
  if (kind != KIND_FORWARD && kind != KIND_REVERSE && kind != KIND_JSD) return BL_E_ARG;
  if (kind == KIND_JSD && !(beta > 0.f && beta < 1.f)) return BL_E_ARG;
  if (!(temperature > 0.f) || !(sft_coef >= 0.f)) return BL_E_ARG;
  if (rows <= 0 || distill_bad_range(n, vocab_first, vocab_count) || (ld % 4) || ld < n || (ldt % 4) || ldt < vocab_count)
    return BL_E_SHAPE;
  if (!bl_aligned16(logits) || !bl_aligned16(teacher)) return BL_E_ALIGN;
  return BL_OK;
}

extern "C" int bl_distill_loss_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                   int64_t ignore_index, const float* teacher, int64_t ldt, int32_t kind, float beta,
                                   float sft_coef, float temperature, float* row_stats, float* stats, int32_t vocab_first,
                                   int32_t vocab_count, void* stream) {
  const int bad = distill_check(logits, ld, rows, n, targets, teacher, ldt, row_stats, stats, kind, beta, sft_coef, temperature,
                                vocab_first, vocab_count);
  if (bad != BL_OK) return bad;
  const DistillParams P = {1.0f / temperature, beta, 1.0f - beta, sft_coef, kind};
  if (vocab_count <= 256)
    hipLaunchKernelGGL(distill_rows_wave_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, (long)ld,
                       vocab_first, vocab_count, rows, targets, (long)ignore_index, teacher, (long)ldt, P, row_stats);
  else
    hipLaunchKernelGGL(distill_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, vocab_first,
                       vocab_count, targets, (long)ignore_index, teacher, (long)ldt, P, row_stats);
  hipLaunchKernelGGL(distill_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_stats, targets, (long)ignore_index,
                     sft_coef, rows, stats);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_distill_loss_backward_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                            int64_t ignore_index, const float* teacher, int64_t ldt, const float* row_stats,
                                            const float* stats, int32_t kind, float beta, float sft_coef, float temperature,
                                            bl_bf16* dlogits, int64_t ldd, int32_t vocab_first, int32_t vocab_count,
                                            void* stream) {
  if (!dlogits) return BL_E_ARG;
  const int bad = distill_check(logits, ld, rows, n, targets, teacher, ldt, row_stats, stats, kind, beta, sft_coef, temperature,
                                vocab_first, vocab_count);
  if (bad != BL_OK) return bad;
  if ((ldd % 8) || ldd < n) return BL_E_SHAPE;
  if (!bl_aligned16(dlogits)) return BL_E_ALIGN;
  const DistillParams P = {1.0f / temperature, beta, 1.0f - beta, sft_coef, kind};
  hipLaunchKernelGGL(distill_backward_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, n, targets,
                     (long)ignore_index, teacher, (long)ldt, row_stats, stats, P, dlogits, (long)ldd, vocab_first, vocab_count);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
