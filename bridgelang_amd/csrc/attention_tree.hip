// attention_tree.hip — attention over a shared prompt and its branches (the shared-prompt training step),
// forward with log-sum-exp and backward, plus the rotary embedding at per-row positions that layout needs.
//
// One row of the layout per batch element:   prefix (rows [0, prefix))  ‖  branch 0 (`branch` rows)  ‖ … ‖  branch G-1
// Key j is visible to query i iff key_mask[j], j <= i, and (j < prefix, or i and j lie in the same branch). Every branch
// therefore reads the prefix K / V rows IN PLACE — there is no K / V copy per branch — and the backward of a prefix key sums
// over the prefix queries and every branch's queries in one fixed order inside one wave: no atomics, no workspace.
//
// The kernels are the streaming forms of attention.hip (attn_fwd_kernel: 64 query rows per workgroup, 64-key chunks through
// LDS, online softmax) and attention_bwd.hip (the chunked dq / dkv kernels: 128 register-side rows per workgroup, 256-row
// chunks of the LDS-side operand, P recomputed from the stored log-sum-exp) with the tree predicate in place of the causal
// one, so any prefix + G·branch up to model_max_length runs. What the tree hides is skipped, not just masked: a
// workgroup skips the chunks and a wave the 32-row steps in which none of its rows can see anything — the other branches. A
// skipped step would have contributed P = 0 exactly (forward: exp2(-inf); backward: P is a select), so skipping changes no bit.
// Same arithmetic contract as bl_attention_lse_bf16 / bl_attention_backward_bf16: fp32 scores and softmax, bf16 P and dS into
// the MFMA, base-2 lse, dq / dk / dv on q's / k's / v's strides. head_dim 128 only (the Llama decoder).
#include "bl_common.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>

namespace bl_attention_tree_impl {
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

struct TreeArgs {
  const uint16_t *q, *k, *v, *o, *dout;
  uint16_t *out, *dq, *dk, *dv;
  const uint8_t* mask;
  float* lse;              // written by the forward, read by the backward
  float* delta;
  long q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs, o_bs, o_hs, o_rs, mask_bs;
  int B, H, S, prefix, branch, stat_rs;
  float scale, scale_log2e;
};

constexpr int HD = 128, KS = 4, KCH = 16, DT = 8;

// first row of the branch that holds row i (i >= prefix); for a prefix row: `prefix` (no branch key is at or below it)
__device__ __forceinline__ int branch_lo(int i, int prefix, int branch) {
  return i < prefix ? prefix : prefix + (i - prefix) / branch * branch;
}
// one past the last row of the branch that holds row j (j >= prefix); for a prefix row: S (every later query may see it)
__device__ __forceinline__ int branch_hi(int j, int prefix, int branch, int S) {
  return j < prefix ? S : min(S, prefix + ((j - prefix) / branch + 1) * branch);
}

// ---- forward: attn_fwd_kernel<128, causal> of attention.hip under the tree predicate -------------------------------------
constexpr int KV_CHUNK = 64;
constexpr int KROW = HD * 2 + 16;          // LDS bytes per K / V row (padded against bank conflicts)

__global__ __launch_bounds__(256) void tree_fwd_kernel(TreeArgs p) {
  __shared__ __attribute__((aligned(16))) char k_lds[KV_CHUNK * KROW];
  __shared__ __attribute__((aligned(16))) char v_lds[KV_CHUNK * KROW];
  __shared__ __attribute__((aligned(16))) uint8_t m_lds[KV_CHUNK];       // visibility of the staged keys (in range, not masked)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64;
  const int qrow = q0 + wave * 16 + l15;
  const int qlo = branch_lo(qrow, p.prefix, p.branch);                   // this lane's query sees keys < prefix and [qlo, qrow]
  const int blk_lo = branch_lo(q0, p.prefix, p.branch);                  // lowest branch row any query of the workgroup sees

  for (int i = tid; i < (int)sizeof(k_lds) / 16; i += 256) ((u32x4_t*)k_lds)[i] = (u32x4_t){0u, 0u, 0u, 0u};
  for (int i = tid; i < (int)sizeof(v_lds) / 16; i += 256) ((u32x4_t*)v_lds)[i] = (u32x4_t){0u, 0u, 0u, 0u};

  bf16x8_t qf[KS];
  {
    const uint16_t* qp = p.q + (long)b * p.q_bs + (long)h * p.q_hs + (long)qrow * p.q_rs;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4_t t = {0u, 0u, 0u, 0u};
      if (qrow < p.S) t = *(const u32x4_t*)(qp + (lg + 4 * ks) * 8);
      qf[ks] = __builtin_bit_cast(bf16x8_t, t);
    }
  }
  f32x4_t o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_part = 0.f;

  const int kv_end = min(p.S, q0 + 64);
  const int nchunk = (kv_end + KV_CHUNK - 1) / KV_CHUNK;
  const uint16_t* kbase = p.k + (long)b * p.k_bs + (long)h * p.k_hs;
  const uint16_t* vbase = p.v + (long)b * p.v_bs + (long)h * p.v_hs;
  const uint8_t* mrow = p.mask ? p.mask + (long)b * p.mask_bs : nullptr;

  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int key0 = c * KV_CHUNK;
    if (key0 >= p.prefix && key0 + KV_CHUNK <= blk_lo) continue;         // other branches only (uniform over the workgroup)
    for (int piece = tid; piece < KV_CHUNK * KCH; piece += 256) {
      const int key = piece / KCH, ch = piece - key * KCH;
      u32x4_t t = {0u, 0u, 0u, 0u}, u = {0u, 0u, 0u, 0u};
      if (key0 + key < p.S) {
        t = *(const u32x4_t*)(kbase + (long)(key0 + key) * p.k_rs + ch * 8);
        u = *(const u32x4_t*)(vbase + (long)(key0 + key) * p.v_rs + ch * 8);
      }
      *(u32x4_t*)(k_lds + key * KROW + ch * 16) = t;
      *(u32x4_t*)(v_lds + key * KROW + ch * 16) = u;
    }
    if (tid < KV_CHUNK) m_lds[tid] = (key0 + tid < p.S && (mrow == nullptr || mrow[key0 + tid] != 0)) ? 1 : 0;
    __syncthreads();

    // S^T = K · Q^T : lane owns query column l15 and keys 16*kt + 4*lg + r
    float s[4][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8_t kf = *(const bf16x8_t*)(k_lds + (kt * 16 + l15) * KROW + (lg + 4 * ks) * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
      }
      const uint32_t vis4 = *(const uint32_t*)(m_lds + kt * 16 + lg * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + kt * 16 + lg * 4 + r;
        const bool vis = ((vis4 >> (8 * r)) & 0xffu) != 0 && key <= qrow && (key < p.prefix || key >= qlo);
        s[kt][r] = vis ? acc[r] * p.scale_log2e : -INFINITY;
      }
    }
    // online softmax (base-2 domain)
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);   // m_run = -inf → 0
    m_run = m_new;
    float psum = 0.f;
    bf16x8_t pf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        e[j] = __builtin_amdgcn_exp2f(s[2 * s2 + (j >> 2)][j & 3] - m_use);
        psum += e[j];
      }
      u32x4_t t;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = pack2bf(e[2 * j], e[2 * j + 1]);
      pf[s2] = __builtin_bit_cast(bf16x8_t, t);
    }
    l_part = l_part * alpha + psum;
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] *= alpha;

    // O^T += V^T · P^T : element j of lane group lg ↔ key 32*s2 + 16*(j>>2) + 4*lg + (j&3) on both operands
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const char* vp = v_lds + (32 * s2 + 4 * lg + (l15 >> 2)) * KROW + (dt * 16 + (l15 & 3) * 4) * 2;
        const s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)vp);
        const s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(vp + 16 * KROW));
        const u32x2_t w0 = __builtin_bit_cast(u32x2_t, v0), w1 = __builtin_bit_cast(u32x2_t, v1);
        const u32x4_t vv = {w0[0], w0[1], w1[0], w1[1]};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vv), pf[s2], o[dt], 0, 0, 0);
      }
    }
    __syncthreads();   // everyone done with this chunk before it is overwritten
  }

  float l = l_part;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  if (lg == 0 && qrow < p.S)
    p.lse[((long)b * p.H + h) * p.stat_rs + qrow] = l > 0.f ? m_run + __builtin_amdgcn_logf(l) : INFINITY;
  if (qrow < p.S) {
    uint16_t* op = p.out + (long)b * p.o_bs + (long)h * p.o_hs + (long)qrow * p.o_rs;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      u32x2_t w;
      w[0] = pack2bf(o[dt][0] * inv, o[dt][1] * inv);
      w[1] = pack2bf(o[dt][2] * inv, o[dt][3] * inv);
      *(u32x2_t*)(op + dt * 16 + lg * 4) = w;
    }
  }
}

// ---- backward: the chunked dq / dkv kernels of attention_bwd.hip under the tree predicate --------------------------------
constexpr int KC = 256, ROWB = 256, MASK = ROWB / 16 - 1;

// stage `rows` rows (128 bf16 each) of two operands into LDS at chunk' = chunk ^ (row & MASK); rows >= n_valid are zero
__device__ __forceinline__ void stage_two(char* a_lds, char* b_lds, const uint16_t* a, long a_rs, const uint16_t* b, long b_rs,
                                          int rows, int n_valid, int tid) {
  constexpr int CH = ROWB / 16, UNR = 4;
  const int npieces = rows * CH;
  for (int base = tid; base < npieces; base += 512 * UNR) {
    u32x4_t aq[UNR], bq[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int piece = base + u * 512, row = piece / CH, ch = piece - row * CH;
      aq[u] = (u32x4_t){0u, 0u, 0u, 0u};
      bq[u] = (u32x4_t){0u, 0u, 0u, 0u};
      if (piece < npieces && row < n_valid) {
        aq[u] = *(const u32x4_t*)(a + (long)row * a_rs + ch * 8);
        bq[u] = *(const u32x4_t*)(b + (long)row * b_rs + ch * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int piece = base + u * 512, row = piece / CH, ch = piece - row * CH;
      if (piece < npieces) {
        *(u32x4_t*)(a_lds + row * ROWB + ((ch ^ (row & MASK)) << 4)) = aq[u];
        *(u32x4_t*)(b_lds + row * ROWB + ((ch ^ (row & MASK)) << 4)) = bq[u];
      }
    }
  }
}

// transposed 16(d) × 32(row) fragment of a row-major LDS operand: MFMA "A" operand T[d = 16*dt + l15][rows row0 ..],
// element j of lane group lg ↔ row row0 + 16*(j>>2) + 4*lg + (j&3)
__device__ __forceinline__ bf16x8_t tr_frag(const char* lds, int row0, int dt, int l15, int lg) {
  const int row = row0 + 4 * lg + (l15 >> 2);                 // (row + 16) & MASK == row & MASK
  const int ch = dt * 2 + ((l15 & 3) >> 1);
  const char* vp = lds + row * ROWB + ((ch ^ (row & MASK)) << 4) + (l15 & 1) * 8;
  const s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)vp);
  const s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(vp + 16 * ROWB));
  const u32x2_t w0 = __builtin_bit_cast(u32x2_t, v0), w1 = __builtin_bit_cast(u32x2_t, v1);
  const u32x4_t vv = {w0[0], w0[1], w1[0], w1[1]};
  return __builtin_bit_cast(bf16x8_t, vv);
}

__device__ __forceinline__ bf16x8_t row_frag(const char* lds, int row, int ch) {
  return *(const bf16x8_t*)(lds + row * ROWB + ((ch ^ (row & MASK)) << 4));
}

__device__ __forceinline__ bf16x8_t pack8(const float* e) {
  u32x4_t t;
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = pack2bf(e[2 * j], e[2 * j + 1]);
  return __builtin_bit_cast(bf16x8_t, t);
}

// dq (and delta = rowsum(dO ∘ O)): a workgroup owns 128 query rows (one 16-row tile per wave), K and V stream through LDS
__global__ __launch_bounds__(512) void tree_bwd_dq_kernel(TreeArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;
  char* v_lds = smem + KC * ROWB;
  uint8_t* m_lds = (uint8_t*)(smem + 2 * KC * ROWB);          // key visibility of the staged chunk, one byte per key
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  const uint8_t* mrow = p.mask ? p.mask + (long)b * p.mask_bs : nullptr;
  const uint16_t* kbase = p.k + (long)b * p.k_bs + (long)h * p.k_hs;
  const uint16_t* vbase = p.v + (long)b * p.v_bs + (long)h * p.v_hs;

  const int q0 = (blockIdx.y * 8 + wave) * 16, qrow = q0 + l15;          // tiles past the end: every guard below is false
  const int kv_hi = q0 < p.S ? min(p.S, q0 + 16) : 0;
  const int block_hi = min(p.S, (int)blockIdx.y * 128 + 128);
  const int qlo = branch_lo(min(qrow, p.S - 1), p.prefix, p.branch);     // this lane's query sees keys < prefix and [qlo, qrow]
  const int wave_lo = branch_lo(min(q0, p.S - 1), p.prefix, p.branch);   // lowest branch row the wave's tile sees
  const int blk_lo = branch_lo((int)blockIdx.y * 128, p.prefix, p.branch);

  bf16x8_t qf[KS], dof[KS];
  float dsum = 0.f;
  {
    const uint16_t* qp = p.q + (long)b * p.q_bs + (long)h * p.q_hs + (long)qrow * p.q_rs;
    const long oo = (long)b * p.o_bs + (long)h * p.o_hs + (long)qrow * p.o_rs;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int ch = lg + 4 * ks;
      u32x4_t t = {0u, 0u, 0u, 0u}, g = {0u, 0u, 0u, 0u}, ov = {0u, 0u, 0u, 0u};
      if (qrow < p.S) {
        t = *(const u32x4_t*)(qp + ch * 8);
        g = *(const u32x4_t*)(p.dout + oo + ch * 8);
        ov = *(const u32x4_t*)(p.o + oo + ch * 8);
      }
      qf[ks] = __builtin_bit_cast(bf16x8_t, t);
      dof[ks] = __builtin_bit_cast(bf16x8_t, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) dsum += bflo(g[i]) * bflo(ov[i]) + bfhi(g[i]) * bfhi(ov[i]);
    }
  }
  dsum += __shfl_xor(dsum, 16, 64);
  dsum += __shfl_xor(dsum, 32, 64);
  const long stat = ((long)b * p.H + h) * p.stat_rs + qrow;
  if (lg == 0 && qrow < p.S) p.delta[stat] = dsum;
  const float lse_q = qrow < p.S ? p.lse[stat] : INFINITY;

  f32x4_t acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int key0 = 0; key0 < block_hi; key0 += KC) {
    if (key0 >= p.prefix && key0 + KC <= blk_lo) continue;       // other branches only (uniform over the workgroup)
    __syncthreads();                                              // the previous chunk has been consumed by every wave
    stage_two(k_lds, v_lds, kbase + (long)key0 * p.k_rs, p.k_rs, vbase + (long)key0 * p.v_rs, p.v_rs, KC, min(KC, p.S - key0), tid);
    if (tid < KC) m_lds[tid] = (key0 + tid < p.S && (mrow == nullptr || mrow[key0 + tid] != 0)) ? 1 : 0;
    __syncthreads();
#pragma unroll 1
    for (int s2 = 0; s2 < KC / 32 && key0 + s2 * 32 < kv_hi; ++s2) {
      const int ks0 = key0 + s2 * 32;
      if (ks0 >= p.prefix && ks0 + 32 <= wave_lo) continue;      // other branches only (uniform over the wave)
      float e[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int kt = 2 * s2 + half;
        f32x4_t as = {0.f, 0.f, 0.f, 0.f}, ap = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          as = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(k_lds, kt * 16 + l15, lg + 4 * ks), qf[ks], as, 0, 0, 0);
          ap = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(v_lds, kt * 16 + l15, lg + 4 * ks), dof[ks], ap, 0, 0, 0);
        }
        const uint32_t vis4 = *(const uint32_t*)(m_lds + kt * 16 + lg * 4);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int key = key0 + kt * 16 + lg * 4 + rr;
          const bool vis = ((vis4 >> (8 * rr)) & 0xffu) != 0 && key <= qrow && (key < p.prefix || key >= qlo);
          const float pr = vis ? __builtin_amdgcn_exp2f(as[rr] * p.scale_log2e - lse_q) : 0.f;
          e[half * 4 + rr] = pr * (ap[rr] - dsum);
        }
      }
      const bf16x8_t dsf = pack8(e);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(k_lds, 32 * s2, dt, l15, lg), dsf, acc[dt], 0, 0, 0);
    }
  }
  if (qrow < p.S) {
    uint16_t* op = p.dq + (long)b * p.q_bs + (long)h * p.q_hs + (long)qrow * p.q_rs;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      u32x2_t w;
      w[0] = pack2bf(acc[dt][0] * p.scale, acc[dt][1] * p.scale);
      w[1] = pack2bf(acc[dt][2] * p.scale, acc[dt][3] * p.scale);
      *(u32x2_t*)(op + dt * 16 + lg * 4) = w;
    }
  }
#endif
}

// dk / dv: a workgroup owns 128 key rows (one 16-row tile per wave), Q and dO stream through LDS. A prefix key tile walks the
// prefix queries from its own row on and then EVERY branch's queries, in row order: that is where the branches' contributions
// to the prefix rows of dk / dv are summed. A branch key tile walks the rows of its own branch(es) only.
__global__ __launch_bounds__(512) void tree_bwd_dkv_kernel(TreeArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* q_lds = smem;
  char* g_lds = smem + KC * ROWB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  const uint8_t* mrow = p.mask ? p.mask + (long)b * p.mask_bs : nullptr;
  const uint16_t* qbase = p.q + (long)b * p.q_bs + (long)h * p.q_hs;
  const uint16_t* gbase = p.dout + (long)b * p.o_bs + (long)h * p.o_hs;
  const float* lse = p.lse + ((long)b * p.H + h) * p.stat_rs;
  const float* delta = p.delta + ((long)b * p.H + h) * p.stat_rs;

  const int k0 = (blockIdx.y * 8 + wave) * 16, key = k0 + l15;
  const bool key_ok = key < p.S && (mrow == nullptr || mrow[min(key, p.S - 1)] != 0);
  const int khi = branch_hi(min(key, p.S - 1), p.prefix, p.branch, p.S);            // this lane's key is seen by queries [key, khi)
  const int wave_hi = k0 < p.prefix ? p.S : branch_hi(min(k0 + 15, p.S - 1), p.prefix, p.branch, p.S);
  const int blk_k0 = (int)blockIdx.y * 128;
  const int blk_hi = blk_k0 < p.prefix ? p.S : branch_hi(min(blk_k0 + 127, p.S - 1), p.prefix, p.branch, p.S);
  bf16x8_t kf[KS], vf[KS];
  {
    const uint16_t* kp = p.k + (long)b * p.k_bs + (long)h * p.k_hs + (long)key * p.k_rs;
    const uint16_t* vp = p.v + (long)b * p.v_bs + (long)h * p.v_hs + (long)key * p.v_rs;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int ch = lg + 4 * ks;
      u32x4_t t = {0u, 0u, 0u, 0u}, u = {0u, 0u, 0u, 0u};
      if (key < p.S) {
        t = *(const u32x4_t*)(kp + ch * 8);
        u = *(const u32x4_t*)(vp + ch * 8);
      }
      kf[ks] = __builtin_bit_cast(bf16x8_t, t);
      vf[ks] = __builtin_bit_cast(bf16x8_t, u);
    }
  }
  f32x4_t dk[DT], dv[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) dk[i] = dv[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // first 32-row query step this wave / this workgroup needs (rows below the key tile see nothing of it)
  int s2_wave = k0 >> 5;
  const int s2_block = blk_k0 >> 5;
  if (k0 >= p.S) s2_wave = (p.S + 31) >> 5;                          // tile past the end: no steps
  for (int qc0 = (s2_block * 32) / KC * KC; qc0 < blk_hi; qc0 += KC) {
    __syncthreads();
    stage_two(q_lds, g_lds, qbase + (long)qc0 * p.q_rs, p.q_rs, gbase + (long)qc0 * p.o_rs, p.o_rs, KC, min(KC, p.S - qc0), tid);
    __syncthreads();
#pragma unroll 1
    for (int s2 = max(s2_wave, qc0 >> 5); s2 * 32 < min(wave_hi, qc0 + KC); ++s2) {
      float pe[8], de[8];
      const int lrow = s2 * 32 - qc0;                                // row of this step inside the staged chunk
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int qt = 2 * s2 + half;
        const f32x4_t l4 = *(const f32x4_t*)(lse + qt * 16 + lg * 4);     // stat rows are padded to 32
        const f32x4_t d4 = *(const f32x4_t*)(delta + qt * 16 + lg * 4);
        f32x4_t as = {0.f, 0.f, 0.f, 0.f}, ap = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          as = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(q_lds, lrow + half * 16 + l15, lg + 4 * ks), kf[ks], as, 0, 0, 0);
          ap = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(g_lds, lrow + half * 16 + l15, lg + 4 * ks), vf[ks], ap, 0, 0, 0);
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int q = qt * 16 + lg * 4 + rr;
          const bool vis = key_ok && key <= q && q < khi;
          const float pr = vis ? __builtin_amdgcn_exp2f(as[rr] * p.scale_log2e - l4[rr]) : 0.f;
          pe[half * 4 + rr] = pr;
          de[half * 4 + rr] = vis ? pr * (ap[rr] - d4[rr]) : 0.f;
        }
      }
      const bf16x8_t pf = pack8(pe), dsf = pack8(de);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(g_lds, lrow, dt, l15, lg), pf, dv[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(q_lds, lrow, dt, l15, lg), dsf, dk[dt], 0, 0, 0);
      }
    }
  }
  if (key < p.S) {
    uint16_t* kp = p.dk + (long)b * p.k_bs + (long)h * p.k_hs + (long)key * p.k_rs;
    uint16_t* vp = p.dv + (long)b * p.v_bs + (long)h * p.v_hs + (long)key * p.v_rs;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int d = dt * 16 + lg * 4;
      u32x2_t w;
      w[0] = pack2bf(dk[dt][0] * p.scale, dk[dt][1] * p.scale);
      w[1] = pack2bf(dk[dt][2] * p.scale, dk[dt][3] * p.scale);
      *(u32x2_t*)(kp + d) = w;
      w[0] = pack2bf(dv[dt][0], dv[dt][1]);
      w[1] = pack2bf(dv[dt][2], dv[dt][3]);
      *(u32x2_t*)(vp + d) = w;
    }
  }
#endif
}

// the argument checks both entry points share; fills everything but the backward's pointers
int fill_tree(const bl_attn_desc* d, int32_t prefix, int32_t branch, TreeArgs& a) {
  if (!d || !d->q || !d->k || !d->v || !d->o) return BL_E_ARG;
  if (prefix < 1 || branch < 1) return BL_E_ARG;
  if (d->B <= 0 || d->H <= 0 || d->Sq <= 0 || d->Skv != d->Sq || !d->causal || d->head_dim != HD) return BL_E_SHAPE;
  if (prefix > d->Sq || (d->Sq - prefix) % branch != 0) return BL_E_SHAPE;
  if ((long)d->B * d->H > 0x7fffffffL || d->B > 65535 || d->H > 65535 || (d->Sq + 63) / 64 > 65535) return BL_E_SHAPE;
  const int64_t st[] = {d->q_bs, d->q_hs, d->q_rs, d->k_bs, d->k_hs, d->k_rs, d->v_bs, d->v_hs, d->v_rs, d->o_bs, d->o_hs, d->o_rs};
  for (int64_t s : st) if (s % 8) return BL_E_SHAPE;
  if (!bl_aligned16(d->q) || !bl_aligned16(d->k) || !bl_aligned16(d->v) || !bl_aligned16(d->o)) return BL_E_ALIGN;
  a = TreeArgs{};
  a.q = d->q; a.k = d->k; a.v = d->v; a.o = d->o; a.out = d->o; a.mask = d->key_mask;
  a.q_bs = d->q_bs; a.q_hs = d->q_hs; a.q_rs = d->q_rs; a.k_bs = d->k_bs; a.k_hs = d->k_hs; a.k_rs = d->k_rs;
  a.v_bs = d->v_bs; a.v_hs = d->v_hs; a.v_rs = d->v_rs; a.o_bs = d->o_bs; a.o_hs = d->o_hs; a.o_rs = d->o_rs;
  a.mask_bs = d->mask_bs;
  a.B = d->B; a.H = d->H; a.S = d->Sq; a.prefix = prefix; a.branch = branch; a.stat_rs = (d->Sq + 31) / 32 * 32;
  a.scale = d->scale; a.scale_log2e = d->scale * 1.44269504088896340736f;
  return BL_OK;
}

// ---- rotary embedding at per-row positions ---------------------------------------------------------------------------------
// rope_kvcache_kernel (glue.hip) without a cache / rope_bwd_kernel (train.hip), with pos[row] in place of pos0 + row % S: the
// same expressions, so the same bits. One thread per (row, head, 8 rotation pairs) [forward] / per (row, head, pairs, q | k).
__device__ __forceinline__ void unpack8(const u32x4_t q, float* v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = bflo(q[i]); v[2 * i + 1] = bfhi(q[i]); }
}
__device__ __forceinline__ u32x4_t pack8u(const float* v) {
  u32x4_t q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = pack2bf(v[2 * i], v[2 * i + 1]);
  return q;
}

__global__ void rope_pos_kernel(uint16_t* qkv, long ld, long rows, int H, int hd, const uint16_t* cos_tab, const uint16_t* sin_tab,
                                const int32_t* pos_tab) {
  const int half = hd >> 1, cpr = half >> 3;
  const long total = rows * H * cpr;
  const long D = (long)H * hd;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cpr);
    const int h = (int)((i / cpr) % H);
    const long tok = i / ((long)cpr * H);
    const int pos = max(pos_tab[tok], 0);
    const u32x4_t cq = *(const u32x4_t*)(cos_tab + (long)pos * half + ch * 8);
    const u32x4_t sq = *(const u32x4_t*)(sin_tab + (long)pos * half + ch * 8);
    uint16_t* row = qkv + tok * ld;
#pragma unroll
    for (int part = 0; part < 2; ++part) {             // 0 = q, 1 = k, both in place
      uint16_t* src = row + part * D + (long)h * hd;
      const u32x4_t x1 = *(const u32x4_t*)(src + ch * 8);
      const u32x4_t x2 = *(const u32x4_t*)(src + half + ch * 8);
      u32x4_t o1, o2;
      rope_pair(x1, x2, cq, sq, o1, o2);
      *(u32x4_t*)(src + ch * 8) = o1;
      *(u32x4_t*)(src + half + ch * 8) = o2;
    }
  }
}

__global__ void rope_pos_bwd_kernel(uint16_t* dqkv, long ld, long rows, int H, int hd, const uint16_t* cos_tab,
                                    const uint16_t* sin_tab, const int32_t* pos_tab) {
  const int half = hd >> 1, cpr = half >> 3;
  const long total = rows * H * cpr * 2;
  const long D = (long)H * hd;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int part = (int)(i & 1);
    const long ii = i >> 1;
    const int ch = (int)(ii % cpr), h = (int)((ii / cpr) % H);
    const long tok = ii / ((long)cpr * H);
    const int pos = max(pos_tab[tok], 0);
    float c[8], s[8], d1[8], d2[8], o1[8], o2[8];
    unpack8(*(const u32x4_t*)(cos_tab + (long)pos * half + ch * 8), c);
    unpack8(*(const u32x4_t*)(sin_tab + (long)pos * half + ch * 8), s);
    uint16_t* p = dqkv + tok * ld + part * D + (long)h * hd + ch * 8;
    unpack8(*(const u32x4_t*)p, d1);
    unpack8(*(const u32x4_t*)(p + half), d2);
#pragma unroll
    for (int e = 0; e < 8; ++e) { o1[e] = d1[e] * c[e] + d2[e] * s[e]; o2[e] = d2[e] * c[e] - d1[e] * s[e]; }
    *(u32x4_t*)p = pack8u(o1);
    *(u32x4_t*)(p + half) = pack8u(o2);
  }
}

static inline int grid_for(long total, int block) { return (int)std::min<long>((total + block - 1) / block, 65535L * 16); }

}  // namespace bl_attention_tree_impl
using namespace bl_attention_tree_impl;

extern "C" int bl_attention_tree_lse_bf16(const bl_attn_desc* d, int32_t prefix, int32_t branch, float* lse, void* stream) {
  if (!lse) return BL_E_ARG;
  TreeArgs a;
  const int rc = fill_tree(d, prefix, branch, a);
  if (rc != BL_OK) return rc;
  if (((uintptr_t)lse) & 15) return BL_E_ALIGN;
  a.lse = lse;
  hipLaunchKernelGGL(tree_fwd_kernel, dim3((a.S + 63) / 64, a.H, a.B), dim3(256), 0, (hipStream_t)stream, a);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_attention_tree_backward_bf16(const bl_attn_desc* d, int32_t prefix, int32_t branch, const bl_bf16* dout,
                                               const float* lse, float* delta, bl_bf16* dq, bl_bf16* dk, bl_bf16* dv, void* stream) {
  if (!dout || !lse || !delta || !dq || !dk || !dv) return BL_E_ARG;
  TreeArgs a;
  const int rc = fill_tree(d, prefix, branch, a);
  if (rc != BL_OK) return rc;
  if ((a.S + 127) / 128 > 65535) return BL_E_SHAPE;
  const void* ptrs[] = {dout, dq, dk, dv, lse, delta};
  for (const void* x : ptrs) if (!bl_aligned16(x)) return BL_E_ALIGN;
  a.dout = dout; a.dq = dq; a.dk = dk; a.dv = dv; a.lse = const_cast<float*>(lse); a.delta = delta;
  constexpr int LDS = 2 * KC * ROWB + KC;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&tree_bwd_dq_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&tree_bwd_dkv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess)
      return BL_E_LAUNCH;
    attr_set = true;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.B * a.H, (a.S + 127) / 128);
  hipLaunchKernelGGL(tree_bwd_dq_kernel, grid, dim3(512), LDS, s, a);
  hipLaunchKernelGGL(tree_bwd_dkv_kernel, grid, dim3(512), LDS, s, a);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

static int rope_pos_check(const void* qkv, int64_t ld, int64_t rows, int32_t H, int32_t hd, const void* cos_tab, const void* sin_tab,
                          const int32_t* pos) {
  if (!qkv || !cos_tab || !sin_tab || !pos) return BL_E_ARG;
  if (rows <= 0 || H <= 0 || hd <= 0 || (hd % 16) || ld < 3L * H * hd || (ld % 8)) return BL_E_SHAPE;
  if (!bl_aligned16(qkv) || !bl_aligned16(cos_tab) || !bl_aligned16(sin_tab) || (((uintptr_t)pos) & 3)) return BL_E_ALIGN;
  return BL_OK;
}

extern "C" int bl_rope_pos_bf16(bl_bf16* qkv, int64_t ld, int64_t rows, int32_t H, int32_t head_dim, const bl_bf16* cos_tab,
                                const bl_bf16* sin_tab, const int32_t* pos, void* stream) {
  const int rc = rope_pos_check(qkv, ld, rows, H, head_dim, cos_tab, sin_tab, pos);
  if (rc != BL_OK) return rc;
  const long total = (long)rows * H * (head_dim / 16);
  hipLaunchKernelGGL(rope_pos_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, qkv, (long)ld, (long)rows, H,
                     head_dim, cos_tab, sin_tab, pos);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

extern "C" int bl_rope_pos_backward_bf16(bl_bf16* dqkv, int64_t ld, int64_t rows, int32_t H, int32_t head_dim, const bl_bf16* cos_tab,
                                         const bl_bf16* sin_tab, const int32_t* pos, void* stream) {
  const int rc = rope_pos_check(dqkv, ld, rows, H, head_dim, cos_tab, sin_tab, pos);
  if (rc != BL_OK) return rc;
  const long total = (long)rows * H * (head_dim / 16) * 2;
  hipLaunchKernelGGL(rope_pos_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, dqkv, (long)ld, (long)rows,
                     H, head_dim, cos_tab, sin_tab, pos);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
