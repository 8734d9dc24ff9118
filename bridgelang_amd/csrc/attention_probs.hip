// attention_probs.hip — the attention probabilities themselves: P = softmax(q k^T * scale [+ causal] [+ key mask]) in fp32,
// and their sums over up to 8 key segments, for head_dim 128 over a rotated-K cache view (bl_attention_probs_f32).
//
// The fused kernels of attention.hip never materialise P and rotate q in registers; this is the read-only "tap" that
// follows them in a plan. It reads q (rotated in memory, or un-rotated and rotated on load with rope_pair, the arithmetic
// of the fused attention kernels, bit for bit) and the rotated K rows of the cache, and writes fp32 P and / or the segment sums.
//
//   * one workgroup = 4 waves = 16 query rows of one (batch, head). The scores of the 16 rows against all ceil16(Skv) keys
//     sit in dynamic LDS as fp32 (row stride s_pad + 4 floats: at most 16 x 2052 x 4 B = 128.25 KiB of the 160 KiB).
//   * QK^T: v_mfma_f32_16x16x32_bf16, computed swapped as in attention.hip (K rows are the "A" operand, q the "B" operand),
//     so a lane owns one query column and 4 consecutive keys of a 16-key tile: one 16-byte LDS write per tile. The waves
//     stride over the key tiles; K fragments come straight from global memory (every K byte is used once per workgroup).
//   * softmax: ONE wave per query row. Lane t owns the 4-key units t, t + 64, ... of the row; per-lane sequential max / sum
//     in increasing key order, then the xor butterfly. This order depends on nothing but the key index, and an invisible
//     key adds an exact 0, so a row's results are the same bits whatever Sq, Skv (beyond its own visible keys) or tile
//     position it is launched with: a Sq = S launch and S launches of Sq = 1 agree bit for bit.
//   * numerics: s' = fp32 MFMA accumulation of the 128 exact bf16 products, times fp32(scale * log2e); e = exp2(s' - m);
//     P = e * (1 / sum e) in fp32. No rounding of P to bf16.
//   * safety: K rows at or beyond Skv are never read; rows of masked keys are read but their scores are SELECTED out
//     (never multiplied by 0), so NaN there reaches no output. Nothing outside probs[.., 0 .. p_cols) and seg is written.
#include "bl_common.h"
#include <math.h>

namespace bl_attention_probs_impl {

struct ProbsArgs {
  const uint16_t* q; const uint16_t* k; const uint8_t* mask;
  long q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, mask_bs;
  int B, H, Sq, Skv, causal;
  float scale_log2e;
  const uint16_t* cos_tab; const uint16_t* sin_tab; const int* rope_pos; int rope_rows, pos0;   // cos_tab == nullptr: q is rotated
  float* probs; long p_bs, p_hs, p_rs; int p_cols, p_vec;                                       // p_vec: 16-byte stores allowed
  float* seg; const int* seg_bounds; int n_seg;
  int s_pad, row_f;                                                                              // ceil16(Skv), LDS row stride (floats)
};

constexpr int NWAVES = 4;

__global__ __launch_bounds__(NWAVES * 64) void attn_probs_kernel(ProbsArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sc[];   // [16][row_f]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 16;
  const int nrows = min(16, p.Sq - q0);
  const int qrow = q0 + l15;
  const int off = p.Skv - p.Sq;                 // causal: key j visible to query i iff j <= i + off
  const uint8_t* mrow = p.mask ? p.mask + (long)b * p.mask_bs : nullptr;

  // ---- q fragments ("B" operand): lane holds q[qrow][8*(lg + 4*ks) .. +7], rotated ----
  bf16x8_t qf[4];
  {
    u32x4_t c[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) c[ks] = (u32x4_t){0u, 0u, 0u, 0u};
    if (l15 < nrows) {
      const uint16_t* qp = p.q + (long)b * p.q_bs + (long)h * p.q_hs + (long)qrow * p.q_rs;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) c[ks] = *(const u32x4_t*)(qp + (lg + 4 * ks) * 8);
      if (p.cos_tab) {
        // chunks lg and lg + 4 pair with lg + 8 and lg + 12: exactly the four chunks this lane holds
        int pos = (p.rope_pos ? p.rope_pos[b] : p.pos0) + qrow;
        pos = min(max(pos, 0), p.rope_rows - 1);          // a position read from the device cannot be checked by the host
        const uint16_t* ct = p.cos_tab + (long)pos * 64;
        const uint16_t* st = p.sin_tab + (long)pos * 64;
        u32x4_t o1, o2;
        rope_pair(c[0], c[2], *(const u32x4_t*)(ct + lg * 8), *(const u32x4_t*)(st + lg * 8), o1, o2);
        c[0] = o1; c[2] = o2;
        rope_pair(c[1], c[3], *(const u32x4_t*)(ct + (lg + 4) * 8), *(const u32x4_t*)(st + (lg + 4) * 8), o1, o2);
        c[1] = o1; c[3] = o2;
      }
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = __builtin_bit_cast(bf16x8_t, c[ks]);
  }

  // ---- scores: S^T = K · q^T per 16-key tile; lane owns query column l15 and keys key0 + 4*lg + {0..3} ----
  const uint16_t* kbase = p.k + (long)b * p.k_bs + (long)h * p.k_hs;
  const int ntiles = p.s_pad >> 4;
  const int last_key = p.causal ? min(p.Skv - 1, q0 + 15 + off) : p.Skv - 1;   // no key beyond it is visible to this tile
  for (int kt = wave; kt < ntiles; kt += NWAVES) {
    const int key0 = kt * 16;
    f32x4_t s = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (key0 <= last_key) {                     // wave-uniform
      u32x4_t kf[4];                            // "A" operand: lane holds K[key0 + l15][8*(lg + 4*ks) .. +7], zeros past Skv
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kf[ks] = (u32x4_t){0u, 0u, 0u, 0u};
      if (key0 + l15 < p.Skv) {
        const uint16_t* kp = kbase + (long)(key0 + l15) * p.k_rs;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const u32x4_t*)(kp + (lg + 4 * ks) * 8);
      }
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[ks]), qf[ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + lg * 4 + r;
        bool vis = key < p.Skv;
        if (p.causal) vis = vis && (key <= qrow + off);
        if (mrow) vis = vis && (key < p.Skv ? mrow[key] != 0 : false);
        s[r] = vis ? acc[r] * p.scale_log2e : -INFINITY;    // select: a NaN score of a hidden key stops here
      }
    }
    if (l15 < nrows) *(f32x4_t*)(sc + l15 * p.row_f + key0 + lg * 4) = s;
  }
  __syncthreads();

  // ---- softmax, stores and segment sums: one wave per row; a lane only ever touches its own 4-key units of the row ----
  const int nunits = p.s_pad >> 2;
  for (int r = wave; r < nrows; r += NWAVES) {
    float* srow = sc + r * p.row_f;
    float mx = -INFINITY;
    for (int u = lane; u < nunits; u += 64) {
      const f32x4_t v = *(const f32x4_t*)(srow + u * 4);
      mx = fmaxf(mx, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    }
    mx = wave_max(mx);
    const float m_use = (mx == -INFINITY) ? 0.f : mx;
    float l = 0.f;
    for (int u = lane; u < nunits; u += 64) {
      f32x4_t v = *(const f32x4_t*)(srow + u * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = __builtin_amdgcn_exp2f(v[j] - m_use); l += v[j]; }
      *(f32x4_t*)(srow + u * 4) = v;
    }
    l = wave_sum(l);
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    const long row_id = q0 + r;

    if (p.probs) {
      float* prow = p.probs + (long)b * p.p_bs + (long)h * p.p_hs + row_id * p.p_rs;
      const int ounits = (p.p_cols + 3) >> 2;
      for (int u = lane; u < ounits; u += 64) {
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (u < nunits) {
          v = *(const f32x4_t*)(srow + u * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= inv;
        }
        const int c0 = u * 4;
        if (p.p_vec && c0 + 3 < p.p_cols) {
          *(f32x4_t*)(prow + c0) = v;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < p.p_cols) prow[c0 + j] = v[j];
        }
      }
    }
    if (p.seg) {
      const int* bd = p.seg_bounds + (long)b * (p.n_seg + 1);
      float* sg = p.seg + (((long)b * p.H + h) * p.Sq + row_id) * p.n_seg;
      int lo = min(max(bd[0], 0), p.Skv);
      for (int s = 0; s < p.n_seg; ++s) {
        const int hi = min(max(bd[s + 1], lo), p.Skv);
        float t = 0.f;
        // the lane's units that overlap [lo, hi), in increasing key order
        const int u_lo = lo >> 2, u_hi = (hi + 3) >> 2;
        int u = u_lo + ((lane - u_lo) & 63);
        for (; u < u_hi; u += 64) {
          const f32x4_t v = *(const f32x4_t*)(srow + u * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = u * 4 + j;
            if (key >= lo && key < hi) t += v[j] * inv;
          }
        }
        t = wave_sum(t);
        if (lane == 0) sg[s] = t;
        lo = hi;
      }
    }
  }
}

}  // namespace bl_attention_probs_impl
using namespace bl_attention_probs_impl;

extern "C" int bl_attention_probs_f32(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t rope_rows,
                                      int32_t pos0, const int32_t* rope_pos, float* probs, int64_t p_bs, int64_t p_hs,
                                      int64_t p_rs, int32_t p_cols, float* seg, const int32_t* seg_bounds, int32_t n_seg,
                                      void* stream) {
  if (!d || !d->q || !d->k) return BL_E_ARG;
  if (!probs && !seg) return BL_E_ARG;
  if ((cos_tab == nullptr) != (sin_tab == nullptr)) return BL_E_ARG;
  if (rope_pos && !cos_tab) return BL_E_ARG;
  if (seg && !seg_bounds) return BL_E_ARG;
  if (d->B <= 0 || d->H <= 0 || d->Sq <= 0 || d->Skv <= 0) return BL_E_SHAPE;
  if (d->head_dim != 128 || d->Skv > 2048 || d->B > 65535 || d->H > 65535) return BL_E_SHAPE;
  if (d->causal && d->Skv < d->Sq) return BL_E_SHAPE;
  if (probs && (p_cols < d->Skv || (d->Sq > 1 && p_rs < p_cols))) return BL_E_SHAPE;
  if (seg && (n_seg < 1 || n_seg > 8)) return BL_E_SHAPE;
  if (cos_tab && (rope_rows < 1 || pos0 < 0 || (!rope_pos && (int64_t)pos0 + d->Sq > rope_rows))) return BL_E_SHAPE;
  const int64_t st[] = {d->q_bs, d->q_hs, d->q_rs, d->k_bs, d->k_hs, d->k_rs};
  for (int64_t s : st) if (s % 8) return BL_E_ALIGN;
  if (!bl_aligned16(d->q) || !bl_aligned16(d->k)) return BL_E_ALIGN;
  if (cos_tab && (!bl_aligned16(cos_tab) || !bl_aligned16(sin_tab))) return BL_E_ALIGN;
  if ((((uintptr_t)probs) & 3) || (((uintptr_t)seg) & 3) || (((uintptr_t)seg_bounds) & 3) || (((uintptr_t)rope_pos) & 3))
    return BL_E_ALIGN;

  ProbsArgs a;
  a.q = d->q; a.k = d->k; a.mask = d->key_mask;
  a.q_bs = d->q_bs; a.q_hs = d->q_hs; a.q_rs = d->q_rs; a.k_bs = d->k_bs; a.k_hs = d->k_hs; a.k_rs = d->k_rs;
  a.mask_bs = d->mask_bs;
  a.B = d->B; a.H = d->H; a.Sq = d->Sq; a.Skv = d->Skv; a.causal = d->causal ? 1 : 0;
  a.scale_log2e = d->scale * 1.44269504088896340736f;
  a.cos_tab = cos_tab; a.sin_tab = sin_tab; a.rope_pos = rope_pos; a.rope_rows = rope_rows; a.pos0 = pos0;
  a.probs = probs; a.p_bs = p_bs; a.p_hs = p_hs; a.p_rs = p_rs; a.p_cols = probs ? p_cols : 0;
  a.p_vec = probs && bl_aligned16(probs) && p_bs % 4 == 0 && p_hs % 4 == 0 && p_rs % 4 == 0;
  a.seg = seg; a.seg_bounds = seg_bounds; a.n_seg = seg ? n_seg : 0;
  a.s_pad = (d->Skv + 15) / 16 * 16;
  a.row_f = a.s_pad + 4;
  const int lds = 16 * a.row_f * (int)sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_probs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess)
      return BL_E_LAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(attn_probs_kernel, dim3((d->Sq + 15) / 16, d->H, d->B), dim3(NWAVES * 64), lds, (hipStream_t)stream, a);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
