// attention_decode_shared.hip — single-query decode attention for rows that share a prompt (head_dim 128).
//
// `group` consecutive rows of the step's fused qkv belong to ONE prompt: samples of a GRPO group, candidates of a reranker,
// beams. Their keys 0 … prefix_len-1 are that prompt's cache rows, stored once ([P, H, cache_len, 128]); the keys after
// them are the row's own generated tokens, kept in a small cache of their own ([P·group, H, gen_len, 128]). Nothing is
// copied: the kernel reads the prompt rows in place.
//
// One workgroup (4 waves) serves GQ consecutive rows of one (prompt, head). It loads every prefix K row — and later V row —
// ONCE into registers and uses it for all its queries; the generated rows and the step's new token are per row.
//
// Per query the arithmetic is attn_decode_kernel<ROPE = true>'s (attention.hip), in its order, so the output equals that
// kernel's on replicated caches bit for bit:
//   * key → (wave, j, ks) by key index: key = g·64 + wave·16 + j·4 + ks, whichever cache the key's row comes from;
//   * a score = 8 in-lane products summed in index order, then the 16-lane xor butterfly (1, 2, 4, 8); sc[key] in LDS;
//   * every wave recomputes max and sum over sc[0 … pos] with the same strided loop and butterfly;
//   * P = bf16(exp2(sc - max)); a lane accumulates its keys in ascending key order (prefix keys, then generated keys: all
//     generated keys come after all prefix keys, so the two passes keep the order); a key outside a pass contributes
//     0 · 0 to an accumulator that is never -0, which leaves it as it is, like the reference's keys past the cache;
//   * the new key is added last, by wave 0's key slot 0; the ks partials fold by xor 16, 32; the four waves sum through
//     LDS in wave order.
// Both forms of that kernel are kept: up to 320 cached keys all prefix rows are requested before anything is computed;
// beyond, 64-key groups stream. Same arithmetic in both.
#include "bl_common.h"
#include <math.h>

namespace bl_attention_shared_impl {

struct SharedArgs {
  const uint16_t* qkv;                 // [R, 3·H·128]: q | k_new | v_new
  const uint16_t* k; const uint16_t* v;   // prompt caches
  uint16_t* kg; uint16_t* vg;          // generated-token caches [R, H, gen_len, 128]
  uint16_t* o;
  const uint16_t* cos_tab; const uint16_t* sin_tab;
  long q_bs, q_hs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs, o_bs, o_hs, g_bs, g_hs;
  int H, group, prefix_len, pos;
  float scale_log2e;
};

template <int GQ>
__global__ __launch_bounds__(256) void attn_decode_shared_kernel(SharedArgs p) {
  extern __shared__ float smem[];      // sc[GQ][n_pad] | part[GQ][4][128]
  const int pos = p.pos, n = pos + 1, n_cache = pos, n_pre = p.prefix_len;
  const int n_pad = (n + 63) & ~63;
  float* sc = smem;
  float* part = smem + GQ * n_pad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ks = lane >> 4, dc = lane & 15;
  // workgroups of one (prompt, head) are neighbours: they read the same prefix rows
  const int chunks = (p.group + GQ - 1) / GQ;
  int bid = blockIdx.x;
  const int chunk = bid % chunks;
  bid /= chunks;
  const int pr = bid / p.H, h = bid - pr * p.H;
  const long D = (long)p.H * 128;
  const uint16_t* kc = p.k + (long)pr * p.k_bs + (long)h * p.k_hs + dc * 8;
  const uint16_t* vc = p.v + (long)pr * p.v_bs + (long)h * p.v_hs + dc * 8;
  // query qi of this workgroup: row pr·group + chunk·GQ + qi. A query past the group (masked tail) recomputes the group's
  // last row and stores nothing.
  long qoff[GQ], goff[GQ];
  bool valid[GQ];
#pragma unroll
  for (int qi = 0; qi < GQ; ++qi) {
    const int jq = chunk * GQ + qi;
    valid[qi] = jq < p.group;
    const long r = (long)pr * p.group + (valid[qi] ? jq : p.group - 1);
    qoff[qi] = r * p.q_bs + (long)h * p.q_hs;
    goff[qi] = r * p.g_bs + (long)h * p.g_hs + dc * 8;
  }

#define BL_LOAD_ROWS(DST, BASE, RS, G0)                                                            \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                   \
    const int key = (G0) + wave * 16 + j * 4 + ks;                                                  \
    DST[j] = (u32x4_t){0u, 0u, 0u, 0u};                                                             \
    if (key < n_pre) DST[j] = *(const u32x4_t*)(BASE + (long)key * (RS));                           \
  }
  // generated keys of query QI in the 64-key group G0: cache row key - prefix_len of the row's own cache
#define BL_LOAD_GEN(DST, BASE, QI, G0)                                                              \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                   \
    const int key = (G0) + wave * 16 + j * 4 + ks;                                                  \
    DST[j] = (u32x4_t){0u, 0u, 0u, 0u};                                                             \
    if (key >= n_pre && key < n_cache) DST[j] = *(const u32x4_t*)(BASE + goff[QI] + (long)(key - n_pre) * 128); \
  }
#define BL_SCORES(KQ, QI, G0, LO, HI)                                                               \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                   \
    const int key = (G0) + wave * 16 + j * 4 + ks;                                                  \
    float d = 0.f;                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) d += qv[QI][2 * i] * bflo(KQ[j][i]) + qv[QI][2 * i + 1] * bfhi(KQ[j][i]); \
    d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 8, 64); \
    if (dc == 0 && key >= (LO) && key < (HI)) sc[(QI) * n_pad + key] = d * p.scale_log2e;           \
  }
#define BL_PV(VQ, QI, G0, LO, HI)                                                                   \
  do {                                                                                              \
    float pk[4];                                                                                    \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                 \
      const int key = (G0) + wave * 16 + j * 4 + ks;                                                \
      pk[j] = (key >= (LO) && key < (HI)) ? rbf(__builtin_amdgcn_exp2f(sc[(QI) * n_pad + key] - m_use[QI])) : 0.f; \
    }                                                                                               \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                   \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
        acc[QI][2 * i] += pk[j] * bflo(VQ[j][i]); acc[QI][2 * i + 1] += pk[j] * bfhi(VQ[j][i]);     \
      }                                                                                             \
  } while (0)

  constexpr int NG = 5;
  const bool resident = n_cache <= NG * 64;
  u32x4_t kr[NG][4], vr[NG][4];
  if (resident) {        // requested first: the q / new-token loads and the rotations below run under their latency
#pragma unroll
    for (int g = 0; g < NG; ++g) BL_LOAD_ROWS(kr[g], kc, p.k_rs, g * 64);
  }

  // ---- every query's rotated q, its new token's score and the append to its own cache ----
  float qv[GQ][8];
  u32x4_t v_new[GQ];
  {
    // half-split rotation: chunk dc pairs with chunk dc ^ 8; out = bf16(bf16(own*cos) + bf16(±partner*sin))
    const u32x4_t cq = *(const u32x4_t*)(p.cos_tab + (long)pos * 64 + (dc & 7) * 8);
    const u32x4_t sq = *(const u32x4_t*)(p.sin_tab + (long)pos * 64 + (dc & 7) * 8);
    const float sgn = dc < 8 ? -1.f : 1.f;
#pragma unroll
    for (int qi = 0; qi < GQ; ++qi) {
      const uint16_t* qp = p.qkv + qoff[qi];
      const uint16_t* kn = qp + D;
      const uint16_t* vn = qp + 2 * D;
      const u32x4_t q_own = *(const u32x4_t*)(qp + dc * 8), q_par = *(const u32x4_t*)(qp + (dc ^ 8) * 8);
      const u32x4_t k_own = *(const u32x4_t*)(kn + dc * 8), k_par = *(const u32x4_t*)(kn + (dc ^ 8) * 8);
      const u32x4_t v_own = *(const u32x4_t*)(vn + dc * 8);
      float knv[8];
      u32x4_t kw;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float c0 = bflo(cq[i]), c1 = bfhi(cq[i]), s0 = bflo(sq[i]) * sgn, s1 = bfhi(sq[i]) * sgn;
        qv[qi][2 * i] = rbf(rbf(bflo(q_own[i]) * c0) + rbf(bflo(q_par[i]) * s0));
        qv[qi][2 * i + 1] = rbf(rbf(bfhi(q_own[i]) * c1) + rbf(bfhi(q_par[i]) * s1));
        knv[2 * i] = rbf(rbf(bflo(k_own[i]) * c0) + rbf(bflo(k_par[i]) * s0));
        knv[2 * i + 1] = rbf(rbf(bfhi(k_own[i]) * c1) + rbf(bfhi(k_par[i]) * s1));
        kw[i] = pack2bf(knv[2 * i], knv[2 * i + 1]);
      }
      v_new[qi] = v_own;
      if (valid[qi] && wave == 0 && ks == 0) {   // append the new token to the row's own cache
        *(u32x4_t*)(p.kg + goff[qi] + (long)(pos - n_pre) * 128) = kw;
        *(u32x4_t*)(p.vg + goff[qi] + (long)(pos - n_pre) * 128) = v_own;
      }
      float d = 0.f;     // score of the new key, from registers
#pragma unroll
      for (int i = 0; i < 8; ++i) d += qv[qi][i] * knv[i];
      d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 8, 64);
      if (wave == 0 && lane == 0) sc[qi * n_pad + pos] = d * p.scale_log2e;
    }
  }

  // ---- scores: the prefix rows once for all queries, then every query's own rows ----
  const int gen0 = n_pre & ~63;        // first 64-key group that holds a generated key
  if (resident) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int qi = 0; qi < GQ; ++qi) BL_SCORES(kr[g], qi, g * 64, 0, n_pre);
    }
    // V after the scores, as the reference kernel requests it; the generated keys' scores run under its latency
#pragma unroll
    for (int g = 0; g < NG; ++g) BL_LOAD_ROWS(vr[g], vc, p.v_rs, g * 64);
  } else {
    for (int g0 = 0; g0 < n_pre; g0 += 64) {
      u32x4_t kq[4];
      BL_LOAD_ROWS(kq, kc, p.k_rs, g0);
#pragma unroll
      for (int qi = 0; qi < GQ; ++qi) BL_SCORES(kq, qi, g0, 0, n_pre);
    }
  }
  for (int g0 = gen0; g0 < n_cache; g0 += 64) {
    u32x4_t kq[GQ][4];
#pragma unroll
    for (int qi = 0; qi < GQ; ++qi) BL_LOAD_GEN(kq[qi], p.kg, qi, g0);
#pragma unroll
    for (int qi = 0; qi < GQ; ++qi) BL_SCORES(kq[qi], qi, g0, n_pre, n_cache);
  }
  __syncthreads();

  // ---- softmax statistics (every wave, redundantly; identical results) ----
  float m_use[GQ], l[GQ];
#pragma unroll
  for (int qi = 0; qi < GQ; ++qi) {
    const float* s = sc + qi * n_pad;
    float mx = -INFINITY;
    for (int i = lane; i < n; i += 64) mx = fmaxf(mx, s[i]);
    mx = wave_max(mx);
    m_use[qi] = (mx == -INFINITY) ? 0.f : mx;
    float t = 0.f;
    for (int i = lane; i < n; i += 64) t += __builtin_amdgcn_exp2f(s[i] - m_use[qi]);
    l[qi] = wave_sum(t);
  }

  // ---- PV: same key assignment; P rounded to bf16 ----
  float acc[GQ][8];
#pragma unroll
  for (int qi = 0; qi < GQ; ++qi) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[qi][i] = 0.f;
  }
  if (resident) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int qi = 0; qi < GQ; ++qi) BL_PV(vr[g], qi, g * 64, 0, n_pre);
    }
  } else {
    for (int g0 = 0; g0 < n_pre; g0 += 64) {
      u32x4_t vq[4];
      BL_LOAD_ROWS(vq, vc, p.v_rs, g0);
#pragma unroll
      for (int qi = 0; qi < GQ; ++qi) BL_PV(vq, qi, g0, 0, n_pre);
    }
  }
  for (int g0 = gen0; g0 < n_cache; g0 += 64) {
    u32x4_t vq[GQ][4];
#pragma unroll
    for (int qi = 0; qi < GQ; ++qi) BL_LOAD_GEN(vq[qi], p.vg, qi, g0);
#pragma unroll
    for (int qi = 0; qi < GQ; ++qi) BL_PV(vq[qi], qi, g0, n_pre, n_cache);
  }
#undef BL_LOAD_ROWS
#undef BL_LOAD_GEN
#undef BL_SCORES
#undef BL_PV
#pragma unroll
  for (int qi = 0; qi < GQ; ++qi) {
    if (wave == 0 && ks == 0) {        // the new key, last
      const float pn = rbf(__builtin_amdgcn_exp2f(sc[qi * n_pad + pos] - m_use[qi]));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[qi][2 * i] += pn * bflo(v_new[qi][i]);
        acc[qi][2 * i + 1] += pn * bfhi(v_new[qi][i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) { acc[qi][i] += __shfl_xor(acc[qi][i], 16, 64); acc[qi][i] += __shfl_xor(acc[qi][i], 32, 64); }
    if (ks == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) part[(qi * 4 + wave) * 128 + dc * 8 + i] = acc[qi][i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int qi = 0; qi < GQ; ++qi) {
    if ((qi & 3) == wave && valid[qi]) {      // one wave per query: lane handles 2 output dims
      const int d0 = lane * 2;
      const float* pq = part + qi * 4 * 128;
      const float inv = l[qi] > 0.f ? 1.0f / l[qi] : 0.f;
      const float o0 = (pq[d0] + pq[128 + d0] + pq[256 + d0] + pq[384 + d0]) * inv;
      const float o1 = (pq[d0 + 1] + pq[128 + d0 + 1] + pq[256 + d0 + 1] + pq[384 + d0 + 1]) * inv;
      const long r = (long)pr * p.group + chunk * GQ + qi;
      *(uint32_t*)(p.o + r * p.o_bs + (long)h * p.o_hs + d0) = pack2bf(o0, o1);
    }
  }
}

template <int GQ>
static int launch_shared(const SharedArgs& a, int P, hipStream_t s) {
  const int n_pad = (a.pos + 1 + 63) & ~63;
  const int lds = (GQ * n_pad + GQ * 4 * 128) * (int)sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {       // GQ = 8 past 1500 keys needs more than the default 64 KiB
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_decode_shared_kernel<GQ>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
      return BL_E_LAUNCH;
    attr_set = true;
  }
  const int chunks = (a.group + GQ - 1) / GQ;
  hipLaunchKernelGGL((attn_decode_shared_kernel<GQ>), dim3(P * a.H * chunks), dim3(256), lds, s, a);
  BL_CHECK_LAUNCH();
  return BL_OK;
}

// dst[r·group + j] = src[r] for j < group: rows of `cols` bf16 (16-byte copies)
__global__ __launch_bounds__(256) void repeat_rows_kernel(const uint16_t* src, long ld_src, uint16_t* dst, long ld_dst, long rows,
                                                          int cols8, int group) {
  const long total = rows * group * cols8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / cols8;
    const int c = (int)(i - row * cols8);
    *(u32x4_t*)(dst + row * ld_dst + c * 8) = *(const u32x4_t*)(src + (row / group) * ld_src + c * 8);
  }
}

}  // namespace bl_attention_shared_impl
using namespace bl_attention_shared_impl;

// Rows per workgroup of bl_attention_decode_rope_shared_bf16, chosen by measured kernel time (16 rows of one
// prompt, 32 heads, pos = 290: 21.7 µs at 2, 34.3 at 4, 68.0 at 8 — the kernel is bound by its per-query arithmetic on one
// wave per SIMD, not by the K/V stream it shares, so fewer rows per workgroup and more workgroups win).
#define BL_SHARED_GQ 2

extern "C" int bl_attention_decode_rope_shared_gq_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab,
                                                       int32_t pos, int32_t group, int32_t prefix_len, bl_bf16* k_gen,
                                                       bl_bf16* v_gen, int32_t gen_len, int32_t gq, void* stream) {
  if (!d || !d->q || !d->k || !d->v || !d->o || !cos_tab || !sin_tab || !k_gen || !v_gen) return BL_E_ARG;
  if (d->key_mask) return BL_E_ARG;    // every row attends to all of its keys: no key mask (and no per-row positions) here
  if (gq != 2 && gq != 4 && gq != 8) return BL_E_ARG;
  if (d->head_dim != 128 || d->Sq != 1 || d->B <= 0 || d->H <= 0) return BL_E_SHAPE;
  if (group < 1 || group > 16 || d->B % group) return BL_E_SHAPE;
  if (prefix_len < 1 || pos < prefix_len || gen_len < 1 || pos - prefix_len >= gen_len || pos >= 2048) return BL_E_SHAPE;
  if (d->Skv != pos + 1) return BL_E_SHAPE;
  // the prefix rows are read in place: a head of the prompt caches must hold them
  if (d->k_rs < 128 || d->v_rs < 128 || d->k_hs < (int64_t)prefix_len * d->k_rs || d->v_hs < (int64_t)prefix_len * d->v_rs)
    return BL_E_SHAPE;
  const int64_t st[] = {d->q_bs, d->q_hs, d->k_bs, d->k_hs, d->k_rs, d->v_bs, d->v_hs, d->v_rs, d->o_bs, d->o_hs};
  for (int64_t s : st) if (s % 8) return BL_E_ALIGN;
  if (!bl_aligned16(d->q) || !bl_aligned16(d->k) || !bl_aligned16(d->v) || !bl_aligned16(d->o) || !bl_aligned16(cos_tab) ||
      !bl_aligned16(sin_tab) || !bl_aligned16(k_gen) || !bl_aligned16(v_gen))
    return BL_E_ALIGN;
  SharedArgs a;
  a.qkv = d->q; a.k = d->k; a.v = d->v; a.kg = k_gen; a.vg = v_gen; a.o = d->o; a.cos_tab = cos_tab; a.sin_tab = sin_tab;
  a.q_bs = d->q_bs; a.q_hs = d->q_hs; a.k_bs = d->k_bs; a.k_hs = d->k_hs; a.k_rs = d->k_rs;
  a.v_bs = d->v_bs; a.v_hs = d->v_hs; a.v_rs = d->v_rs; a.o_bs = d->o_bs; a.o_hs = d->o_hs;
  a.g_hs = (long)gen_len * 128; a.g_bs = (long)d->H * a.g_hs;
  a.H = d->H; a.group = group; a.prefix_len = prefix_len; a.pos = pos;
  a.scale_log2e = d->scale * 1.44269504088896340736f;
  const int P = d->B / group;
  hipStream_t s = (hipStream_t)stream;
  switch (gq) {
    case 2: return launch_shared<2>(a, P, s);
    case 4: return launch_shared<4>(a, P, s);
    default: return launch_shared<8>(a, P, s);
  }
}

extern "C" int bl_attention_decode_rope_shared_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab,
                                                    int32_t pos, int32_t group, int32_t prefix_len, bl_bf16* k_gen, bl_bf16* v_gen,
                                                    int32_t gen_len, void* stream) {
  return bl_attention_decode_rope_shared_gq_bf16(d, cos_tab, sin_tab, pos, group, prefix_len, k_gen, v_gen, gen_len, BL_SHARED_GQ,
                                                 stream);
}

extern "C" int bl_repeat_rows_bf16(const bl_bf16* src, int64_t ld_src, bl_bf16* dst, int64_t ld_dst, int64_t rows, int32_t cols,
                                   int32_t group, void* stream) {
  if (!src || !dst) return BL_E_ARG;
  if (rows <= 0 || cols <= 0 || group < 1 || cols % 8 || ld_src < cols || ld_dst < cols) return BL_E_SHAPE;
  if (ld_src % 8 || ld_dst % 8 || !bl_aligned16(src) || !bl_aligned16(dst)) return BL_E_ALIGN;
  const long total = rows * group * (cols / 8);
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(repeat_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (long)ld_src, dst, (long)ld_dst,
                     (long)rows, cols / 8, group);
  BL_CHECK_LAUNCH();
  return BL_OK;
}
