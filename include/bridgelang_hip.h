/*
 * bridgelang_hip.h — C ABI of libbridgelang_hip.so (gfx950 / MI355X).
 *
 * The reference (CliffKai/BridgeLang, a thin OpenVLA fork) has no C ABI of its own: its hot path is Python that
 * calls timm / transformers / flash-attn / torch. The drop-in seam is therefore the Python classes
 * in bridgelang_amd/extern/hf/modeling_prismatic.py; *behind* that seam every arithmetic operation goes through the
 * entry points declared here. Each entry point cites the reference call site whose arithmetic it replaces.
 *
 * Conventions
 *   - plain pointers (device memory) and integer sizes only; no torch / C++ types cross the boundary
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*) and returns immediately
 *   - no allocation, no host synchronisation, no global mutable state (thread-compatible, graph-capturable)
 *   - return value: 0 = ok, negative = error (BL_E_*); nothing is thrown across the ABI
 *   - bf16 tensors are raw uint16 bit patterns (`bl_bf16`); row-major; strides in ELEMENTS
 */
#ifndef BRIDGELANG_HIP_H
#define BRIDGELANG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t bl_bf16;

#define BL_OK 0
#define BL_E_SHAPE (-1)   /* unsupported / inconsistent shape        */
#define BL_E_ALIGN (-2)   /* pointer or stride alignment not met     */
#define BL_E_LAUNCH (-3)  /* hipLaunchKernel reported an error       */
#define BL_E_ARG (-4)     /* null pointer / bad enum                 */

/* ---- library info ------------------------------------------------------------------------------------------- */
int bl_abi_version(void);          /* bumps when a signature changes */
const char* bl_build_arch(void);   /* "gfx950" */

/* ---- deterministic synthetic tensors ------------------------------------------------------------------------ */
/* Fills dst[i] = bf16(mean + scale * irwin_hall4(seed, i)) — bit-identical to oracle/synth.py (integer hash +
 * two exactly-rounded fp32 ops). Stands in for `from_pretrained` weights (no checkpoint exists offline): the
 * reference initialises with normal(0, initializer_range), prismatic/extern/hf/modeling_prismatic.py:185-205. */
int bl_fill_synth_bf16(bl_bf16* dst, int64_t n, uint32_t seed, float mean, float scale, void* stream);
/* Same generator for a [rows, cols] logical matrix stored with leading dimension ld >= cols: element (r, c) gets the
 * value of logical index r*cols + c, so padded / interleaved device layouts hold the same numbers as the unpadded
 * tensor. Columns [cols, ld) are NOT written (allocate zeroed). */
int bl_fill_synth_bf16_2d(bl_bf16* dst, int64_t rows, int64_t cols, int64_t ld, uint32_t seed, float mean,
                          float scale, void* stream);

/* ---- weight layout ------------------------------------------------------------------------------------------------- */
/* Every GEMM weight lives in HBM in MFMA-fragment-major order: packed[nt][ks][lane][8] (nt = n/16, ks = k/32) holds
 * W[16*nt + (lane & 15)][32*ks + 8*(lane >> 4) .. +7] — the 16 bytes lane `lane` feeds v_mfma_f32_16x16x32_bf16. Each
 * (nt, ks) block is one contiguous KiB. bl_pack_weight_bf16 converts an nn.Linear-layout matrix src[n, k] (leading
 * dimension ld) once at load time; n % 16 == 0, k % 32 == 0 (pad with zeros first). */
int bl_pack_weight_bf16(const bl_bf16* src, int64_t ld, int64_t n, int64_t k, bl_bf16* dst, void* stream);

/* ---- GEMM: C[M,N] = epilogue(A[M,K] * W[N,K]^T) ------------------------------------------------------------- */
/* Replaces every nn.Linear on the path: timm Attention.qkv/proj + Mlp.fc1/fc2 (created at
 * modeling_prismatic.py:78-101), PrismaticProjector fc1/fc2/fc3 (modeling_prismatic.py:146-158), and the HF Llama
 * q/k/v/o/gate/up/down projections + lm_head (built at modeling_prismatic.py:248-250). fp32 accumulate on MFMA;
 * rounding points follow the bf16 reference (output of each Linear rounded to bf16 before the next elementwise op). */
enum bl_epilogue {
  BL_EPI_NONE = 0,        /* C = bf16(acc)                                                              */
  BL_EPI_BIAS = 1,        /* C = bf16(acc + bias[n])                                                    */
  BL_EPI_BIAS_GELU = 2,   /* t = bf16(acc + bias[n]);  C = bf16(gelu_erf(t))                            */
  BL_EPI_BIAS_RES = 3,    /* t = bf16(acc + bias[n]);  [t = bf16(t*scale[n])];  C = bf16(res + t)       */
  BL_EPI_RES = 4,         /* t = bf16(acc);            C = bf16(res + t)                                */
  BL_EPI_SWIGLU = 5,      /* W rows interleaved (2j = gate_j, 2j+1 = up_j); C[m, j] = silu(g)*u, N/2 wide */
  BL_EPI_F32 = 6,         /* C = acc  (fp32 output)                                                     */
  BL_EPI_F32_BF16R = 7,   /* C = (float)bf16(acc): HF `lm_head(h).float()` — logits are bf16 values upcast     */
  /* Training-step forms (bl_gemm_bf16 only; what autograd keeps / computes around the same nn.Linear under
   * `loss.backward()`, prismatic/training/strategies/base_strategy.py:296-302). The *_KEEP forms write the pre-activation
   * to C (autograd's saved tensor) AND the activation to C2; the *_BWD forms apply the activation's backward to the
   * input-gradient GEMM's result, reading the saved pre-activation through `res`. Bit-identical to the plain epilogue
   * followed by bl_swiglu_bf16 / bl_gelu_bf16 / bl_swiglu_backward_bf16 / bl_gelu_backward_bf16. */
  BL_EPI_SWIGLU_KEEP = 8,     /* C[m, n] = bf16(acc) (gate/up interleaved, N wide); C2[m, j] = silu(g)*u (N/2 wide)  */
  BL_EPI_BIAS_GELU_KEEP = 9,  /* C = t = bf16(acc + bias[n]);  C2 = bf16(gelu_erf(t))                                */
  BL_EPI_SWIGLU_BWD = 10,     /* d = bf16(acc) = dL/d act[m, n];  res = saved gate/up [m, 2n..]; C[m, 2n..2n+1] = (d gate, d up) — C is 2N wide */
  BL_EPI_GELU_BWD = 11        /* d = bf16(acc) = dL/d gelu(t)[m, n];  res = saved t;  C = bf16(d * gelu'(t))          */
};

typedef struct bl_gemm_desc {
  const bl_bf16* A;  int64_t lda;      /* [M, K] activations                                                  */
  const bl_bf16* W;  int64_t ldw;      /* [N, K] weights, fragment-major (bl_pack_weight_bf16); ldw must equal K */
  void* C;           int64_t ldc;      /* [M, N] (or [M, N/2] for SWIGLU); bf16, or fp32 for BL_EPI_F32*      */
  int32_t M, N, K;                     /* K % 64 == 0 (pad in HBM), N % 16 == 0                               */
  int32_t epilogue;                    /* enum bl_epilogue                                                    */
  const bl_bf16* bias;                 /* [N] or NULL                                                         */
  const bl_bf16* scale;                /* [N] LayerScale (modeling_prismatic.py:52-59) or NULL                */
  const bl_bf16* res; int64_t ldres;   /* residual / additive table; row = res_row_mod ? m % res_row_mod : m  */
  int32_t res_row_mod;
  /* output-row remap: out_row = (m / out_group) * out_stride + (m % out_group) + out_offset; rows whose
   * (m % out_group) + out_offset falls outside [0, out_stride) are dropped. out_group == 0 → identity.
   * Used to write patch-embeddings behind the cls/register tokens, to strip prefix tokens at the ViT tap
   * (modeling_prismatic.py:85-87,121-123) and to write projector output straight into LLM embedding rows 1..256
   * (modeling_prismatic.py:383-385). */
  int32_t out_group, out_stride, out_offset;
  /* Optional fused HF LlamaRMSNorm on the A operand (bl_gemm_skinny_bf16 only): A rows are normalised in registers as
   * t = bf16(a * rsqrt(mean(a^2) + eps)), a' = bf16(a_norm_weight[k] * t) before the product. NULL = off. */
  const bl_bf16* a_norm_weight;
  float a_norm_eps;
  /* Optional scratch for bl_gemm_bf16's split-K tail (fp32 partial tiles of the last, partially filled round of
   * 256x256 tiles); 64 MiB always suffices. NULL / too small → the tail runs as 128x128 tiles instead. Contents are
   * undefined after the call; calls that share a workspace must be ordered on one stream. */
  void* workspace;
  int64_t workspace_bytes;
  /* second output of the BL_EPI_*_KEEP epilogues (bf16); NULL otherwise */
  bl_bf16* C2;
  int64_t ldc2;
} bl_gemm_desc;

int bl_gemm_bf16(const bl_gemm_desc* d, void* stream);

/* Skinny GEMM for M <= 16 rows (decode steps and last-row lm_head): weight-streaming, HBM-bound.
 * Supports BL_EPI_NONE / BL_EPI_RES / BL_EPI_SWIGLU / BL_EPI_F32 / BL_EPI_F32_BF16R. Replaces the same nn.Linear modules on the
 * cached-decode branch (modeling_prismatic.py:325-341). */
int bl_gemm_skinny_bf16(const bl_gemm_desc* d, void* stream);

/* The skinny kernel's arithmetic for 16 < M <= 128 stacked rows: the same 8-way K partition (slice w = K/8 contiguous
 * columns), the same per-slice k order on the MFMA, the same slice-order fp32 combine and fused epilogue, so every row's
 * result is bit-identical to bl_gemm_skinny_bf16 on that row alone — whatever batch or row position it is computed in.
 * Used by the merged decode iteration of StaggeredDecodePipeline (the decode steps of n_new-1 batches stacked into one
 * pass over the weights; same nn.Linear modules on the cached-decode branch, modeling_prismatic.py:325-341).
 * K % 256 == 0; epilogues as bl_gemm_skinny_bf16; no out_map, no fused a_norm (see bl_rmsnorm_skinny_bf16). */
int bl_gemm_skinny_rows_bf16(const bl_gemm_desc* d, void* stream);

/* Weight gradient of an nn.Linear straight from row-major buffers: C[M, N] (fp32, BL_EPI_F32 only) = A^T * W with
 * A = dy [K token rows, M] (lda) and W = x [K token rows, N] (ldw), both row-major bf16 — what autograd computes for
 * `weight.grad` in loss.backward() (base_strategy.py:301; torch.nn.functional.linear backward). K is arbitrary (token
 * rows past the end read as zeros); M, N multiples of 8. workspace (optional): fp32 scratch for a K-split last round. */
int bl_gemm_tn_bf16(const bl_gemm_desc* d, void* stream);

/* Which kernel form the calling thread's last bl_gemm_bf16 / bl_gemm_skinny_bf16 / bl_gemm_skinny_rows_bf16 /
 * bl_gemm_tn_bf16 / bl_gemm_fp8 call launched (0: none — the call returned an error before launching). A host-side, thread-local
 * record for tests; it takes no part in dispatch. Bits 0-7 main kernel, 8-11 and 12-15 its template parameters,
 * 16-21 K slices (skinny kernel: k-steps per wave), 22-24 tail treatment, 25-29 split-K tail slices; the codes are in
 * csrc/gemm_plan.h and decoded by ops.gemm_last_form(). */
int bl_gemm_last_form(void);

/* HF LlamaRMSNorm (transformers modeling_llama.py LlamaRMSNorm.forward; called per decoder layer from the cached-decode
 * branch, modeling_prismatic.py:325-341) in exactly the arithmetic of bl_gemm_skinny_bf16's fused a_norm (same
 * sum-of-squares order, same two roundings): y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))). dim in {512, 1024, 1536,
 * 4096, 5120, 11008, 13824}. norm kernel + bl_gemm_skinny_rows_bf16 == bl_gemm_skinny_bf16 with a_norm, bit for bit. */
int bl_rmsnorm_skinny_bf16(const bl_bf16* x, int64_t ldx, const bl_bf16* w, bl_bf16* y, int64_t ldy, int32_t rows,
                           int32_t dim, float eps, void* stream);

/* ---- FP8 (OCP e4m3) GEMM family — BASELINE configs[4] "fp8 MFMA GEMMs"; the reference has no fp8 path ------------- */
/* C = epilogue(scale_a[m] * scale_w[n] * (A8 @ W8^T)) on v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales, 2x the
 * bf16 MFMA rate). d->A: e4m3 codes [M, K] (lda in bytes, % 16), d->W: e4m3 weight in the fragment-major packing of
 * bl_pack_weight_bf16 applied to the [N, K/2] matrix of byte pairs, K % 128 == 0; scale_a fp32 [M] (per token),
 * scale_w fp32 [N] (per output channel, 16-byte aligned). Epilogues, bias / residual / output as bl_gemm_bf16; no
 * workspace, no fused A-norm. One form for every shape (gemm256s_fp8_kernel, planned by plan_gemm_fp8), which
 * bl_gemm_last_form reports as "gemm256s_fp8". */
int bl_gemm_fp8(const bl_gemm_desc* d, const float* scale_a, const float* scale_w, void* stream);
/* x bf16 [rows, cols] (cols % 8 == 0) -> q e4m3 [rows, cols] (ldq bytes) + scales[row] = amax(row) / 448;
 * q = RNE_e4m3(x * (448 / amax)). A row with amax < 2^-100 counts as a zero row: scale 1, every code a signed zero (448 / amax
 * overflows below 1.3e-36). */
int bl_quantize_rows_fp8(const bl_bf16* x, int64_t ldx, int32_t rows, int32_t cols, uint8_t* q, int64_t ldq, float* scales,
                         void* stream);
/* Weight-gradient operands of the e4m3 path (dW = dyT . x contracts over tokens: one scale per CHANNEL, token-contiguous
 * codes). bl_colamax_bf16: amax[c] = max_t |x[t, c]| into a PRE-ZEROED fp32 vector (atomic max; several calls may
 * accumulate into one vector). bl_transpose_quantize_fp8: x bf16 [rows = tokens, cols = channels] -> e4m3 codes
 * q[c][t] = rne(x[t, c] * 448 / amax[c]), tokens zero-padded to ldq (a multiple of 64), scales[c] = amax[c] / 448 (1, with
 * zero codes, for a channel with amax[c] < 2^-100); packed = 0: q row-major [cols, ldq] (bl_gemm_fp8's activation operand), packed = 1: q in the
 * fragment-major packing of its weight operand, [cols/16][ldq/64][64][16 B]. No reference counterpart. */
int bl_colamax_bf16(const bl_bf16* x, int64_t ldx, int32_t rows, int32_t cols, float* amax, void* stream);
int bl_transpose_quantize_fp8(const bl_bf16* x, int64_t ldx, int32_t rows, int32_t cols, const float* amax, uint8_t* q,
                              int64_t ldq, int32_t packed, float* scales, void* stream);

/* ---- normalisation ------------------------------------------------------------------------------------------ */
/* timm Block.norm1/norm2: LayerNorm(eps, affine), fp32 statistics, bf16 out. y may alias x. */
int bl_layernorm_bf16(const bl_bf16* x, int64_t ldx, const bl_bf16* w, const bl_bf16* b, bl_bf16* y, int64_t ldy,
                      int32_t rows, int32_t dim, float eps, void* stream);
/* HF LlamaRMSNorm: t = bf16(x * rsqrt(mean(x^2) + eps)); y = bf16(w * t). */
int bl_rmsnorm_bf16(const bl_bf16* x, int64_t ldx, const bl_bf16* w, bl_bf16* y, int64_t ldy, int32_t rows,
                    int32_t dim, float eps, void* stream);

/* ---- attention ---------------------------------------------------------------------------------------------- */
/* Flash-style softmax(q k^T * scale [+ causal] [+ key mask]) v, fp32 scores/softmax, bf16 P for the PV product.
 * Replaces timm Attention (SDPA, non-causal, head_dim 64 / 72) and HF LlamaAttention prefill (causal, head_dim 128;
 * the reference callers hard-wire flash_attention_2 / sdpa: deploy.py:67, run_openvla_demo.py:25).
 * Element strides: *_bs batch, *_hs head, *_rs row (token). head_dim contiguous. key_mask: [B, Skv] uint8 or NULL. */
typedef struct bl_attn_desc {
  const bl_bf16* q; int64_t q_bs, q_hs, q_rs;
  const bl_bf16* k; int64_t k_bs, k_hs, k_rs;
  const bl_bf16* v; int64_t v_bs, v_hs, v_rs;
  bl_bf16* o;       int64_t o_bs, o_hs, o_rs;
  const uint8_t* key_mask; int64_t mask_bs;
  int32_t B, H, Sq, Skv, head_dim;
  int32_t causal;      /* 1: key j visible to query i iff j <= i + (Skv - Sq) */
  float scale;         /* head_dim^-0.5 */
} bl_attn_desc;
int bl_attention_bf16(const bl_attn_desc* d, void* stream);
/* Prefill attention with the rotary embedding and the KV-cache write fused in (HF apply_rotary_pos_emb +
 * DynamicCache.update + attention of LlamaAttention.forward in one pass): d->q / d->k / d->v are the UN-rotated thirds of the
 * fused qkv rows; q and k are rotated at positions pos0 + row while they are loaded (same three bf16 roundings as
 * bl_rope_kvcache_bf16), the rotated k and v rows are written to k_cache / v_cache [B, H, cache_len, 128]. head_dim 128,
 * causal, Skv == Sq <= 320. The qkv buffer is left untouched. */
int bl_attention_rope_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t pos0, bl_bf16* k_cache,
                           bl_bf16* v_cache, int32_t cache_len, void* stream);
/* Training forward: as bl_attention_bf16, and also writes the base-2 log-sum-exp of the scaled scores of every query
 * row to lse[(b*H + h) * pad32(Sq) + i] (fp32; +inf for a row with no visible key) for bl_attention_backward_bf16. */
int bl_attention_lse_bf16(const bl_attn_desc* d, float* lse, void* stream);
/* Backward of bl_attention_bf16 (what autograd runs under HF LlamaAttention / timm Attention in the reference's
 * `loss.backward()`, prismatic/training/strategies/base_strategy.py:300). d describes the forward call (o = its
 * output); dout uses o's strides; dq / dk / dv use q's / k's / v's strides (so they can alias the three thirds of a
 * fused dqkv row). lse from bl_attention_lse_bf16; delta is scratch of the same size, [B*H*pad32(Sq)] fp32.
 * Any Sq, Skv (causal: Skv >= Sq): up to 320 positions one workgroup per (batch, head) holds the whole sequence in LDS;
 * longer sequences (the collator pads to model_max_length = 2048, prismatic/util/data_utils.py:101-142) stream 256-row
 * chunks against 128-row register blocks — same summation order, same bits. All strides multiples of 8. */
int bl_attention_backward_bf16(const bl_attn_desc* d, const bl_bf16* dout, const float* lse, float* delta, bl_bf16* dq,
                               bl_bf16* dk, bl_bf16* dv, void* stream);
/* Attention over a shared prompt and its branches (the shared-prompt training step), forward with lse and backward.
 * d describes one row of the layout  prefix (rows [0, prefix)) | branch 0 (`branch` rows) | ... | branch G-1  per batch element:
 * Sq == Skv == prefix + G*branch, head_dim 128, causal = 1, key_mask [B, Skv] or NULL. Key j is visible to query i iff
 * key_mask[j] != 0, j <= i, and (j < prefix, or i >= prefix and (i - prefix) / branch == (j - prefix) / branch). The branches
 * read the prefix K / V rows in place (no copy per branch); the backward sums every branch's contribution to the prefix rows
 * of dk / dv in row order inside one wave (no atomics, no workspace; two calls give the same bits). Arithmetic contract, lse
 * (base 2, +inf for a row with no visible key) and the aliasing rules of dq / dk / dv as bl_attention_lse_bf16 /
 * bl_attention_backward_bf16. lse and delta (scratch) are fp32 [B*H*pad32(Sq)], 16-byte aligned, indexed
 * (b*H + h) * pad32(Sq) + i; the pair is the tree kernels' own. Any Sq up to model_max_length. BL_E_ARG for prefix < 1 or
 * branch < 1; BL_E_SHAPE for (Sq - prefix) % branch != 0, prefix > Sq, Skv != Sq, causal == 0, head_dim != 128 or a stride
 * that is not a multiple of 8; nothing is launched then. */
int bl_attention_tree_lse_bf16(const bl_attn_desc* d, int32_t prefix, int32_t branch, float* lse, void* stream);
int bl_attention_tree_backward_bf16(const bl_attn_desc* d, int32_t prefix, int32_t branch, const bl_bf16* dout, const float* lse,
                                    float* delta, bl_bf16* dq, bl_bf16* dk, bl_bf16* dv, void* stream);
/* bl_rope_bf16 / bl_rope_backward_bf16 with a position per row: row r of the fused qkv (dqkv) rows [rows, ld] is rotated at
 * position pos[r] (device int32 [rows], a static buffer of the caller; a negative entry counts as 0 and every entry must lie
 * inside the tables). The same expressions, so with pos[r] = pos0 + r % S the same bits as those two. */
int bl_rope_pos_bf16(bl_bf16* qkv, int64_t ld, int64_t rows, int32_t H, int32_t head_dim, const bl_bf16* cos_tab,
                     const bl_bf16* sin_tab, const int32_t* pos, void* stream);
int bl_rope_pos_backward_bf16(bl_bf16* dqkv, int64_t ld, int64_t rows, int32_t H, int32_t head_dim, const bl_bf16* cos_tab,
                              const bl_bf16* sin_tab, const int32_t* pos, void* stream);
/* Single-query decode attention over a KV cache; kv_len = number of valid keys (same for the whole batch). */
int bl_attention_decode_bf16(const bl_attn_desc* d, void* stream);
/* The attention probabilities themselves (what HF returns as `attentions`), read-only: P = softmax over the visible keys of
 * q k^T * scale, in fp32, never rounded to bf16. Uses d->q (any strides that are multiples of 8, the fused-qkv row stride
 * included), d->k (ROTATED keys, e.g. a KV-cache view), d->key_mask, B, H, Sq, Skv, scale, causal; d->v and d->o are ignored.
 * head_dim 128 and Skv <= 2048, else BL_E_SHAPE. Key j is visible to query i iff key_mask[b][j] != 0 and (not causal or
 * j <= i + Skv - Sq). K rows >= Skv are never read and rows of hidden keys may hold anything, NaN included.
 *   q: cos_tab == sin_tab == NULL: already rotated in memory. Otherwise un-rotated: row i of sequence b is rotated on load at
 *      position pos0 + i, or rope_pos[b] + i when rope_pos (device int32 [B]) is given, with the arithmetic of
 *      bl_rope_kvcache_bf16 bit for bit; tables [rope_rows, 64] bf16 (a position outside them is clamped).
 *   probs (or NULL): fp32, element strides p_bs / p_hs / p_rs, columns [0, Skv) = P (0 for hidden keys, a row without a
 *      visible key is all 0), columns [Skv, p_cols) = 0: no memset needed, nothing outside [0, p_cols) is written.
 *   seg (or NULL): fp32 [B, H, Sq, n_seg], n_seg <= 8: seg[b][h][i][s] = sum of P over keys [bounds[b][s], bounds[b][s+1]),
 *      seg_bounds device int32 [B, n_seg + 1], non-decreasing, clipped to [0, Skv] by the kernel.
 * A row's results do not depend on the other rows of the launch: Sq = S and S calls with Sq = 1 agree bit for bit.
 * Definition: bridgelang_amd/attention_taps.py::probs_reference. */
int bl_attention_probs_f32(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t rope_rows, int32_t pos0,
                           const int32_t* rope_pos, float* probs, int64_t p_bs, int64_t p_hs, int64_t p_rs, int32_t p_cols,
                           float* seg, const int32_t* seg_bounds, int32_t n_seg, void* stream);

/* Training forward: rotate q and k of the fused qkv rows IN PLACE (same arithmetic as bl_rope_kvcache_bf16, no cache). */
int bl_rope_bf16(bl_bf16* qkv, int64_t ld, int32_t B, int32_t S, int32_t H, int32_t head_dim, const bl_bf16* cos_tab,
                 const bl_bf16* sin_tab, int32_t pos0, void* stream);

/* Decode attention with the rotary embedding and the KV-cache append of the NEW token fused in: q / k_new / v_new are
 * the three thirds of the step's fused qkv row (strides d->q_*; k_new = q + H*hd, v_new = q + 2*H*hd elements). q and
 * k_new are rotated at position `pos` (HF apply_rotary_pos_emb, bf16 roundings as bl_rope_kvcache_bf16), k_new', v_new
 * are written to cache row `pos` of d->k / d->v, and attention runs over keys 0..pos (d->Skv must equal pos + 1). */
int bl_attention_decode_rope_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t pos,
                                  void* stream);
/* bl_attention_decode_rope_bf16 for a batch of RIGHT-PADDED prompts (HF generation with an attention mask,
 * modeling_prismatic.py:387-390 + transformers' position_ids = cumsum(mask) - 1): sequence b's new token sits at ITS
 * position rope_pos[b] (device int32 [B]) = the number of real tokens before it — that is its rotation angle, the cache
 * row its k / v are written to (over the pad rows' entries) and its key count - 1; `pos` = max_b rope_pos[b] bounds the
 * cache. The cache of every sequence is then laid out exactly as in its own un-padded run: identical results, bit for
 * bit. */
int bl_attention_decode_rope_pos_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t pos,
                                      const int32_t* rope_pos, void* stream);

/* n_groups (<= 8) decode iterations of DIFFERENT batches in one launch (continuous batching, pipeline.py): rows
 * g*B .. (g+1)*B-1 of the fused qkv / output buffers belong to group g, which has its own KV caches
 * k_caches[g] / v_caches[g] ([B, H, cache_len, 128], strides from d->k_* / d->v_*) and position pos[g]. The three arrays
 * are HOST arrays read at call time. d->k / d->v / d->Skv are ignored. Per group identical to
 * bl_attention_decode_rope_bf16. */
int bl_attention_decode_rope_grouped_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t n_groups,
                                          bl_bf16* const* k_caches, bl_bf16* const* v_caches, const int32_t* pos, void* stream);
/* The grouped form for RIGHT-PADDED batches (StaggeredDecodePipeline(padded=True)): group g carries a DEVICE array
 * rope_pos[g] (int32 [B]) in place of the one host position; sequence b of group g rotates, appends and attends at
 * rope_pos[g][b], as in bl_attention_decode_rope_pos_bf16 — per row bit-identical to that call on the group alone, and to
 * bl_attention_decode_rope_bf16 where a group's positions coincide. The pointer arrays are HOST arrays read at call time;
 * the positions are read by the kernel, so nothing on the host can check them: a sequence whose position lies outside
 * [0, cache_len) is skipped (no cache write, no output). cache_len <= 2048 rows per head (d->k_hs / d->v_hs must hold
 * them), and cos_tab / sin_tab must hold at least cache_len rows: the call cannot see their length. d->k / d->v / d->Skv
 * are ignored and d->key_mask must be NULL. */
int bl_attention_decode_rope_pos_grouped_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab,
                                              int32_t n_groups, bl_bf16* const* k_caches, bl_bf16* const* v_caches,
                                              const int32_t* const* rope_pos, int32_t cache_len, void* stream);
/* bl_attention_decode_rope_bf16 for rows that SHARE a prompt (samples of one observation, candidates, beams), without a copy
 * of the prompt's cache rows: d->q is the step's fused qkv [R, 3*H*128] of R = P*group rows (d->B = R), row r belongs to
 * prompt p = r / group. d->k / d->v are the PROMPT caches [P, H, cache_len, 128] (strides d->k_* / d->v_*, batch stride per
 * prompt), read only; k_gen / v_gen are contiguous [R, H, gen_len, 128] caches of the rows' own generated tokens. Row r's
 * keys 0 … prefix_len-1 are prompt p's cache rows, keys prefix_len … pos-1 rows 0 … pos-prefix_len-1 of its own gen cache,
 * and key `pos` is the step's new token, rotated at `pos` and appended to gen row pos - prefix_len. o [R, H*128]
 * (d->o_*); d->Skv must equal pos + 1. Per row bit-identical to bl_attention_decode_rope_bf16 on caches that hold the
 * prompt rows followed by the generated rows. One workgroup serves several rows of one (prompt, head) and loads each prompt
 * row once for all of them. head_dim != 128, group outside 1 … 16, R % group != 0, prefix_len < 1, pos < prefix_len,
 * pos - prefix_len >= gen_len, pos >= 2048 or a cache head stride that does not hold prefix_len rows: BL_E_SHAPE; a NULL
 * pointer or a key mask in the descriptor (every row attends to all of its keys, at one common position): BL_E_ARG; nothing
 * is launched on a rejection. */
int bl_attention_decode_rope_shared_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t pos,
                                         int32_t group, int32_t prefix_len, bl_bf16* k_gen, bl_bf16* v_gen, int32_t gen_len,
                                         void* stream);
/* The same with the rows per workgroup given: gq in {2, 4, 8} (else BL_E_ARG). Every gq gives the same bits; the entry point
 * above uses the one measured fastest (tools/bench_shared_prefill.py times all three). */
int bl_attention_decode_rope_shared_gq_bf16(const bl_attn_desc* d, const bl_bf16* cos_tab, const bl_bf16* sin_tab, int32_t pos,
                                            int32_t group, int32_t prefix_len, bl_bf16* k_gen, bl_bf16* v_gen, int32_t gen_len,
                                            int32_t gq, void* stream);
/* dst[r * group + j, :cols] = src[r, :cols] for r < rows, j < group: every bf16 row replicated group-fold (the step-0 residual
 * rows of a shared prefill). 16-byte copies: cols, ld_src, ld_dst multiples of 8 (BL_E_SHAPE / BL_E_ALIGN). */
int bl_repeat_rows_bf16(const bl_bf16* src, int64_t ld_src, bl_bf16* dst, int64_t ld_dst, int64_t rows, int32_t cols,
                        int32_t group, void* stream);

/* ---- Llama glue -------------------------------------------------------------------------------------------- */
/* Half-split RoPE (HF apply_rotary_pos_emb) on the q and k thirds of a fused qkv buffer [B*S, 3*H*hd], bf16 cos/sin
 * tables [max_pos, hd/2] (built on the host exactly as HF does: fp32 trig → bf16). q is rotated in place; rotated k
 * and v are appended to the KV cache [B, H, cache_len, hd] at positions pos0 .. pos0+S-1. */
int bl_rope_kvcache_bf16(bl_bf16* qkv, int32_t B, int32_t S, int32_t H, int32_t hd, const bl_bf16* cos_tab,
                         const bl_bf16* sin_tab, int32_t pos0, bl_bf16* k_cache, bl_bf16* v_cache,
                         int32_t cache_len, void* stream);
/* Token-embedding gather for the multimodal splice (modeling_prismatic.py:380-385): writes
 * dst[b, 0] = table[ids[b,0]] and dst[b, 1+n_patches+j] = table[ids[b,1+j]]; rows 1..n_patches are left for the
 * projector epilogue. ids int64 [B, L]; dst [B, L+n_patches, dim]. With n_patches = 0 it is a plain gather. */
int bl_embed_splice_bf16(const int64_t* ids, int32_t B, int32_t L, const bl_bf16* table, int32_t dim,
                         int32_t n_patches, bl_bf16* dst, void* stream);
/* dst[b, :width] = src[b, row_index[b], :width] for b < B: src is [B, rows_per_batch] rows of row_stride elements, dst a
 * dense [B, width]; row_index is a DEVICE int64 [B] (the last real position of each right-padded prompt). 16-byte copies:
 * width and row_stride multiples of 8. An index outside [0, rows_per_batch) copies nothing for that row. */
int bl_gather_rows_bf16(const bl_bf16* src, const int64_t* row_index, int64_t rows_per_batch, int64_t row_stride,
                        int32_t width, bl_bf16* dst, int32_t B, void* stream);
/* Row-wise argmax of fp32 logits [rows, n] (row stride ld >= n) as torch.argmax: the first NaN of the row, else the first
 * maximal index, so always an index in [0, n); out int64 [rows]. */
int bl_argmax_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, int64_t* out, void* stream);
/* Seeded sampling of one token per row of fp32 logits [rows, n] (leading dimension ld; columns >= n are never read):
 * temperature → top-k → top-p → one Philox4x32-10 draw, bit-identical to bridgelang_amd/sampling.py::sample_rows. The
 * settings are DEVICE arrays with one entry per row — temperature fp32 (0 = greedy: the row's answer is bl_argmax_f32's),
 * top_k int32 (0 = off), top_p fp32 (>= 1 = off), seed int64 (the Philox key; the counter is `step`) — so one captured
 * graph serves any settings. ids int64 [rows]; wt int64 [rows, 2] = (weight of the drawn token, kept total): its
 * probability under the warped distribution is their quotient. n % 4 == 0 and n <= 36480 (the row's weights live in LDS),
 * else BL_E_SHAPE. */
int bl_sample_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                  const int32_t* top_k, const float* top_p, const int64_t* seed, int32_t step, int64_t* ids,
                  int64_t* wt, void* stream);
/* The score of a GIVEN token per row under the same warped distribution: bl_sample_f32 with the draw replaced by a read,
 * bit-identical to bridgelang_amd/sampling.py::score_rows. tokens int64 [rows]; wt int64 [rows, 2] = (kept weight of
 * tokens[row], kept total) — weight 0 for a token that top-k or top-p removed or whose weight rounds to 0; a greedy row
 * (temperature 0) scores (token == argmax, 1). A token outside [0, n) is a caller error; the kernel reads nothing for it
 * and writes (0, kept total). range_count > 0 also writes range_wt int32 [rows, range_count]: the kept weights of tokens
 * range_first … range_first + range_count - 1 (a greedy row: the one-hot of its argmax); it needs 0 <= range_first and
 * range_first + range_count <= n (else BL_E_SHAPE); range_count == 0 ignores range_wt (may be NULL). Shapes and alignment
 * as bl_sample_f32. */
int bl_score_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                 const int32_t* top_k, const float* top_p, const int64_t* tokens, int64_t* wt,
                 int32_t range_first, int32_t range_count, int32_t* range_wt, void* stream);
/* bl_sample_f32 with the policy restricted to the token range [vocab_first, vocab_first + vocab_count) of every row: the
 * draw is from the softmax of logits[vocab_first : vocab_first + vocab_count] alone (maximum, top-k, top-p and the greedy
 * argmax are all taken over the range; bit-identical to sampling.py::sample_rows(vocab=(first, count))), ids are in
 * full-row numbering, and no column outside the range is read. vocab_first % 4 == 0, vocab_count % 4 == 0,
 * 0 < vocab_count <= 36480 and the range inside [0, n), else BL_E_SHAPE. (0, n) is bl_sample_f32 bit for bit. */
int bl_sample_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                        const int32_t* top_k, const float* top_p, const int64_t* seed, int32_t step, int64_t* ids,
                        int64_t* wt, int32_t vocab_first, int32_t vocab_count, void* stream);
/* bl_score_f32 under the same restricted policy (sampling.py::score_rows(vocab=(first, count))): a token outside the
 * vocabulary range scores (0, kept total), like a token that top-k removed. range_first keeps full-row numbering; the
 * report range must lie inside the vocabulary range (else BL_E_SHAPE). Other constraints as bl_sample_range_f32. */
int bl_score_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const float* temperature,
                       const int32_t* top_k, const float* top_p, const int64_t* tokens, int64_t* wt,
                       int32_t range_first, int32_t range_count, int32_t* range_wt, int32_t vocab_first,
                       int32_t vocab_count, void* stream);
/* One step of beam search, bit-identical to bridgelang_amd/beam.py::beam_step: logits [groups * W, n] (row stride ld); the W
 * rows of a group are the beams of one prompt, scores_in fp32 [groups * W] their joint log-probabilities so far. Over the
 * token range [vocab_first, vocab_first + vocab_count) of every row, candidate (j, i) scores
 * c = ((scores_in[j] + (l_i - max_j)) - lz_j), each operation rounded alone, lz_j the log of the row's integer softmax total
 * (bl_sample_f32's weights at temperature 1). The W survivors of a group, in the order c descending then j * vocab_count + i
 * ascending, go to slot k = 0 … W-1 of the group: tokens int64 (full-row numbering), parents int32 (j, in [0, W)), wt int64
 * [., 2] = (weight of the token on row j, that row's total: bl_score_range_f32's pair under the default settings) and
 * scores_out fp32 (c). Step 0 passes scores_in = (0, -inf, …). Two launches on `stream`: one workgroup per row (maximum and
 * total, kept in that row's wt pair in between), then one workgroup per group, which reads all of its inputs before it writes
 * any output, so scores_out may be scores_in. W in 1 … 16 and W <= vocab_count, other shapes as bl_sample_range_f32, else
 * BL_E_SHAPE; a NULL pointer: BL_E_ARG; nothing is launched on a rejection. */
int bl_beam_step_f32(const float* logits, int64_t ld, int32_t groups, int32_t W, int32_t n, const float* scores_in,
                     int64_t* tokens, int32_t* parents, int64_t* wt, float* scores_out, int32_t vocab_first,
                     int32_t vocab_count, void* stream);
/* The KV-cache half of a beam step, in place: in each of the n_caches bf16 caches [rows, H, cache_len, head_dim] whose base
 * pointers are the DEVICE table `caches`, batch row g * W + k takes the cache rows r0 … r0 + n_rows - 1 of batch row
 * g * W + parents[g * W + k] (parents DEVICE int32 [rows]; an entry outside [0, W) keeps the slot's own rows). r0 = row0, or
 * with row0_dev (DEVICE int32 [rows], right-padded prompts) every batch row's own first generated row; a cache row outside
 * [0, cache_len) moves nothing. A workgroup owns all W slots of one (cache, prompt, head, cache row): it loads them, barriers,
 * then stores, so a parent may have several children or be overwritten; everything outside the moved rows is untouched.
 * One launch for the whole table. rows % W == 0, W in 1 … 16, head_dim % 8 == 0, W * head_dim <= 4096, row0 + n_rows <=
 * cache_len, else BL_E_SHAPE; NULL caches / parents: BL_E_ARG; nothing is launched on a rejection. */
int bl_beam_reorder_kv_bf16(bl_bf16* const* caches, int32_t n_caches, int32_t rows, int32_t W, int32_t H, int32_t cache_len,
                            int32_t head_dim, const int32_t* parents, int32_t row0, const int32_t* row0_dev, int32_t n_rows,
                            void* stream);

/* Shifted causal-LM cross-entropy (HF LlamaForCausalLM loss; labels prepared by the caller as `targets[row]` =
 * label of the NEXT position, -100 = ignore; base_strategy.py:287-297 consumes `output.loss`). row_loss[rows] receives
 * the per-row loss (0 where ignored); mean_and_count[0] = mean over valid rows, [1] = number of valid rows. A target
 * outside [0, n) other than ignore_index indexes nothing: its row_loss and the mean are NaN, and it counts as valid.
 * Row stride ld >= n. */
int bl_cross_entropy_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                         int64_t ignore_index, float* row_loss, float* mean_and_count, void* stream);

/* ---- training step: backward + optimizer (base_strategy.py:284-366, fsdp.py:190-246) --------------------------------- */
/* Activation gradients are bf16, parameter gradients / AdamW state / master weights fp32 (train.py:156-157,
 * fsdp.py:140-146). Reductions are deterministic (per-block partials in caller-provided workspaces + a second pass). */
/* dlogits = (softmax(logits) - onehot(target)) / n_valid (0 on ignored rows); mean_and_count from bl_cross_entropy_f32. */
int bl_cross_entropy_backward_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                  int64_t ignore_index, const float* mean_and_count, bl_bf16* dlogits, int64_t ldd,
                                  void* stream);
/* Clipped-surrogate policy-gradient loss (PPO / GRPO form) over the same logits rows and `targets` convention as
 * bl_cross_entropy_f32; bridgelang_amd/training/policy_loss.py is the fp64 definition. With z = logits / temperature,
 * logp = log_softmax(z)[target], ratio = exp(logp - old_logprob[row]):
 *   row_loss = -min(ratio*A, clip(ratio, 1 - clip_low, 1 + clip_high)*A) - entropy_coef*H(softmax(z))
 *              + kl_coef*(exp(d) - d - 1),  d = ref_logprob[row] - logp   (ref_logprob NULL: no KL term).
 * advantages / old_logprob / ref_logprob fp32 [rows], read on valid rows only. row_stats fp32 [rows, 8] receives
 * (logp, H, ratio, row_loss, clipped 0/1, max z, log sum exp(z - max), d row_loss / d logp), zeros on ignored rows.
 * stats fp32 [8] = (loss, n_valid, mean pg, mean H, mean kl, clipped fraction, mean (ratio - 1) - log ratio, mean ratio)
 * over valid rows in a fixed summation order. n % 8 == 0, ld % 4 == 0, logits 16-byte aligned. */
int bl_policy_loss_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                       int64_t ignore_index, const float* advantages, const float* old_logprob, const float* ref_logprob,
                       float temperature, float clip_low, float clip_high, float entropy_coef, float kl_coef,
                       float* row_stats, float* stats, void* stream);
/* dlogits (bf16) = d loss / d logits from the logits and what bl_policy_loss_f32 saved (same temperature and
 * entropy_coef); stats[1] = n_valid. 0 on ignored rows. ldd % 8 == 0, dlogits 16-byte aligned. */
int bl_policy_loss_backward_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                int64_t ignore_index, const float* row_stats, const float* stats, float temperature,
                                float entropy_coef, bl_bf16* dlogits, int64_t ldd, void* stream);
/* bl_policy_loss_f32 with the policy taken over the token range [vocab_first, vocab_first + vocab_count) of every row
 * (training/policy_loss.py with PolicyLossConfig.token_range): max, sum, entropy and logp are over the range and only the
 * range of a valid row is read. targets stay in full-row numbering; a valid target outside the range gives NaN in that
 * row's statistics, never a stray read. vocab_first % 8 == 0, vocab_count % 8 == 0, the range inside [0, n), else
 * BL_E_SHAPE. (0, n) gives bl_policy_loss_f32's results. */
int bl_policy_loss_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                             int64_t ignore_index, const float* advantages, const float* old_logprob,
                             const float* ref_logprob, float temperature, float clip_low, float clip_high,
                             float entropy_coef, float kl_coef, float* row_stats, float* stats, int32_t vocab_first,
                             int32_t vocab_count, void* stream);
/* bl_policy_loss_backward_f32 for the same range: writes the whole [rows, n] dlogits — exact zeros outside the range and on
 * ignored rows, the gradient inside — and reads logits only inside the range of valid rows. */
int bl_policy_loss_backward_range_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                      int64_t ignore_index, const float* row_stats, const float* stats, float temperature,
                                      float entropy_coef, bl_bf16* dlogits, int64_t ldd, int32_t vocab_first,
                                      int32_t vocab_count, void* stream);
/* bl_policy_loss_range_f32 with the importance ratio taken per ACTION instead of per token (training/policy_loss.py with
 * PolicyLossConfig.ratio_level = "action"). Rows [k*group_rows, (k+1)*group_rows) are one sequence and its valid rows are
 * one group G: s_G = c * sum_G (logp - old_logprob), c = 1 (ratio_norm 0, sum) or 1 / n_G (ratio_norm 1, mean),
 * ratio_G = exp(s_G) is clipped once for the group, and every valid row gets
 *   row_stats ratio = ratio_G, clipped = its advantage's side of the clip, row_loss with the group's surrogate, and
 *   d row_loss / d logp = c * sum_{j in G} (-A_j * ratio_G * [active_j]) - kl_coef * expm1(ref_logprob - logp).
 * Entropy and KL stay per token and loss stays the mean over valid rows. stats keeps its layout: mean ratio, clipped
 * fraction and mean (ratio - 1) - log ratio are over valid rows of the group values. group_stats fp32 [rows / group_rows, 4]
 * = (s_G, ratio_G, n_G, sum_G logp), zeros for a sequence without a valid row. Three launches on `stream` (rows, groups,
 * statistics), deterministic. (vocab_first, vocab_count) = (0, n) is the unranged loss. There is no grouped backward:
 * bl_policy_loss_backward_f32 / bl_policy_loss_backward_range_f32 read H, max z, log sum and d row_loss / d logp from
 * row_stats and n_valid from stats[1], all of which this forward leaves in place. Constraints as
 * bl_policy_loss_range_f32; group_stats NULL is BL_E_ARG; group_rows <= 0, rows % group_rows != 0 or ratio_norm outside
 * {0, 1} is BL_E_SHAPE; nothing is launched on a rejection. */
int bl_policy_loss_grouped_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                               int64_t ignore_index, const float* advantages, const float* old_logprob,
                               const float* ref_logprob, float temperature, float clip_low, float clip_high,
                               float entropy_coef, float kl_coef, float* row_stats, float* stats, int32_t vocab_first,
                               int32_t vocab_count, int32_t group_rows, int32_t ratio_norm, float* group_stats,
                               void* stream);
/* bl_policy_loss_range_f32 (group_rows = 0, group_stats NULL) or bl_policy_loss_grouped_f32 (group_rows > 0, group_stats
 * given) with the ROLLOUT CORRECTION of decoupled PPO (training/policy_loss.py with PolicyLossConfig.rollout_is_cap): the
 * tokens were drawn by a behaviour policy with log-probability behaviour_logprob (mu, fp32 [rows], what the sampler
 * reported), the ratio is clipped around a proximal policy q, and the surrogate carries a truncated importance weight
 * between the two. q is old_logprob, or with old_logprob NULL (self-proximal) the row's own logp of this call taken as a
 * constant: log ratio = 0 exactly, ratio = 1, nothing is clipped. Per valid row, lambda = q - mu at token level, or
 * lambda_G = c * sum_G (q - mu) with the group and the c of ratio_norm at action level (every valid row of G carries it):
 *   rho = exp(lambda),  masked = rho < is_mask_low or rho > is_mask_high,  w = masked ? 0 : min(rho, is_cap),
 *   pg = w * (-min(ratio*A, clip(ratio)*A)),  d row_loss / d logp = w * (surrogate share) + the unchanged KL share.
 * w carries no gradient; entropy and KL are not weighted; a masked row still counts in n_valid. No mask is (0, +inf);
 * is_cap may be +inf. stats keeps its layout (loss and mean pg are the weighted ones; ratio, clipped fraction and
 * approximate KL stay about ratio). is_rows fp32 [rows, 2] = (lambda, w), zeros on ignored rows. is_stats fp32 [8] = means
 * over valid rows, in the summation order of stats, of (w, rho, truncated = not masked and rho > is_cap, masked,
 * rho - 1 - lambda, -lambda), then two zeros. With mu = q bit for bit, is_cap >= 1 and no mask, w = 1 and row_stats,
 * stats and group_stats are bit for bit those of the uncorrected entry point. As many launches as the uncorrected form of
 * the level (two / three), deterministic, no allocation. The gradient is bl_policy_loss_backward_f32 /
 * bl_policy_loss_backward_range_f32, unchanged. Constraints as bl_policy_loss_grouped_f32 except that old_logprob may be
 * NULL; NULL behaviour_logprob / is_rows / is_stats, group_stats given without group_rows > 0 or the reverse, is_cap <= 0,
 * is_mask_low < 0 or is_mask_low >= is_mask_high (NaN included) is BL_E_ARG; group_rows < 0, rows % group_rows != 0 or
 * ratio_norm outside {0, 1} is BL_E_SHAPE; nothing is launched on a rejection. */
int bl_policy_loss_is_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                          int64_t ignore_index, const float* advantages, const float* old_logprob,
                          const float* behaviour_logprob, const float* ref_logprob, float temperature, float clip_low,
                          float clip_high, float entropy_coef, float kl_coef, float* row_stats, float* stats,
                          int32_t vocab_first, int32_t vocab_count, int32_t group_rows, int32_t ratio_norm,
                          float* group_stats, float is_cap, float is_mask_low, float is_mask_high, float* is_rows,
                          float* is_stats, void* stream);
/* The preference-pair loss (DPO family; training/preference_loss.py is the definition) over the same rows. Rows
 * [b*group_rows, (b+1)*group_rows) are sequence b; pair int32 [rows / group_rows] holds +k (chosen side of pair k), -k
 * (rejected side) or 0 (in no pair), k in 1..P; an id outside +-P counts as 0 on the device. With delta_b = c_b * sum over
 * the sequence's valid rows of (logp - ref_logprob) (ref_logprob NULL: reference-free; c_b = 1 for seq_norm 0, 1 / n_b for
 * seq_norm 1), Delta_k = sum_chosen delta_b - sum_rejected delta_b and h_k = beta * Delta_k - margin, the pair's loss is
 *   kind 0 (sigmoid): -(1 - eps) log sigma(h) - eps log sigma(-h), eps = label_smoothing;  kind 1 (ipo): (h / beta -
 *   1 / (2 beta))^2;  kind 2 (hinge): max(0, 1 - h);  plus sft_coef * nll_k, the chosen side's token-mean NLL,
 * and the loss is the mean over the P pairs. P is n_pairs, or *n_pairs_dev (int32 on the device, read by the kernels, kept
 * inside [1, n_pairs]) when that is not NULL: n_pairs is then the capacity of pair_stats and a captured launch serves
 * batches with any number of pairs up to it. Outputs, every element written: row_stats fp32 [rows, 8] as
 * bl_policy_loss_f32 with logp, entropy, max z, log sum, zeros for ratio / row_loss / clipped, and d loss * P / d logp in
 * slot 7; stats fp32 [8] = (loss, P, mean pair loss, accuracy, margin, chosen reward, rejected reward, nll); pair_stats
 * fp32 [n_pairs, 4] = (h, loss, d loss / d h, nll), zeros from row P on; seq_stats fp32 [rows / group_rows, 4] = (delta_b,
 * n_b, sum logp, the sequence's d / d logp without the sft term). Four launches on `stream` (rows, sequences, pairs and
 * statistics, gradient factors), deterministic. The gradient is bl_policy_loss_backward_f32 /
 * bl_policy_loss_backward_range_f32 with entropy_coef = 0: they divide by stats[1] = P. NULL logits / targets / pair / an
 * output, beta <= 0, temperature <= 0, label_smoothing outside [0, 0.5), margin < 0, sft_coef < 0 or n_pairs < 1 is
 * BL_E_ARG; a bad range, rows % group_rows != 0, kind outside {0, 1, 2} or seq_norm outside {0, 1} is BL_E_SHAPE;
 * alignment as bl_policy_loss_range_f32; nothing is launched on a rejection. */
int bl_preference_loss_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                           int64_t ignore_index, const int32_t* pair, const float* ref_logprob, int32_t n_pairs,
                           const int32_t* n_pairs_dev, int32_t group_rows, int32_t kind, int32_t seq_norm, float beta,
                           float label_smoothing, float margin, float sft_coef, float temperature, float* row_stats,
                           float* stats, float* pair_stats, float* seq_stats, int32_t vocab_first, int32_t vocab_count,
                           void* stream);
/* The distribution-matching (distillation) loss over the same rows and `targets` convention (training/distill_loss.py is
 * the fp64 definition): the student is the softmax of logits / temperature over the token range [vocab_first, vocab_first +
 * vocab_count) of every row, exactly as in bl_policy_loss_range_f32, and it is compared with a TEACHER row q >= 0. teacher
 * is fp32 [rows, vocab_count] with leading dimension ldt, in ROW layout: row r is row r's teacher and column j is token
 * vocab_first + j. With p, logp of the student, Q = sum q and
 *   kind 0 (forward_kl): D = sum q (log q - logp),                                        c = Q
 *   kind 1 (reverse_kl): D = sum p (logp - log q),                                        c = D
 *   kind 2 (jsd): mi = beta q + (1 - beta) p,  D = beta sum q log(q / mi) + c,            c = (1 - beta) sum p log(p / mi)
 * (a term whose weight q or p is 0 is 0), row_loss = D + sft_coef * (-logp[target]) and the loss is the mean over valid
 * rows. beta is read by kind 2 only. There is no temperature^2 factor. Outputs, every element written: row_stats fp32
 * [rows, 8] = (logp[target], H, D, row_loss, agree 0/1 = student and teacher share their first argmax, max z, log sum
 * exp(z - max), c), zeros on ignored rows; stats fp32 [8] = (loss, n_valid, mean D, mean H, mean teacher entropy
 * -sum q log q, agreement, mean -logp[target], mean |sum_j j (p_j - q_j)| with j counted from vocab_first) over valid rows
 * in a fixed summation order, all exactly 0 when every row is ignored. Two launches on `stream` (rows: one workgroup per
 * row, or one wave per row for vocab_count <= 256; statistics: one workgroup), deterministic, no float atomics. Logits are
 * read inside the range of valid rows only and the teacher on valid rows only. A valid target outside the range gives NaN
 * in that row's logp, a teacher zero under kind 1 inf or NaN in that row's outputs: caller errors, never a stray access.
 * n % 8 == 0, vocab_first % 8 == 0, vocab_count % 8 == 0, the range inside [0, n), ld % 4 == 0, ld >= n, ldt % 4 == 0,
 * ldt >= vocab_count, else BL_E_SHAPE; a NULL pointer, kind outside {0, 1, 2}, beta outside (0, 1) with kind 2,
 * temperature <= 0 or sft_coef < 0 (NaN included) is BL_E_ARG; logits or teacher not 16-byte aligned is BL_E_ALIGN;
 * nothing is launched on a rejection. */
int bl_distill_loss_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                        int64_t ignore_index, const float* teacher, int64_t ldt, int32_t kind, float beta, float sft_coef,
                        float temperature, float* row_stats, float* stats, int32_t vocab_first, int32_t vocab_count,
                        void* stream);
/* dlogits (bf16) = d loss / d logits of bl_distill_loss_f32 from the logits, the teacher and what the forward saved (max z,
 * log sum and c in row_stats, n_valid in stats[1]; same kind, beta, sft_coef and temperature):
 *   kind 0: dD/dz_i = p_i c - q_i;   kinds 1, 2: dD/dz_i = p_i (u_i - c), u_i = logp_i - log q_i or (1 - beta)(logp_i - log mi_i);
 *   dlogits_i = (dD/dz_i + sft_coef (p_i - [i == target])) / (temperature * n_valid).
 * Writes the whole [rows, n] dlogits: exact +0 outside the range and on ignored rows. One launch, one workgroup per row;
 * a row's logits (inside the range) and teacher row are read once. Constraints and codes as the forward, and ldd % 8 == 0,
 * ldd >= n (BL_E_SHAPE), dlogits 16-byte aligned (BL_E_ALIGN). */
int bl_distill_loss_backward_f32(const float* logits, int64_t ld, int32_t rows, int32_t n, const int64_t* targets,
                                 int64_t ignore_index, const float* teacher, int64_t ldt, const float* row_stats,
                                 const float* stats, int32_t kind, float beta, float sft_coef, float temperature,
                                 bl_bf16* dlogits, int64_t ldd, int32_t vocab_first, int32_t vocab_count, void* stream);
/* The critic of the policy step (training/value_loss.py is the definition): a linear value head on the bf16 final-norm
 * rows hn [rows, dim] (leading dimension ld) and PPO's clipped value loss. The VALUE ROWS are found on the device from
 * `targets` (the convention of bl_cross_entropy_f32): level 0 (token) every valid row, level 1 (action) the first valid row
 * of each run of group_rows rows (group_rows is ignored at level 0). Per value row r, with w bf16 [dim] and b bf16 [1]:
 *   v = sum_k hn[r,k]*w[k] + b,  e = v - returns[r],  ec = old_values[r] + clamp(v - old_values[r], -clip, clip) - returns[r],
 *   l = max(e^2, ec^2) / 2,  dv = coef * (e^2 >= ec^2 ? e : 0) / n   (clip < 0: unclipped, old_values may be NULL).
 * returns / old_values fp32 [rows] and hn are read on value rows only. Outputs, every element written: index int32 [cap]
 * (cap = rows at level 0, rows / group_rows at level 1) = the value rows in ascending order, then -1; count int32 [1] = n;
 * value_rows fp32 [rows, 4] = (v, l, clipped 0/1, dv), zeros elsewhere; stats fp32 [8] = (mean l, n, clipped fraction,
 * mean v, mean return, explained variance, mean |e|, total) with total = policy_stats[0] + coef * mean l (policy_stats, the
 * stats of bl_policy_loss_f32, may be NULL: 0). n = 0 gives zeros. The dot product is one chain per lane over its 8-column
 * pieces in ascending k, then the wave's xor butterfly; the statistics are one workgroup in a fixed order. Four launches
 * on `stream`, deterministic, no host-side knowledge of the labels. dim % 8 == 0, ld % 8 == 0, ld >= dim, a level outside
 * {0, 1} or rows % group_rows != 0 at level 1: BL_E_SHAPE; hn, w, value_rows 16-byte aligned; a NULL pointer, coef < 0 or
 * clip >= 0 without old_values: BL_E_ARG; nothing is launched on a rejection. */
int bl_value_head_f32(const bl_bf16* hn, int64_t ld, int32_t rows, int32_t dim, const int64_t* targets, int64_t ignore_index,
                      int32_t group_rows, int32_t level, const bl_bf16* w, const bl_bf16* b, const float* returns,
                      const float* old_values, float coef, float clip, const float* policy_stats, int32_t* index,
                      int32_t* count, float* value_rows, float* stats, void* stream);
/* Its gradient from what it left (value_rows, index, count; same rows / group_rows / level): with dv_r = value_rows[r][3] *
 * inv_world, dw fp32 [dim] = sum_r dv_r * hn[r,:] (a thread owns its columns and walks the value rows in ascending order),
 * db fp32 [1] = sum_r dv_r, and dh[r,k] = bf16(float(dh[r,k]) + dv_r * w[k]) on the value rows only; dh NULL: the trunk gets no
 * gradient from the value loss (detach) and dw / db are the same bits. dw and db are overwritten. Constraints as the
 * forward; lddh % 8 == 0, lddh >= dim, dw and dh 16-byte aligned; inv_world <= 0 is BL_E_ARG. */
int bl_value_head_backward_f32(const bl_bf16* hn, int64_t ld, int32_t rows, int32_t dim, int32_t group_rows, int32_t level,
                               const bl_bf16* w, const float* value_rows, const int32_t* index, const int32_t* count,
                               float inv_world, float* dw, float* db, bl_bf16* dh, int64_t lddh, void* stream);
/* The critic at inference: V(s) of `rows` residual rows x [rows, dim] (leading dimension ldx), the final RMSNorm and the
 * head in one launch: out[r * out_stride] = sum_k hn[r,k]*w[k] + b with hn[r,:] the bf16 row bl_rmsnorm_bf16(x, norm_w, eps)
 * would write — bit for bit the v of bl_value_head_f32 over that row (the same lane ownership, the same sum of squares, the
 * same roundings, the same fmaf chain and butterfly); hn is never written. One wave per row; rows at or beyond `rows` and
 * columns in [dim, ldx) are not read; the one store per row is the fp32 at out[r * out_stride]. w, norm_w bf16 [dim], b bf16
 * [1], read when the kernel runs (a captured graph sees their current contents). A NULL pointer: BL_E_ARG; rows <= 0,
 * dim % 8 != 0, dim > 5120 or out_stride < 1: BL_E_SHAPE; x, norm_w or w not 16-byte aligned or ldx % 8 != 0: BL_E_ALIGN;
 * nothing is launched on a rejection. */
int bl_value_predict_f32(const bl_bf16* x, int64_t ldx, int32_t rows, int32_t dim, const bl_bf16* norm_w, float eps,
                         const bl_bf16* w, const bl_bf16* b, float* out, int64_t out_stride, void* stream);
/* LlamaRMSNorm backward: dx = rstd*(w*dy - xhat*mean(w*dy*xhat)) [+ dres: the residual stream's own gradient];
 * dw[j] = sum_rows dy*bf16(xhat). partial_ws >= ceil(rows/64)*dim floats. */
int bl_rmsnorm_backward_bf16(const bl_bf16* x, int64_t ldx, const bl_bf16* w, const bl_bf16* dy, int64_t lddy,
                             const bl_bf16* dres, int64_t lddres, bl_bf16* dx, int64_t lddx, float* dw, float* partial_ws,
                             int64_t partial_ws_floats, int32_t rows, int32_t dim, float eps, void* stream);
/* timm nn.LayerNorm backward (vision towers, stages vla-full-train / sandwich): as above with the mean removed;
 * db = column sums of dy. partial_ws needs >= 2 * ceil(rows / rpb) * dim floats for some rpb in {8, 16, ...}. */
int bl_layernorm_backward_bf16(const bl_bf16* x, int64_t ldx, const bl_bf16* w, const bl_bf16* dy, int64_t lddy,
                               const bl_bf16* dres, int64_t lddres, bl_bf16* dx, int64_t lddx, float* dw, float* db,
                               float* partial_ws, int64_t partial_ws_floats, int32_t rows, int32_t dim, float eps,
                               void* stream);
/* out[c] = sum_r a[r][c] (bias gradients). partial_ws >= ceil(rows/rpb)*cols floats for some rpb = 16, 32, 64, ...: the smallest
 * that fits is used (more room = more workgroups). */
int bl_colsum_bf16(const bl_bf16* a, int64_t lda, int32_t rows, int32_t cols, float* out, float* partial_ws,
                   int64_t partial_ws_floats, void* stream);
/* SwiGLU on an interleaved [rows, 2*inter] gate/up buffer (the training forward keeps it for the backward). */
int bl_swiglu_bf16(const bl_bf16* gu, int64_t ldg, bl_bf16* act, int64_t lda, int64_t rows, int32_t inter, void* stream);
int bl_swiglu_backward_bf16(const bl_bf16* gu, int64_t ldg, const bl_bf16* dact, int64_t ldd, bl_bf16* dgu, int64_t ldo,
                            int64_t rows, int32_t inter, void* stream);
/* exact-erf GELU and its derivative on [rows, cols] matrices with leading dimensions (projector: nn_utils.py:42-48;
 * timm Mlp). */
int bl_gelu_bf16(const bl_bf16* x, int64_t ldx, bl_bf16* y, int64_t ldy, int64_t rows, int32_t cols, void* stream);
int bl_gelu_backward_bf16(const bl_bf16* x, int64_t ldx, const bl_bf16* dy, int64_t lddy, bl_bf16* dx, int64_t lddx, int64_t rows,
                          int32_t cols, void* stream);
/* Transposed rotation on the q and k thirds of dqkv [B*S, 3*H*hd], in place. */
int bl_rope_backward_bf16(bl_bf16* dqkv, int64_t ld, int32_t B, int32_t S, int32_t H, int32_t hd, const bl_bf16* cos_tab,
                          const bl_bf16* sin_tab, int32_t pos0, void* stream);
/* out[c][r] = in[r][c], rows padded with zeros to rows_pad (the reduction dim of a wgrad GEMM must be a multiple of 64). */
int bl_transpose_pad_bf16(const bl_bf16* in, int64_t ldi, int32_t rows, int32_t cols, bl_bf16* out, int64_t ldo,
                          int32_t rows_pad, void* stream);
/* Same transpose written straight into the fragment-major packed layout of bl_pack_weight_bf16 for the [cols, rows_pad]
 * matrix (cols % 64 == 0, rows_pad % 32 == 0): the packed operand of a wgrad GEMM in one pass. */
int bl_transpose_pack_bf16(const bl_bf16* in, int64_t ld_in, int32_t rows, int32_t cols, bl_bf16* out_packed,
                           int32_t rows_pad, void* stream);
/* The two packers with a destination window: the source becomes k-blocks [kb_offset, kb_offset + K/32) of every n-tile
 * of a packed matrix that has kt_total k-blocks per n-tile — the adapter columns of a K-concatenated LoRA weight
 * [W | s·B] / [Wᵀ | Aᵀ] (training/step.py), refreshed after every optimizer step without touching the frozen part. */
int bl_pack_weight_into_bf16(const bl_bf16* w, int64_t ldw, int64_t N, int64_t K, bl_bf16* out, int64_t kt_total,
                             int64_t kb_offset, void* stream);
int bl_transpose_pack_into_bf16(const bl_bf16* in, int64_t ld_in, int32_t rows, int32_t cols, bl_bf16* out_packed,
                                int32_t rows_pad, int64_t kt_total, int64_t kb_offset, void* stream);
/* ONE launch for a table of independent small ops — copies, (scaled) packs, (scaled) transposing packs: the re-pack plan of a
 * training step (every LoRA adapter's five refresh launches, the optimizer's write-backs). ops_table: device array of
 *   struct { int32 kind, nblocks, rows, cols, rows_pad, bx_count; int64 ld, kt_total, kb_off, n; const void* src; void* dst;
 *            float scale; int32 pad; }        (kind 0: copy n bytes; 1: pack rows x cols into k-blocks [kb_off, ...) of a packed
 *   matrix with kt_total k-blocks per 16-row tile; 2: transposing pack of [rows, cols], rows padded to rows_pad; scale != 1:
 *   bf16(scale * x) first), block_start: device int32 [n_ops] prefix sums of nblocks. Same device code, same results, as
 * bl_copy_bytes / bl_pack_weight_into_bf16 / bl_transpose_pack_into_bf16 (+ bl_scale_bf16). */
int bl_batched_ops(const void* ops_table, const int32_t* block_start, int32_t n_ops, int32_t total_blocks, void* stream);
/* LoRA dropout (PEFT: base(x) + lora_B(lora_A(dropout(x))) * scaling; vla-scripts/finetune.py:101,177 `lora_dropout`).
 * bl_dropout_bf16: out = bf16(x / (1 - p)) where kept, 0 elsewhere; element (row, col) is kept iff the top 24 bits of
 * mix32((row * cols + col) ^ mix32(mix32(*seed) + salt)) >= p * 2^24 (seed on the DEVICE: a replayed plan draws a new mask when the
 * host bumps it; salt = the adapted linear). bl_dropout_grad_fix_bf16: turns the fused input gradient dx = dy.W + u (u = dt.A,
 * un-masked) into dy.W + mask/(1-p) * u with the same mask: dx += (1/(1-p) - 1) * u where kept, dx -= u where dropped. */
int bl_dropout_bf16(const bl_bf16* x, int64_t ldx, int32_t rows, int32_t cols, float p, const uint32_t* seed, uint32_t salt,
                    bl_bf16* out, int64_t ldo, void* stream);
int bl_dropout_grad_fix_bf16(const bl_bf16* u, int64_t ldu, int32_t rows, int32_t cols, float p, const uint32_t* seed, uint32_t salt,
                             bl_bf16* dx, int64_t lddx, void* stream);
/* Global gradient norm (fsdp.py:268-270): per-tensor partial sums of squares, then norm and clip coefficient
 * out_norm_coef = {||g||, min(1, max_norm / (||g|| + 1e-6))} (torch.nn.utils.clip_grad_norm_). */
int bl_sumsq_partial_f32(const float* g, int64_t n, float* partial, int32_t nblocks, void* stream);
int bl_clip_coef_f32(const float* partial, int32_t n, float max_norm, float* out_norm_coef, void* stream);
/* torch.optim.AdamW step `step` (1-based) on fp32 master weights; g is scaled by norm_coef[1] when given; p_bf16
 * (optional) receives the bf16 copy of the updated weights. */
int bl_adamw_f32(float* p, float* m, float* v, const float* g, const float* norm_coef, int64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int32_t step, bl_bf16* p_bf16, void* stream);
/* timm LayerScale (patched to `scale_factor`, modeling_prismatic.py:52-59) around a residual branch, training form:
 * y = bf16(bf16(u * scale) + res) with the branch output u kept; backward du = dy * scale, dscale = sum_rows dy * u
 * (partial_ws >= ceil(rows / 64) * cols floats). */
int bl_scale_residual_bf16(const bl_bf16* u, int64_t ldu, const bl_bf16* scale, const bl_bf16* res, int64_t ldres, bl_bf16* y,
                           int64_t ldy, int64_t rows, int32_t cols, void* stream);
int bl_layerscale_backward_bf16(const bl_bf16* dy, int64_t lddy, const bl_bf16* u, int64_t ldu, const bl_bf16* scale,
                                bl_bf16* du, int64_t lddu, float* dscale, float* partial_ws, int64_t partial_ws_floats,
                                int32_t rows, int32_t cols, void* stream);
/* Small-output TN GEMM for the LoRA adapter gradients (dA = dt^T x, dB = (ts^T dy)^T; finetune.py:174-189 → PEFT's
 * autograd): C = P^T Q with P [T, R] (R = 64, 128 or 192), Q [T, N] (N % 64 == 0), both row-major bf16, reduction over
 * the T rows, fp32 output scaled by alpha — C [R, N] (transpose_out = 0) or C [N, R] (transpose_out = 1), dense (ldc = N or R). Reads Q
 * once, untransposed. partial_ws (optional, fp32) lets small-N calls split T across workgroups deterministically. */
int bl_gemm_tn_small_bf16(const bl_bf16* P, int64_t ldp, const bl_bf16* Q, int64_t ldq, int32_t T, int32_t R, int32_t N,
                          float* C, int64_t ldc, int32_t transpose_out, float alpha, float* partial_ws, int64_t partial_ws_floats,
                          void* stream);
/* LoRA (vla-scripts/finetune.py:174-189): out = bf16(s * x) for the small rank-space tensors; gradient mask that keeps
 * the off-block entries of a fused adapter's B [n_rows, members * rp] at zero (row n belongs to member n / (n_rows /
 * members), or n % members when the members' rows are interleaved). */
int bl_scale_bf16(const bl_bf16* x, float s, bl_bf16* out, int64_t n, void* stream);
int bl_lora_block_mask_f32(float* g, int32_t n_rows, int32_t R, int32_t rp, int32_t members, int32_t interleave, void* stream);
/* LoRA deployment by merging (vla-scripts/finetune.py:331-341, PEFT `merge_and_unload()`), on the device and on the packed
 * layout: out[n, k] = bf16(W[n, k] + sum_r bf16(scale * B[n, r]) * A[r, k]), w_packed and out_packed both fragment-major
 * [n/16, k/32, 64, 8] (bl_pack_weight_bf16), A [R, k] and B [n, R] row-major bf16 with R = members * rp (the fused members'
 * adapters side by side, B block structured: row n of B only sees member(n)'s rp columns, member(n) = n / (n / members), or
 * n % members with interleave != 0). The update is accumulated in fp32 over R on the MFMA, added to W in fp32 and rounded
 * once; an element whose update is exactly zero keeps its bits, so B = 0 or scale = 0 copies W bit for bit. Stacked members
 * that own whole 16-row tiles read only their own rp columns of B / rows of A (the rest are zeros by construction).
 * n % 16 == 0, k % 32 == 0, R % 32 == 0, rp % 32 == 0, the rank span of one row (rp for such stacked members, else R) <= 128, 16-byte aligned pointers, and
 * out_packed must not overlap w_packed (BL_E_ARG). No atomics, no workspace; definition: training/lora.py::merged_reference. */
int bl_lora_merge_bf16(const bl_bf16* w_packed, const bl_bf16* A, const bl_bf16* B, float scale, bl_bf16* out_packed, int64_t n,
                       int64_t k, int32_t R, int32_t rp, int32_t members, int32_t interleave, void* stream);
/* ONE launch for a device table of the above — every adapted group of a model after an optimizer step. table: device array of
 *   struct { const bl_bf16 *w, *A, *B; bl_bf16* out; float scale; int32 n, k, R, rp, members, interleave, n_items;
 *            int64 first_item; }
 * n_items = ceil(k / 128) * m * ceil(n / 16 / m / 16) work items of the group (m = members when they are stacked and
 * n % (16 * members) == 0, else 1), first_item = prefix sum of n_items. The entries are NOT validated (the table is on the
 * device): build them with train_ops.lora_merge_batched, which checks what bl_lora_merge_bf16 checks. Same device code and
 * summation order as bl_lora_merge_bf16: bit-identical results. */
int bl_lora_merge_batched_bf16(const void* table, int32_t n_groups, void* stream);
/* Packed bf16 GEMM weight → the W8 operand of bl_gemm_fp8 and its per-channel scales, on the device (csrc/
 * quantize_weight_fp8.hip): w_packed fragment-major [n/16, k/32, 64, 8] (bl_pack_weight_bf16, bl_lora_merge_bf16), w8_packed the
 * n·k bytes of [n/16, k/64, 64 lanes, 16 B], scale fp32 [n]. Per output channel, the quantiser specification of
 * bl_quantize_rows_fp8: amax = max |w|; scale = amax / 448 and inv = 448 / amax when amax >= 2^-100, else scale = inv = 1;
 * code = e4m3_rne_sat(fl32(w * inv)). e4m3 lane L of fragment (nt, ks8) = row 16·nt + (L & 15), columns 64·ks8 + 16·(L >> 4) + 0…15
 * = the 16 bytes of bf16 fragment (nt, 2·ks8 + (L >> 5)), lane (L & 15) + 32·((L >> 4) & 1), then those of the lane 16 above.
 * n % 16 == 0, k % 128 == 0 (bl_gemm_fp8's limit), 16-byte aligned pointers, no buffer overlapping another (BL_E_ARG). Every
 * output byte is written whatever the buffers held; no atomics, no workspace. */
int bl_quantize_weight_fp8_packed(const bl_bf16* w_packed, int64_t n, int64_t k, void* w8_packed, float* scale, void* stream);
/* ONE launch for a device table of the above — every e4m3 copy of a model's adapted weights after a refresh. table: device array of
 *   struct { const bl_bf16* w; void* w8; float* scale; int32 n, k, n_items, pad; int64 first_item; }
 * n_items = n / 16 (one work item per 16-row tile), first_item = prefix sum of n_items. The entries are NOT validated (the
 * table is on the device): build them with train_ops.quantize_packed_batched, which checks what the single call checks.
 * Same device code as bl_quantize_weight_fp8_packed: bit-identical results. */
int bl_quantize_weight_fp8_packed_batched(const void* table, int32_t n_entries, void* stream);
/* y += a * x on flat fp32 buffers: gradient accumulation over micro-batches with the loss normalised by the number of
 * accumulation steps (vla-scripts/finetune.py:256-262, 307-310). */
int bl_axpy_f32(float* y, const float* x, float a, int64_t n, void* stream);
/* fp32 <-> bf16 casts of flat buffers: the bf16 wire format of the gradient reduce-scatter (fsdp.py:139-147,
 * `reduce_in_full_precision=False`); round-to-nearest-even. 16-byte aligned pointers. */
int bl_cast_f32_bf16(const float* src, bl_bf16* dst, int64_t n, void* stream);
int bl_cast_bf16_f32(const bl_bf16* src, float* dst, int64_t n, void* stream);
/* Device memset / device-to-device copy on `stream` (replayable steps of the training plans). */
int bl_memset_zero(void* dst, int64_t bytes, void* stream);
int bl_copy_bytes(void* dst, const void* src, int64_t bytes, void* stream);
/* Row gather (scatter = 0: dst[r] = src[map(r)]) or scatter (dst[map(r)] = src[r]) with
 * map(r) = (r / group) * stride + offset + r % group — the 256 projected patch rows inside the [B, S, D] embedding
 * buffer (modeling_prismatic.py:343-351) for the projector's backward. */
int bl_map_rows_bf16(const bl_bf16* src, int64_t ld_src, bl_bf16* dst, int64_t ld_dst, int64_t rows, int32_t cols,
                     int32_t group, int32_t stride, int32_t offset, int32_t scatter, void* stream);
/* dW_embed[ids[b,j]] += dx[b, row(j)] over the text positions of the multimodal splice (fp32 atomics; dw pre-zeroed). */
int bl_embed_backward_bf16(const int64_t* ids, int32_t B, int32_t L, const bl_bf16* dx, int32_t dim, int32_t n_patches,
                           float* dw, void* stream);

/* ---- vision glue ------------------------------------------------------------------------------------------- */
/* Frames already at the model resolution: uint8 [B, H, W, 3] → pixel_values [B, 6, H, W] bf16 = to_tensor + the two
 * normalisations of PrismaticImageProcessor.apply_transform (processing_prismatic.py:128-145; DINOv2 ImageNet mean/std,
 * SigLIP 0.5/0.5) in its fp32 operation order, channel-stacked, rounded to bf16 as the call sites do
 * (`.to(torch.bfloat16)`). mean_std: 12 device floats = mean[6] | std[6]. H*W % 8 == 0. (Resize first: bl_resample_pass_u8.) */
int bl_preprocess_u8_bf16(const uint8_t* frames, int32_t B, int32_t height, int32_t width, const float* mean_std, bl_bf16* out,
                          void* stream);
/* One pass of the PIL resize behind `TVF.resize(img, size, BICUBIC)` (processing_prismatic.py:133; Pillow
 * libImaging/Resample.c, 8 bits per channel): out = clip8((2^21 + Σ_k src[first + k]·coef[k]) >> 22) with the host's
 * 22-bit fixed-point coefficient table coefs [out_len, ksize] and bounds [out_len, 2] = (first, count).
 * horizontal != 0: src [B, lines, in_len, 3] → dst [B, lines, out_len, 3]; else src [B, in_len, lines, 3] →
 * dst [B, out_len, lines, 3]. uint8 RGB, packed. Bit-exact against Pillow (tests/test_ops_gpu.py). */
int bl_resample_pass_u8(const uint8_t* src, uint8_t* dst, int32_t B, int32_t lines, int32_t in_len, int32_t out_len,
                        int32_t horizontal, const int32_t* bounds, const int32_t* coefs, int32_t ksize, void* stream);
/* The eval-time centre crop of the robot loops, `get_vla_action(center_crop=True)` (experiments/robot/openvla_utils.py:
 * 81-155: tf.image.convert_image_dtype → tf.image.crop_and_resize(bilinear, one box) → clip → convert back, saturating):
 * uint8 frames src [B, H, W, 3] → dst [B, out_h, out_w, 3]. Output pixel (i, j) samples ys = y_base + i·y_step,
 * xs = x_base + j·x_step (fp32 constants computed by the host: y1·(H−1) and (y2−y1)·(H−1)/(out_h−1) for the normalised
 * box), bilinear on u8/255, 0 outside the image, then uint8(clamp(clamp(v,0,1)·255.5, 0, 255)). Bit-identical to the host
 * restatement bridgelang_amd/vla/eval_preprocess.py (TensorFlow itself is absent: unpinned against TF). */
int bl_crop_resize_bilinear_u8(const uint8_t* src, uint8_t* dst, int32_t B, int32_t H, int32_t W, int32_t out_h, int32_t out_w,
                               float y_base, float y_step, float x_base, float x_step, void* stream);
/* OpenVLA's training-time image augmentation (`image_aug`, prismatic/vla/datasets/datasets.py:121-136 → dlimp
 * augment_image) on uint8 frames src [B, H, W, 3] (H, W >= 2), output at the input size: u8/255 → random_resized_crop
 * (tf.image.crop_and_resize, bilinear, box (y1, x1, y1 + side_y, x1 + side_x)) → + brightness δ → contrast
 * (x − mean_c)·f + mean_c about the per-image channel means → saturation (RGB → HSV, S·f, → RGB) → hue (h + δ mod 1), each
 * followed by clip [0, 1], then the saturating uint8 convert (× 255.5, truncate). params [B, 8] device fp32 rows =
 * (y1, x1, side_y, side_x, brightness δ, contrast f, saturation f, hue δ): the host draws them, the op is a pure function
 * of (src, params). Two passes: the first accumulates mean_c as Σ rint(x·2^24) into workspace [B, 3] int64 (zeroed on
 * the stream inside the call: the op is replayable), the second recomputes the sample and writes dst [B, H, W, 3] uint8
 * and / or, fused (H*W % 8 == 0), pixel_values [B, 6, H, W] bf16 = bl_preprocess_u8_bf16 of that uint8 output with
 * mean_std as there (either output may be NULL, not both). Bit-identical to the host restatement
 * bridgelang_amd/vla/image_augment.py::augment_frame (TensorFlow and dlimp are absent: unpinned against them). */
int bl_augment_frames_u8(const uint8_t* src, int32_t B, int32_t H, int32_t W, const float* params, int64_t* workspace,
                         uint8_t* dst, bl_bf16* pixel_values, const float* mean_std, void* stream);
/* pixel_values [B, 6, 224, 224] bf16 (processing_prismatic.py:128-145 layout) → 14x14 patch rows for one tower:
 * out[b*256 + py*16 + px, c*196 + i*14 + j] = pixel_values[b, chan0 + c, py*14 + i, px*14 + j]; columns 588..ld-1
 * are zeroed (K padded to a multiple of 64 for the patch-embed GEMM; timm PatchEmbed conv flattening order). */
int bl_im2col_patch14_bf16(const bl_bf16* pixel_values, int32_t B, int32_t chan0, bl_bf16* out, int64_t ld,
                           void* stream);
/* Broadcast `n_prefix` learned prefix tokens (cls + registers) into rows [b*T, b*T + n_prefix) of x [B*T, dim]. */
int bl_write_prefix_tokens_bf16(const bl_bf16* prefix, int32_t n_prefix, int32_t dim, bl_bf16* x, int32_t B,
                                int32_t T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BRIDGELANG_HIP_H */
