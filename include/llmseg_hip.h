/* libllmseg_hip.so -- C ABI of the MI355X (gfx950) kernels behind LLM-Seg's `model_forward` hot path.
 *
 * The reference (wangjunchi/LLMSeg) has no FFI boundary: its path is PyTorch eager ops
 * (SURVEY.md §8b).  Each entry point below replaces the eager op sequence cited next to it
 * (paths relative to the reference tree).  All pointers are DEVICE pointers owned by the caller
 * (PyTorch's caching allocator); kernels never allocate, never synchronise, and launch on the
 * `stream` argument (a hipStream_t passed as void*).  bf16 tensors are raw uint16 storage.
 * Every function returns 0 on success or a negative LLMSEG_E* code; llmseg_last_error() gives text.
 * Rows of every bf16 matrix must be 16-byte aligned (pointer and leading dimension % 8 == 0)
 * unless stated otherwise.
 */
#ifndef LLMSEG_HIP_H
#define LLMSEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLMSEG_OK 0
#define LLMSEG_EINVAL (-1)
#define LLMSEG_ELAUNCH (-2)
#define LLMSEG_NOT_TAKEN 1 /* llmseg_linear_bwd: the shape is not covered, nothing was launched or written; the caller runs the separate kernels */

/* epilogue activation */
enum { LLMSEG_ACT_NONE = 0, LLMSEG_ACT_RELU = 1, LLMSEG_ACT_GELU = 2, LLMSEG_ACT_QUICKGELU = 3, LLMSEG_ACT_SILU = 4,
       LLMSEG_ACT_SIGMOID = 5 };

/* ABI guard.  Every argument struct starts with `struct_size`: the caller writes sizeof() of the struct AS ITS OWN BINDING DECLARES IT;
 * an entry point whose struct does not have exactly that size returns LLMSEG_EINVAL ("ABI mismatch") before reading any other field,
 * so a binding written against an older header (fields were appended in every round) fails loudly instead of having the library read
 * past the caller's struct.  llmseg_struct_size(which) returns the library's sizeof (0 = llmseg_gemm_args, 1 = llmseg_attn_args,
 * 2 = llmseg_attn_bwd_args, 3 = llmseg_dropout, 4 = llmseg_gemm_w8_args, 5 = llmseg_lora_down_args; -1 for an unknown index) so a binding can assert at load time;
 * llmseg_version() is bumped whenever a struct or a signature changes (22: llmseg_decode_attn_chunk, llmseg_lookup_draft, llmseg_lookup_accept; 21: llmseg_kv_quantize_mxfp8, llmseg_decode_attn_mxfp8; 20: llmseg_logits_process; 19: llmseg_quantize_rows_mxfp4, llmseg_gemm_mxfp4 and llmseg_gemm_mxfp4_args; 18: llmseg_decode_attn_beams, llmseg_beam_step; 17: llmseg_lora_down takes llmseg_lora_down_args and replaces llmseg_lora_down_ws / _parts / _pack; 16: llmseg_sample_tokens; 15: llmseg_sam_dense_prompt, llmseg_sam_prompt_tokens; 14: llmseg_decode_attn_rows; 13: llmseg_quantize_rows_i8, llmseg_gemm_w8 and llmseg_gemm_w8_args; 12: llmseg_rle_encode, llmseg_rle_parse and their workspace queries; 11: llmseg_image_resize_u8_filter, llmseg_clip_preprocess, llmseg_mask_union; 10: llmseg_linear_bwd; 9: llmseg_attn_args.win_grid / win_nw / pad_q / pad_k / pad_v; 7: the fp32-activation head entry points; 4: the reduction entry points take a workspace; 5 = this header:
 * llmseg_dropout.seg_rows; 6: llmseg_gemm_args.norm_w / norm_eps / norm_out / ldn). */
#define LLMSEG_ABI_VERSION 22

/* Determinism (round 4).  No kernel adds floating-point numbers with atomics: every sum whose terms come from several workgroups is
 * written as per-workgroup partials into CALLER-OWNED scratch (`workspace`, `workspace_bytes`; any device memory, 256-byte aligned, not
 * shared with a concurrently running stream) and folded in a fixed order by a second launch, so the same inputs give the same bits on
 * every run (the reference's resume contract, training.py:404-421,460-477).  LLMSEG_REDUCE_WS_BYTES is enough for every call the model
 * makes; entry points that can fall back to a single partial (llmseg_colsum, llmseg_norm_bwd* for rows <= 8 KiB, llmseg_lora_outer)
 * accept NULL / a smaller buffer and stay deterministic (slower), the others return LLMSEG_EINVAL when it is too small. */
#define LLMSEG_REDUCE_WS_BYTES (16 << 20)
int llmseg_version(void);
/* kernel launches issued by this library since it was loaded (all streams; a captured hipGraph counts at capture, not at replay):
 * a benchmark reads the difference across one eager micro-step to report launches per step */
int64_t llmseg_launch_count(void);
int64_t llmseg_struct_size(int which);
const char* llmseg_last_error(void);

/* ---- GEMM ------------------------------------------------------------------------------------
 * C[b][m][n] = epi( alpha * sum_k A[b][m][k] * W[b][n][k] ),  A,W bf16 (K contiguous), fp32 accumulate on MFMA.
 * epi(v) = residual[m][n] + gamma[n] * act(v + bias[n])   (each term optional, NULL = absent).
 * Replaces every nn.Linear / 1x1 conv / patch-embed conv on the path: HF LlamaAttention/LlamaMLP projections and
 * lm_head (model/llava/model/language_model/llava_llama.py:93-105), SAM qkv/proj/mlp
 * (model/segment_anything/modeling/image_encoder.py:238-258, common.py:25-26), neck convs (:92-108),
 * mm_projector (model/llava/model/llava_arch.py:93-96), text_hidden_fcs / lisa_* heads (model/LISA.py:54-121).
 * out_f32 != 0 writes fp32 C (ldc in elements of the output type).  batch/strides (in elements) give a strided-batched GEMM.
 */
typedef struct {
  uint32_t struct_size;  /* = sizeof(llmseg_gemm_args) of the caller's declaration (ABI guard, see above) */
  uint32_t reserved0;    /* 0 */
  const void* A; const void* W; void* C;
  const void* bias;      /* bf16 [N] or NULL */
  const void* gamma;     /* bf16 [N] or NULL (DINOv2 LayerScale) */
  const void* residual;  /* bf16 [M][ldr] or NULL */
  int64_t M, N, K;
  int64_t lda, ldw, ldc, ldr;
  int64_t batch, strideA, strideW, strideC;
  float alpha;
  int act;
  int out_f32;
  int trans_a;   /* 1: A is stored [K][M] (M contiguous, lda >= M) -- used by the backward pass (dW = dY^T X) */
  int trans_w;   /* 1: W is stored [K][N] (N contiguous, ldw >= N) -- used by the backward pass (dX = dY W) */
  int64_t batch2, strideA2, strideW2, strideC2;   /* optional outer batch dimension (0/1 = none): entry (b1, b2) is at b1*stride + b2*stride2 */
  /* optional 64-wide extension of the contraction: C = epi(alpha * (A.W^T + A2.W2^T)), A2 bf16 [M][64] (lda2), W2 bf16 [N][64]
   * (ldw2); NULL = none.  Fuses low-rank updates (the r = 8 LoRA products of q_proj / v_proj, zero-padded to 64 columns) into the
   * big GEMM as one more K-tile instead of a read-modify-write pass over C.  batch == 1, no trans_*. */
  const void* A2; const void* W2; int64_t lda2, ldw2;
  /* optional caller-owned scratch (fp32 partial tiles of the split-K path: short matrices with a long contraction, e.g. the
   * Llama o / down projections and every dX GEMM at M = 2 x 319 rows, run as S K-slices + one reduce launch); NULL / too small =
   * no split-K.  Must not be shared between streams that run concurrently. */
  void* workspace; int64_t workspace_bytes;
  /* out_f32 only: C += result instead of C = result (weight gradients accumulate over micro-steps in an fp32 arena, as the
   * reference's DeepSpeed engine accumulates them: training.py:79-82 gradient_accumulation_steps, :292-332 bf16 config) */
  int accumulate;
  /* decode-step fusions, M <= 8 only (one token per sequence: every kernel launch saved is ~8 us of a ~100 us layer):
   *   a_norm_w (bf16 [K]) : A := RMSNorm(A) * a_norm_w on load (HF LlamaRMSNorm arithmetic, eps = a_norm_eps);
   *   a_swiglu            : A rows are [gate | up] of width 2K (lda >= 2K), A := silu(gate) * up on load (HF LlamaMLP).
   * Same bits as llmseg_norm / llmseg_swiglu followed by the GEMM. */
  const void* a_norm_w; float a_norm_eps; int a_swiglu;
  /* optional second output (ABI 6): norm_out[m][:] = RMSNorm(C[m][:]) * norm_w, bf16 [M][ldn], with exactly the arithmetic of llmseg_norm(rms = 1) applied to
   * the bf16 C this call writes (HF LlamaRMSNorm: fp32 statistics, rounding before the weight multiply) -- the residual stream's next pre-norm
   * (llava_llama.py:93-102: o_proj / down_proj + residual, then the following LlamaRMSNorm).  bf16 output, batch 1, N % 8 == 0, ldn % 8 == 0.  When the product runs
   * as K-slices (Llama o / down at M = 2 x 319) the reduce launch computes it on the row it has just summed (one launch and one pass over the row instead of
   * two); otherwise the library runs llmseg_norm behind the GEMM.  Same bits either way.  NULL = off. */
  const void* norm_w; float norm_eps; int reserved1; void* norm_out; int64_t ldn;
  /* fused Llama-layer epilogues (ABI 8): the pointwise launch that used to follow the product runs inside the GEMM's store.  Plain bf16 product only
   * (batch 1, alpha 1, no bias / activation / gamma / residual / norm_out / trans_*).  Same bits as the product followed by that launch: the library runs
   * exactly that two-launch route on every shape its fused kernel (the 128 x 256 tile in one K-slice: the Llama layer at 2 x 319 rows) does not take.
   *   LLMSEG_FX_ROPE        C = q|k|v [M][N]: the heads (width 128) of columns < fx_cols are rotated (rotate-half; fx_cos / fx_sin fp32 [fx_T][64], position
   *                         = row % fx_T) as llmseg_rope(C, ...) would after the product (HF LlamaAttention: apply_rotary_pos_emb on q and k,
   *                         call site llava_llama.py:93-102);
   *   LLMSEG_FX_SWIGLU      N = 2 I, C = gate|up [M][2 I] as without fx AND fx_out[m][c] = silu(gate[m][c]) * up[m][c], bf16 [M][fx_ld] (HF LlamaMLP), as
   *                         llmseg_swiglu would after the product;
   *   LLMSEG_FX_SWIGLU_BWD  N = I: the product is d(silu(gate) * up) [M][I] (dX of down_proj); fx_in = the saved gate|up [M][fx_ld >= 2 I]; C = d(gate|up)
   *                         bf16 [M][ldc >= 2 I], as llmseg_swiglu_bwd would compute from the stored product. */
  int fx; int fx_T; int64_t fx_cols; const float* fx_cos; const float* fx_sin; void* fx_out; const void* fx_in; int64_t fx_ld;
  /* norm-backward tail (ABI 8): the product is the gradient dy [M][N] of a pre-norm's OUTPUT (dX of q|k|v or of gate|up: HF LlamaDecoderLayer,
   * hidden = residual + sublayer(norm(hidden))), and what the caller wants is the gradient of the norm's INPUT:
   *   C = norm_backward(dy, nb_x, nb_w; nb_eps, nb_rms) + nb_dres          (llmseg_norm_bwd_add: frozen norm weight, nb_dres = the residual branch's gradient or NULL)
   * with, optionally, the LoRA branches' dX added to dy first (llmseg_lora_apply with w_rn = 1: dy += nb_lora_alpha * mask_b * (nb_lora_t[:, 8 b ..] . nb_lora_w_b),
   * nb_lora_t bf16 [M][nb_lora_ldt >= 16], nb_lora_w0 / nb_lora_w1 bf16 [8][N] (w1 NULL = one branch), nb_lora_drop = llmseg_dropout* or NULL).  A K-sliced product
   * (the Llama dX products at 2 x 319 rows) does all of it in its reduce launch -- one pass over the gradient instead of three launches; otherwise the library
   * runs the product into the tail of `workspace` (>= M N 2 bytes, required) followed by llmseg_lora_apply / llmseg_norm_bwd_add.  Same bits either way.
   * Plain bf16 product, ldc == N, N % 8 == 0.  nb_x NULL = off. */
  const void* nb_x; const void* nb_w; const void* nb_dres; float nb_eps; int nb_rms;
  const void* nb_lora_t; int64_t nb_lora_ldt; const void* nb_lora_w0; const void* nb_lora_w1; float nb_lora_alpha; int reserved2; const void* nb_lora_drop;
  /* delta tail (ABI 8): the product is dO [batch * dl_T][dl_heads * 128] of an attention (dX of o_proj; rows = b * dl_T + q) whose output was dl_o (bf16, row pitch
   * dl_ldo); the call also writes dl_out[b][h][q] = sum_d dO * O (fp32 [batch][dl_heads][dl_T]) -- llmseg_attn_bwd's `delta`, which can then be passed with
   * delta_ready = 1.  In the reduce launch of a K-sliced product, by the attention backward's delta kernel behind the product otherwise; same bits.  NULL = off. */
  const void* dl_o; int64_t dl_ldo; float* dl_out; int32_t dl_heads; int32_t dl_T;
  /* with nb_lora_t (ABI 8): the LoRA operand still as the K-slice partials llmseg_lora_down left on request (llmseg_lora_down_args.parts_S;fp32 [nb_lora_S][M][16]); the tail adds them in order, scales by
   * nb_lora_scale, rounds to bf16 (llmseg_lora_down's finish arithmetic), uses the result AND stores it to nb_lora_t[:, 0:16] (+ nb_lora_zero zero columns) for
   * llmseg_lora_wgrads: the finish launch of the backward's rank-8 down projection rides in the reduce launch.  NULL = nb_lora_t is an input. */
  const float* nb_lora_part; int32_t nb_lora_S; float nb_lora_scale; int32_t nb_lora_zero; int32_t reserved3;
} llmseg_gemm_args;
enum { LLMSEG_FX_NONE = 0, LLMSEG_FX_ROPE = 1, LLMSEG_FX_SWIGLU = 2, LLMSEG_FX_SWIGLU_BWD = 3 };
int llmseg_gemm_bf16(const llmseg_gemm_args* args, void* stream);
/* tuning knob (results are identical up to fp32 summation order of split-K; only speed differs):
 * bits 0-3: GEMM kernel for K % 64 == 0 shapes: 0 = register staging 128x128, 2 = LDS-DMA 128x128, 8 = LDS-DMA 256x256 ping-pong,
 *           9 = LDS-DMA 128x256 ping-pong, 10 = LDS-DMA 160x256 ping-pong (K-sliced only: needs a slice count >= 2 in bits 8-12, the call fails
 *           otherwise), 5 = auto [default: a cost model picks kernel and split count]; any other value = 5;
 * bits 4-7: XCD skew + 1 (0 = keep); bits 8-12: forced split-K slice count for variants 8 / 9 / 10 (0 = 1 slice);
 * nothing sits above bit 12: higher bits are ignored. */
int llmseg_gemm_set_variant(int variant);

/* ---- int8 weight-only decode (per-row scales) ------------------------------------------------
 * The decode step of generation streams every decoder weight once per token (HBM-bound): int8 rows with one fp32 scale each halve
 * the stream.  The reference offers 8-bit weights through bitsandbytes (its `--load_in_8bit` flag); this is NOT that arithmetic
 * but the plain symmetric per-row quantiser below, stated exactly so that a caller can reproduce it bit for bit.
 *
 * llmseg_quantize_rows_i8: per row n of w [N][ldw] bf16 (finite values):
 *   amax = max_k |w|;  scale[n] = amax / 127.0f;  inv = 127.0f / amax, 0 when amax == 0 (both divisions IEEE fp32);
 *   q[n][k] = clamp(rintf((float)w * inv), -127, 127) (the product rounded once, ties to even), int8 two's complement [N][ldq];
 *   w_hat[n][k] = bf16_rne((float)q * scale[n]), bf16 [N][ldh], written in the same pass when w_hat != NULL (the dequantised operand
 *   of the prefill costs no extra read of w).
 * K % 16 == 0, ldw % 8 == 0, ldh % 8 == 0, ldq % 16 == 0, every pointer 16-byte aligned.  One launch. */
int llmseg_quantize_rows_i8(const void* w, int64_t ldw, int64_t N, int64_t K, void* q, int64_t ldq, float* scale, void* w_hat /* nullable */,
                            int64_t ldh, void* stream);
/* llmseg_gemm_w8: C[m][n] = residual[m][n] + scale[n] * sum_k A[m][k] * q[n][k], 1 <= M <= 8 (one token per sequence).
 * A bf16 [M][lda], q int8 [N][ldq], fp32 FMA accumulation (a * q is exact in fp32), the scale applied once to the finished sum;
 * C bf16 or fp32 (out_f32; ldc in elements of the output type).  K % 16 == 0, lda % 8 == 0, ldq % 16 == 0, A and q 16-byte aligned.
 * A weight stream without MFMA, LDS staging or atomics: same inputs, same bits.  One launch. */
typedef struct {
  uint32_t struct_size;  /* = sizeof(llmseg_gemm_w8_args) of the caller's declaration (ABI guard, see above) */
  uint32_t reserved0;    /* 0 */
  const void* A; const void* Q; const float* scale;
  const void* residual;  /* bf16 [M][ldr] or NULL */
  void* C;
  int64_t M, N, K;
  int64_t lda, ldq, ldc, ldr;
  int32_t out_f32; int32_t reserved1;
} llmseg_gemm_w8_args;
int llmseg_gemm_w8(const llmseg_gemm_w8_args* args, void* stream);

/* ---- MXFP4 weight-only decode (OCP Microscaling: 4-bit E2M1 elements, one E8M0 scale per block of 32) ------------------------------
 * 4.25 bits per weight: a quarter of the bf16 stream.  The dequantised weight w_hat = element * 2^e has one mantissa bit, so it is
 * exact in bf16 and a * w_hat is exact in fp32: the model the decode steps run is exactly the one whose matrices are w_hat.  The
 * stored bytes are the operand layout of the block-scaled MFMA forms (v_mfma_scale_f32_*_f8f6f4).
 *
 * llmseg_quantize_rows_mxfp4: per row n of w [N][ldw] bf16 (finite values) and per block b of 32 consecutive columns (K % 32 == 0):
 *   amax = the largest |w| of the block;
 *   e = the smallest integer >= -127 with amax <= 6 * 2^e (amax == 0: e = -127); scale[n][b] = e + 127, one E8M0 byte.  A finite
 *     bf16 never needs e > 126: nothing saturates.  For a normal amax = m * 2^E, m in [1, 2): e = E - 2 when m <= 1.5, else E - 1
 *     (integer work on the bf16 bits, no division and no logarithm);
 *   x = w / 2^e (exact); |x| is rounded to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} = magnitude codes 0 .. 7, a tie going to the
 *     EVEN code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4;
 *   the 4-bit code is sign << 3 | magnitude, the sign cleared when the magnitude code is 0 (-0 is never stored);
 *   byte j of packed row n holds element 2 j in its LOW nibble and element 2 j + 1 in its HIGH nibble: packed uint8 [N][ldq];
 *   w_hat[n][k] = bf16(element * 2^e), bf16 [N][ldh], exact whenever the result is a normal bf16; written in the same pass when
 *     w_hat != NULL (the prefill's operand costs no extra read of w).
 * ldq is in bytes, >= K / 2 and % 16 == 0; lds >= K / 32; ldw >= K, ldh >= K, both % 8 == 0; w, packed and w_hat 16-byte aligned.
 * One launch; the argument checks come before it. */
int llmseg_quantize_rows_mxfp4(const void* w, int64_t ldw, int64_t N, int64_t K, void* packed, int64_t ldq, void* scale, int64_t lds,
                               void* w_hat /* nullable */, int64_t ldh, void* stream);
/* llmseg_gemm_mxfp4: C[m][n] = residual[m][n] + sum_k A[m][k] * w_hat[n][k], 1 <= M <= 8 (one token per sequence), with
 * w_hat[n][k] = element(Q[n][k / 2] nibble k % 2) * 2^(scale[n][k / 32] - 127) decoded on the fly (a block
 * of scale byte 0 -- what the quantiser writes below 6 * 2^-127, the all-zero block among them -- holds w_hat below the fp32 normal range, which may be flushed to zero).
 * A bf16 [M][lda]; Q uint8 [N][ldq] (ldq in bytes); scale uint8 [N][lds]; fp32 FMA accumulation of exact products; C bf16 or fp32
 * (out_f32; ldc in elements of the output type).  K % 32 == 0, lda % 8 == 0, ldq >= K / 2 and % 16 == 0, lds >= K / 32, A and Q
 * 16-byte aligned.  One launch (a vector-ALU weight stream at 1-2 rows, w_hat as the bf16 operand of the matrix cores from 3 rows: the products are exact
 * either way), no atomics: same inputs, same bits. */
typedef struct {
  uint32_t struct_size;  /* = sizeof(llmseg_gemm_mxfp4_args) of the caller's declaration (ABI guard, see above) */
  uint32_t reserved0;    /* 0 */
  const void* A; const void* Q; const void* scale;
  const void* residual;  /* bf16 [M][ldr] or NULL */
  void* C;
  int64_t M, N, K;
  int64_t lda, ldq, lds, ldc, ldr;
  int32_t out_f32; int32_t reserved1;
} llmseg_gemm_mxfp4_args;
int llmseg_gemm_mxfp4(const llmseg_gemm_mxfp4_args* args, void* stream);

/* ---- sampling (generate(do_sample=True)): temperature, top-k, top-p, the draw, the eos rule: ONE launch ----
 * Per row n of logits [N][ldl] bf16, with temperature T > 0, top_k k >= 0 (0 = off), top_p p in (0, 1] (1 = off) and a uniform u[n] in [0, 1),
 * in Hugging Face's order (temperature, top-k, top-p, draw), stated in exact arithmetic:
 *   1. z_i = l_i / T.
 *   2. K1 = { i : z_i >= the k-th largest z } when 1 <= k < V (ties at the k-th value are ALL kept), every index otherwise; -inf is never
 *      kept while a larger logit exists.
 *   3. q = softmax of z over K1.
 *   4. p < 1: m_i = sum of q_j over { j in K1 : q_j <= q_i };  K2 = { i in K1 : m_i > 1 - p }.  p = 1: K2 = K1.  A group of equal logits is
 *      kept or dropped AS A WHOLE; the top group has m = 1 and is always kept (min_tokens_to_keep = 1).  (TopPLogitsWarper splits a tie group
 *      that straddles the boundary by torch.sort's unspecified order; this rule keeps the whole group, so its kept set is a superset whose
 *      extra members all have the smallest kept logit.)
 *   5. r_i = q_i / sum_{K2} q.  next[n] = the smallest i in K2, in TOKEN-ID order, with sum_{j in K2, j <= i} r_j > u[n]; the largest index of
 *      K2 if rounding leaves none.  logprob[n] = ln r_next.
 * Then the greedy loop's eos rule, when eos >= 0: a row with unfinished[n] == 0 emits `pad` (logprob 0), and unfinished[n] &= (next[n] != eos);
 * unfinished == NULL: every row is unfinished.  eos < 0: no eos rule, `unfinished` is not touched.
 * Optional outputs (NULL = not written): logprob fp32 [N]; kept int32 [N] = |K2|; probs fp32 [N][ldp] = r, zeros outside K2.
 * Arithmetic: a token's weight is e = expf((l - l_max) / T) in fp32, held as the integer floor(e * 2^40) (2^(62 - bits(V)) above V = 2^22);
 * every sum (per-bin mass of the two-level histogram selects on the order-preserving 16-bit key, the softmax denominator, the CDF) is an
 * INTEGER sum and every threshold ((1 - p) S, u S2: formed once in fp64, floored) an integer compare: no floating-point atomics and no
 * order-dependent sum, so the result is a pure function of (logits, T, k, p, u).  One workgroup per row; V <= 32768 reads the row once into
 * registers, larger V re-reads it per pass.  next[n] is always in [0, V) (or `pad`); a row with a NaN or without a finite logit gives an
 * unspecified token of that range.  Checked before the launch: pointers and their alignment, 1 <= N, V < 2^31, ldl >= V, ldp >= V, T finite
 * and > 0, k >= 0, 0 < p <= 1. */
int llmseg_sample_tokens(const void* logits, int64_t ldl, int64_t N, int64_t V, float temperature, int32_t top_k, float top_p, const float* u,
                         int64_t eos, int64_t pad, int64_t* unfinished /* nullable, in/out */, int64_t* next, float* logprob /* nullable */,
                         int32_t* kept /* nullable */, float* probs /* nullable */, int64_t ldp, void* stream);

/* ---- logits processors (generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=)): ONE launch per token ----
 * Per row n: the logits l (bf16, V entries of logits[n][.], rewritten IN PLACE) and the row's history h[0 .. len): its prompt ids as given (the <image> placeholder
 * -200 stays in as it is) followed by every token it has emitted so far.  First the append, when `append` is given: append[n] is written at hist[n][hist_len[n]]
 * and hist_len[n] grows by 1; a full row (hist_len[n] >= ld_hist) drops the write and does not count it.  hist_len[n] is clamped to [0, ld_hist] when read.  Then,
 * on the history INCLUDING the appended token, in Hugging Face's order (processors come before the warpers of llmseg_sample_tokens):
 *   1. repetition penalty theta > 0 (1 = off): every DISTINCT token t of the history with 0 <= t < V, exactly once however often it occurs:
 *      l_t <- bf16(fl32(l_t) * fl32(theta)) if l_t < 0, else bf16(fl32(l_t) / fl32(theta)): a true fp32 division, the result rounded to nearest even; -0.0 (not
 *      < 0: divided, stays -0.0), +inf, -inf and NaN (the canonical quiet NaN 0x7fc0) fall out of that formula.  This is RepetitionPenaltyLogitsProcessor on a
 *      bf16 tensor, bit for bit.
 *   2. no-repeat n-gram g >= 0 (0 = off): if len >= g, for every j in [0, len - g] with h[j .. j + g - 2] == h[len - g + 1 .. len - 1] (raw int64 values), the
 *      token h[j + g - 1] gets -inf if it lies in [0, V).  g = 1 bans every token of the history; len < g bans nothing.  (NoRepeatNGramLogitsProcessor; the prompt
 *      counts, as it does there.)
 *   3. minimum length: l_ban <- -inf for ban_token >= 0 (-1 = none).  All rows step together, so the host knows how many tokens were emitted and passes the eos id
 *      while fewer than min_new_tokens were (MinNewTokensLengthLogitsProcessor).
 *   4. suppressed tokens: every id of the device list suppress[0 .. n_suppress) that lies in [0, V) gets -inf (SuppressTokensLogitsProcessor; the Python wrapper
 *      refuses ids outside [0, V) given on the host).
 * Steps 2 to 4 only write -inf, and a penalised -inf stays -inf (theta > 0), so the result does not depend on the order of the steps.  A row that ends up with every
 * logit -inf gives an unspecified token of [0, V) at the pick.  Two deviations from Hugging Face: history values outside [0, V) are skipped by steps 1 and 2 (HF's
 * gather on -200 is an out-of-range index; inside a compared window they still compare as values); and the history of a finished row goes on collecting `pad`, which is
 * harmless because a finished row emits `pad` whatever its logits say.
 * One workgroup per row; only the O(len) affected logits are touched, never the whole row.  A token at several history positions is penalised ONCE: every thread
 * loads the original logit of ALL its positions, a barrier, then every thread stores f(original) -- duplicates store the same bits -- which holds because the whole
 * history is loaded before the first store: hence the cap on ld_hist.  The -inf writes follow a second barrier.  No floating-point atomics: a pure function of the inputs.
 * Checked before the launch (LLMSEG_EINVAL): logits, hist, hist_len non-NULL; alignment (8 for int64, 4 for int32, 2 for bf16); N >= 1; 1 <= V < 2^31; ldl >= V;
 * 1 <= ld_hist <= LLMSEG_LOGITS_HIST_CAP; theta finite and > 0; no_repeat_ngram >= 0; ban_token in [-1, V); n_suppress >= 0, and 0 exactly when suppress is NULL. */
#define LLMSEG_LOGITS_HIST_CAP 4096
int llmseg_logits_process(void* logits, int64_t ldl, int64_t N, int64_t V, int64_t* hist, int64_t ld_hist, int32_t* hist_len /* in/out */,
                          const int64_t* append /* nullable */, float repetition_penalty, int32_t no_repeat_ngram, int64_t ban_token,
                          const int32_t* suppress /* nullable */, int64_t n_suppress, void* stream);

/* ---- beam search (generate(num_beams >= 2)): one pick per token, TWO launches ----
 * N prompts, B = num_beams live beams each (2 <= B <= 16), V >= 2 B.  Inputs: logits bf16 [N * beams_in][ldl] (beams_in = 1 for the first pick, which reads the
 * prefill's one row per prompt; B afterwards), beam_scores fp32 [N * beams_in], done int32 [N], src_in int32 [N * B][ld_src], pos_rows int32 [N * B] (the position
 * of the token about to be fed to each row).  Per prompt n that is not done, in exact arithmetic:
 *   1. candidate (b, v) has score s_b + log_softmax(l_b)_v; rank the beams_in * V candidates by score descending, equal scores by the SMALLER flat index b * V + v,
 *      and take the best 2 B.
 *   2. walk them in rank order: an eos candidate (v == eos, eos >= 0) of rank < B is recorded, fin_parent[n][k] = b, fin_score[n][k] = its score, k counting from 0 in
 *      rank order, fin_count[n] = their number; an eos candidate of rank >= B is dropped; any other candidate fills the next free slot i < B:
 *      next_token[n B + i] = v, parent[n B + i] = b (the slot within the prompt, 0 .. beams_in - 1), next_scores[n B + i] = its score.  At most one candidate per
 *      beam is eos, so B slots are always filled.  step_best[n] = the score of rank 0.
 * A done prompt (done[n] != 0): next_token = pad, parent = own slot, next_scores = beam_scores unchanged, fin_count[n] = 0, step_best[n] = 0.
 * The table, for row r = n B + i with parent j and p = pos_rows[r]: src_out[r][t] = src_in[n B + j][t] for t < p - 1, src_out[r][p - 1] = n B + j (where the parent
 * wrote the key of the token it was just fed).  First pick (beams_in == 1; no decode step has run, the prefill's K and V lie in physical row n B only):
 * src_out[r][t] = n B for every t < p, src_in is not read.  Entries t >= p of src_out are NOT WRITTEN (they keep what the buffer held).  src_in == src_out is refused
 * (LLMSEG_EINVAL): one row's copy would read another row's output.
 * Arithmetic: with l_max the row's largest logit, a weight is e = expf(l - l_max) in fp32, held as the integer floor(e * 2^40); S = their INTEGER sum (associative:
 * any order gives the same bits); lse = fp32(ln(S) - 40 ln 2), the logarithm in fp64; score = fl(s_b + fl(fl(l - l_max) - lse)), three fp32 operations rounded once
 * each.  No floating-point atomics and no floating-point sum: the result is a pure function of the inputs, and two candidates of one row with equal bf16 logits get
 * EQUAL scores, so the flat-index rule is exact within a row.  The ranking compares these fp32 scores.
 * Checked before any launch: pointers (all required) and their alignment, 2 <= B <= 16, beams_in in {1, B}, 2 B <= V <= 2^22, ldl >= V, ld_src >= 1, eos < V,
 * pad >= 0, N >= 1, workspace_bytes >= N * beams_in * 2 B * 8 (8-byte aligned device memory, overwritten).  pos_rows[r] is clamped to ld_src.  A row with fewer than
 * 2 B finite logits, or with a NaN, gives unspecified tokens in [0, V) and parents in [0, beams_in). */
int llmseg_beam_step(const void* logits, int64_t ldl, const float* beam_scores, const int32_t* done, int64_t eos, int64_t pad, const int32_t* src_in,
                     int32_t* src_out, int64_t ld_src, const int32_t* pos_rows, int64_t N, int32_t B, int32_t beams_in, int64_t V, int64_t* next_token,
                     int32_t* parent, float* next_scores, float* step_best, int32_t* fin_count, int32_t* fin_parent, float* fin_score, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* ---- fused attention forward -----------------------------------------------------------------
 * O[b][h][q][:] = softmax_k( scale * Q.K^T + bias + mask ) V, online softmax in fp32, bf16 MFMA.
 * Q/K/V/O are addressed as base + b*stride_b + h*stride_h + row*stride_row (elements); head_dim in {32,64,80,128}.
 *  - causal + key_mask: HF LlamaAttention eager path (transformers 4.29; call site llava_llama.py:93-102)
 *  - rel_h/rel_w: SAM decomposed relative position (image_encoder.py:244-251, 354-392):
 *      bias(q,k) = rel_h[h][b][q][qh-kh+grid_h-1] + rel_w[h][b][q][qw-kw+grid_w-1], q=(qh,qw), k=(kh,kw) on a grid_h x grid_w grid,
 *      rel_* are fp32 [heads][batch*Nq][rel_ld] (the q . R^T products, as the strided-batched llmseg_gemm_bf16 with out_f32 writes them)
 *  - plain: CLIP / DINOv2 ViT attention, mask-selection head attention (model/transformer.py:319-341)
 * o_row_map (int32 [batch][Nq] or NULL): output row for query (b,q) inside O (rows of stride o_stride_row, ignoring
 * o_stride_b); negative = skip.  Used to fold SAM's window_unpartition + crop (image_encoder.py:291-318) into the store.
 */
typedef struct {
  uint32_t struct_size;  /* = sizeof(llmseg_attn_args) (ABI guard) */
  uint32_t reserved0;
  const void* Q; const void* K; const void* V; void* O;
  int64_t q_stride_b, q_stride_h, q_stride_row;
  int64_t k_stride_b, k_stride_h, k_stride_row;
  int64_t v_stride_b, v_stride_h, v_stride_row;
  int64_t o_stride_b, o_stride_h, o_stride_row;
  int32_t batch, heads, Nq, Nk, head_dim;
  float scale;
  int32_t causal;
  const uint8_t* key_mask;   /* [batch][Nk] 1 = attend, or NULL (Nk = the capacity when nk_dev is set); a row with no key to attend gets O = 0 */
  const float* rel_h; const float* rel_w; int32_t rel_ld, grid_h, grid_w;
  const int32_t* o_row_map;
  /* Fused variant for SAM's 14x14 windows (head_dim 80): instead of rel_h/rel_w pass the bf16 tables themselves,
   * [32][head_dim] with rows >= 27 zero; q . R^T is then computed inside the kernel (grid_h = grid_w = 14 still required). */
  const void* rel_tab_h; const void* rel_tab_w;
  /* optional fp32 [batch][heads][Nq]: log2-sum-exp of every score row (max*scale*log2e + log2 sum), what llmseg_attn_bwd needs */
  float* lse;
  /* optional device int32: the number of keys present NOW (<= Nk, which is then the capacity of K / V); read by the kernel, so that a
   * decode step captured in a hipGraph can be replayed while the KV cache grows (llava_llama.py:137-163 prepare_inputs_for_generation) */
  const int32_t* nk_dev;
  /* window gather (ABI 9; only with rel_tab_h / rel_tab_w): the kernel applies SAM's window_partition + zero padding (image_encoder.py:263-289) and window_unpartition +
   * crop (:291-318) itself.  Q / K / V / O rows are then the UNPARTITIONED token rows of images on a win_grid x win_grid grid (row = image * win_grid^2 + y * win_grid + x,
   * *_stride_row apart; *_stride_b and o_row_map are ignored), batch = images * win_nw^2 windows (win_nw = ceil(win_grid / 14)); row (iy, ix) of window (wy, wx) is token
   * (14 wy + iy, 14 wx + ix) or, outside the grid, the row pad_q / pad_k / pad_v (bf16, head h at + h * *_stride_h): the reference pads AFTER norm1 (:178-183), so a padded
   * token's q|k|v row is the projection's bias -- the q|k|v product then runs on the real tokens only (4096 instead of 4900 rows per 1024^2 image).  win_grid = 0: off. */
  int32_t win_grid; int32_t win_nw;
  const void* pad_q; const void* pad_k; const void* pad_v;
} llmseg_attn_args;
int llmseg_attn_fwd(const llmseg_attn_args* args, void* stream);
/* tuning knob, process-global (identical results up to fp32 summation order).  variant & 3 = the kernel of SAM's 14x14 windows (rel_tab_*):
 * 0 = the general tiled kernel, 1 = the resident-window kernel with register staging (persistent workgroups walk (window, head) items, no
 * key tiling), 2 [default] = its LDS-DMA form (the only one with the window gather).  At 2, a call that asks for lse takes the tiled kernel and
 * one whose k_stride_row != v_stride_row the register-staged one.  Bits 4 and up = the cap on the persistent workgroups of the window
 * kernels (0 = 256, one per CU); an item's arithmetic does not depend on it.  Bits 2-3 are ignored. */
int llmseg_attn_set_variant(int variant);

/* ---- fused attention backward ----------------------------------------------------------------
 * Gradients of O = softmax(scale * Q.K^T + mask) V w.r.t. Q, K, V (plain / causal / key_mask forms; no relative position:
 * the SAM tower is frozen).  Scores are recomputed tile by tile from Q, K and the forward's `lse`; nothing of size Nq x Nk is
 * written.  HF LlamaAttention backward (the LoRA gradients of training.py:218-226 flow through every layer's q/v) and the
 * mask-selection head's self attention (model/transformer.py:319-341).  head_dim in {32, 64, 128}; causal needs Nq == Nk.
 * Every tensor is addressed as base + b*stride_b + h*stride_h + row*stride_row (elements); dQ/dK/dV may be strided views of
 * one packed buffer.  delta is an fp32 [batch][heads][Nq] workspace (rowsum(dO * O), written by the dQ pass). */
typedef struct {
  uint32_t struct_size;  /* = sizeof(llmseg_attn_bwd_args) (ABI guard) */
  uint32_t reserved0;
  const void* Q; const void* K; const void* V; const void* O; const void* dO;
  void* dQ; void* dK; void* dV;
  int64_t q_stride_b, q_stride_h, q_stride_row;
  int64_t k_stride_b, k_stride_h, k_stride_row;
  int64_t v_stride_b, v_stride_h, v_stride_row;
  int64_t o_stride_b, o_stride_h, o_stride_row;
  int64_t do_stride_b, do_stride_h, do_stride_row;
  int64_t dq_stride_b, dq_stride_h, dq_stride_row;
  int64_t dk_stride_b, dk_stride_h, dk_stride_row;
  int64_t dv_stride_b, dv_stride_h, dv_stride_row;
  int32_t batch, heads, Nq, Nk, head_dim;
  float scale;
  int32_t causal;
  const uint8_t* key_mask;   /* [batch][Nk] 1 = attend, or NULL */
  const float* lse;
  float* delta;
  /* optional (ABI 8): fp32 [Nq][head_dim / 2] tables of a rotate-half rotation applied to every dQ and dK row (position = row index,
   * Nq == Nk) before it is stored, with llmseg_rope's arithmetic on the bf16-rounded gradient -- bit for bit what llmseg_rope over the
   * stored dQ | dK gives.  The Llama layer passes (cos, -sin): the inverse rotation of HF apply_rotary_pos_emb's backward
   * (modeling_llama.py, transformers 4.29), which used to be a launch of its own per layer.  head_dim 64 or 128. */
  const float* rope_cos; const float* rope_sin;
  /* 1: `delta` already holds rowsum(dO * O) (llmseg_gemm_args.dl_o wrote it): the delta launch is skipped (ABI 8) */
  int32_t delta_ready; int32_t reserved1;
} llmseg_attn_bwd_args;
int llmseg_attn_bwd(const llmseg_attn_bwd_args* args, void* stream);

/* ---- row-wise normalisation ------------------------------------------------------------------
 * y[row_map ? row_map[r] : r][:] = norm(x[r][:]) * w (+ b); statistics in fp32.
 * rms != 0: HF LlamaRMSNorm (variance over x^2, no mean, no bias).  Otherwise nn.LayerNorm / SAM LayerNorm2d in
 * channels-last form (common.py:31-43).  row_map folds SAM's window_partition (image_encoder.py:263-288) into the store
 * (padding rows of y are left untouched -- the caller zero-fills them once).
 */
int llmseg_norm(const void* x, const void* w, const void* b, void* y, int64_t rows, int64_t cols, int64_t ldx, int64_t ldy,
                float eps, int rms, const int32_t* row_map, void* stream);

/* RoPE, rotate-half form, applied in place to `heads` heads of width head_dim starting at x (row stride ld):
 * positions = row % T (HF LlamaRotaryEmbedding, position_ids = arange(T)); cos/sin fp32 [T][head_dim/2]. */
int llmseg_rope(void* x, const float* cos, const float* sin, int64_t rows, int64_t T, int32_t heads, int32_t head_dim,
                int64_t ld, void* stream);
/* Decode step of generation (HF LlamaAttention with past_key_values; call site llava_llama.py:93-102,137-163): qkv bf16 [N][3 * heads *
 * head_dim] (row stride ld) holds one new token per sequence.  With pos = *pos_dev: q is rotated in place at position pos, k is
 * rotated and written to kcache[n][pos], v is copied to vcache[n][pos] (caches bf16 [N][capacity][heads * head_dim], sequence stride
 * cache_stride_n elements).  cos/sin fp32 [capacity][head_dim/2].  The position lives in device memory so that the step can be
 * replayed from a hipGraph. */
int llmseg_rope_kv_append(void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                          const int32_t* pos_dev, int64_t N, int32_t heads, int32_t head_dim, void* stream);

/* The same decode step with the attention in the launch (head_dim 128): with pos = *pos_dev, k is rotated and written to kcache[n][pos], v
 * copied to vcache[n][pos], and out[n][h*128 ..] = softmax(rot(q_h) K_h^T * scale) V_h over the pos + 1 cached keys (HF LlamaAttention
 * with past_key_values and a one-token query: no mask).  qkv is not modified.  scratch (optional, fp32, >= N * heads * splits * 130 * 4
 * bytes for splits = min(16, 256 / (N * heads))): the keys of a head are split over workgroups until the launch covers the chip and a
 * second launch merges the partial softmaxes; without scratch one workgroup walks all keys of a head. */
int llmseg_decode_attn(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                       const int32_t* pos_dev, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                       void* scratch, int64_t scratch_bytes, void* stream);
/* llmseg_decode_attn with one position per sequence (a batch whose prompts differ in length): pos_rows_dev int32 [N] in device memory, and
 * sequence n uses pos = pos_rows_dev[n] for everything llmseg_decode_attn derives from *pos_dev -- the RoPE angle of its q and k, the
 * cache slot kcache[n][pos] / vcache[n][pos] it writes, and the pos + 1 keys it attends to.  Cache slots beyond a sequence's own position
 * are neither read nor written.  Same kernel, same argument checks, same scratch; equal positions give the bits of llmseg_decode_attn. */
int llmseg_decode_attn_rows(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                            const int32_t* pos_rows_dev, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                            void* scratch, int64_t scratch_bytes, void* stream);
/* llmseg_decode_attn_rows over a BEAM-INDEXED cache (beam search: the cache is never re-ordered, a table is).  R = N rows (prompts x beams); src int32
 * [R][ld_src] in device memory.  Write side as llmseg_decode_attn_rows: row r at pos = pos_rows_dev[r] rotates q and k and writes k / v to the physical slot
 * [r][pos].  Read side: it attends to keys t = 0 .. pos; key t < pos is read from physical row src[r][t], i.e. from kcache + src[r][t] * cache_stride_n + t * D
 * (D = heads * head_dim; vcache alike), key pos is the row's own new key (src[r][pos] is NOT read, nor any entry beyond it).  Entries of src are TRUSTED to
 * lie in [0, R): they are not checked, an entry outside reads outside the cache.  Checked before the launch: everything llmseg_decode_attn_rows checks, src
 * non-NULL and 4-byte aligned, ld_src >= capacity > 0 (capacity = the caches' positions per row: every position is < capacity).  Split count, scratch layout, key
 * groups and merge are llmseg_decode_attn_rows's with N := R: a table with src[r][t] == r gives its bits, in the output and in both caches. */
int llmseg_decode_attn_beams(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                             const int32_t* pos_rows_dev, const int32_t* src, int64_t ld_src, int64_t capacity, int64_t N, int32_t heads, int32_t head_dim,
                             float scale, void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- MXFP8 KV cache (OCP Microscaling: 8-bit E4M3 elements -- the OCP `fn` encoding gfx950 has natively, not MI300's `fnuz` -- and one E8M0 scale
 * per block of 32) ----
 * 8.25 bits per cached value: 4224 bytes instead of 8192 per token, layer and tensor at Llama-7B.  The rule, per bf16 row of D elements (D % 32 == 0, finite
 * values) and per block of 32 consecutive elements:
 *   amax = the largest |x| of the block;
 *   e = the smallest integer >= -127 with amax <= 448 * 2^e (amax == 0: e = -127); the scale byte is e + 127, one E8M0 byte.  For a normal
 *     amax = m * 2^E, m in [1, 2): e = E - 8 when m <= 1.75, else E - 7 (integer work on the bf16 bits).  A finite bf16 never needs e > 120: nothing
 *     saturates, and the NaN code 0x7f is never produced;
 *   y = x / 2^e (exact, |y| <= 448) is rounded to the nearest OCP E4M3 value (sign, 4 exponent bits of bias 7, 3 mantissa bits), ties to the even
 *     code, subnormals included: the smallest non-zero magnitude is 2^-9, and 2^-10 rounds to 0.  The sign bit is cleared when the magnitude is 0
 *     (-0 is never stored);
 *   x_hat = bf16(element * 2^e) has four significant bits: exact whenever it is a normal bf16.  A result below the smallest normal bf16 (possible only
 *     under a scale byte <= 9) is flushed to +0, in x_hat and in the decode step alike.  (|x| >= 1.96875 * 2^127 rounds to y = 256 under e = 120: element * 2^e
 *     is 2^128 there, not a finite bf16.)  x_hat is a fixed point of the rule in value; its bytes are too unless amax was rounded down onto 1.75 * 2^E (y = 224
 *     under e = E - 7), which the rule then stores as y = 448 under e = E - 8.
 * Layout of a cache row [n][t] of heads * 128 elements: bytes q[n][t][h * 128 + d], scales scale[n][t][h * 4 + d / 32].
 *
 * llmseg_kv_quantize_mxfp8: ONE launch over batch x rows rows of D elements.  Row (b, r) of an operand lives at base + b * stride_b + (row0 + r) * stride_r
 * (strides in elements of the operand: bf16 for x and x_hat, bytes for q and scale), row0 = row0_dev[b * row0_stride] (int32 in device memory,
 * row0_stride 0 or 1) or 0 when row0_dev is NULL: the same first row for every operand.  Outputs: q + scale (nullable as a pair) and x_hat bf16 (nullable);
 * at least one must be given.  x_hat may alias x (same strides): a block is read whole before any of it is written.  Two uses: the prefill (K and V
 * slices of the packed q|k|v buffer -> cache rows [n][0 .. T)), and a bf16 cache that holds x_hat, rewritten in place at slot [n][pos_n] with
 * row0_dev = the decode step's position tensor.  Checked before the launch: x non-NULL; x and x_hat 16-byte aligned with strides % 8 == 0, q 8-byte
 * aligned with strides % 8 == 0, row0_dev 4-byte aligned; D % 32 == 0; batch, rows >= 1; every row stride >= the row's extent (D, or D / 32 for scale) and,
 * for batch > 1, every batch stride >= rows * row stride. */
int llmseg_kv_quantize_mxfp8(const void* x, int64_t x_stride_b, int64_t x_stride_r, void* q, int64_t q_stride_b, int64_t q_stride_r, void* scale,
                             int64_t s_stride_b, int64_t s_stride_r, void* x_hat, int64_t h_stride_b, int64_t h_stride_r, const int32_t* row0_dev,
                             int64_t row0_stride, int64_t batch, int64_t rows, int64_t D, void* stream);
/* llmseg_decode_attn / _rows / _beams on the packed cache: kcache / vcache uint8 [N][capacity][heads * 128] (cache_stride_n bytes per sequence), kscale /
 * vscale uint8 [N][capacity][heads * 4] (scale_stride_n bytes per sequence).  pos_stride 0: one position *pos_dev for every sequence; 1: pos_dev[n].  src
 * (nullable): the beam table of llmseg_decode_attn_beams with ld_src >= capacity > 0; NULL: every row reads its own row.  The rule of a step: the new
 * token's k (after RoPE) and v take part in this step's attention as the bf16 values just computed, exactly as on the bf16 routes; slot [n][pos] receives
 * their MXFP8 rounding (128 bytes and four scale bytes per head and tensor); every earlier key is element * 2^e, decoded on load.  One more compile-time
 * instance of the one kernel: key -> lane mapping, trip, split count, scratch and merge are the bf16 routes', so `out` equals, bit for bit, the bf16 entry
 * point on the cache of x_hat values.  Bytes beyond a row's position are never read.  Checked before the launch: what the bf16 entry points check with
 * 8-byte instead of 16-byte cache alignment, cache_stride_n >= heads * 128, the scales non-NULL and 4-byte aligned with scale_stride_n % 4 == 0 and >= heads * 4,
 * pos_stride 0 or 1, head_dim 128. */
int llmseg_decode_attn_mxfp8(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                             void* kscale, void* vscale, int64_t scale_stride_n, const int32_t* pos_dev, int64_t pos_stride, const int32_t* src /* nullable */,
                             int64_t ld_src, int64_t capacity, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                             void* scratch, int64_t scratch_bytes, void* stream);

/* ---- prompt-lookup decoding (generate(prompt_lookup_num_tokens = k)): Q = k + 1 tokens per sequence and step, THREE entry points ----
 * A step feeds sequence n its last emitted token and up to k draft tokens as the step rows n * Q .. n * Q + Q - 1, verifies the drafts against the step's own
 * arg-maxes and keeps the longest confirmed prefix plus one more token.  Every emitted token is the arg-max of the logits computed at the position in front of
 * it: the result is a greedy continuation.
 *
 * llmseg_decode_attn_chunk: llmseg_decode_attn_rows for Q tokens per sequence (bf16 cache, head_dim 128, 1 <= Q <= LLMSEG_DECODE_CHUNK_MAX).  qkv [N * Q][ld];
 * with pos = pos_rows_dev[n], token j of sequence n is rotated at pos + j (cos / sin fp32 [capacity][64]), its k (rotated) and v are written to cache slot
 * [n][pos + j], and out[n * Q + j] = softmax over the keys 0 .. pos + j (the chunk is causal within itself).  The bits written to the cache are those Q successive
 * llmseg_decode_attn_rows steps write; no other cache element is touched; a slot at or beyond `capacity` is not written (the caller keeps pos + Q <= capacity).
 * A cached K or V row is loaded once and serves all Q queries; the Q new rows are taken from LDS by every workgroup of the head and stored by exactly one.  Key
 * split and merge are llmseg_decode_attn's; scratch (optional): >= N * Q * heads * splits * 130 * 4 bytes for splits = min(16, 256 / (N * heads)), fewer
 * splits if it is smaller.  Slots beyond the position the caller moves to afterwards hold keys of rejected tokens: the next step overwrites Q slots from the new
 * position on before any query's key count reaches them.  Checked before the launch: what llmseg_decode_attn_rows checks, 1 <= Q <= LLMSEG_DECODE_CHUNK_MAX,
 * N * Q < 65536, Q <= capacity, cache_stride_n >= capacity * heads * 128, ld >= 3 * heads * 128, ldo >= heads * 128. */
#define LLMSEG_DECODE_CHUNK_MAX 8
int llmseg_decode_attn_chunk(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                             const int32_t* pos_rows_dev, int64_t capacity, int64_t N, int32_t Q, int32_t heads, int32_t head_dim, float scale,
                             void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream);
/* llmseg_lookup_draft, ONE launch (one workgroup per row): the draft of Hugging Face's PromptLookupCandidateGenerator.get_candidates (no logits processor, no eos
 * cut) on the row's history h[0 .. len) = hist[n][0 .. hist_len[n]) -- the buffer of llmseg_logits_process: prompt ids as given, the <image> placeholder included,
 * then the emitted tokens; ld_hist <= LLMSEG_LOGITS_HIST_CAP.  For g = min(max_ngram, len - 1) down to 1: among the windows h[i .. i + g) equal to the last g ids
 * (raw int64 values) whose continuation is not empty (i + g < len: the tail itself is no match) the EARLIEST is taken, and the first g that has one ends the
 * search.  The draft is h[i + g ..), at most k ids, cut at the end of the history, at max_new_tokens - count[n] - 1 ids (the step emits the accepted drafts and
 * one more token) and before the first id outside [0, V).  No match: draft length 0.  A row with unfinished[n] == 0 or count[n] >= max_new_tokens drafts nothing.
 * forced (nullable, int64 [N][ld_forced]; a test hook): the draft is forced[n][count[n] ..) instead of the lookup, under the same three cuts (ld_forced for the
 * end of the history).  Written: tok [N][k + 1] = the last id of the history (the last emitted token), the draft, then pad_token; draft_len [N].
 * Checked before the launch: non-NULL pointers and their alignment, 1 <= N, V < 2^31, 1 <= ld_hist <= LLMSEG_LOGITS_HIST_CAP, 0 <= k < LLMSEG_DECODE_CHUNK_MAX,
 * max_ngram >= 1, max_new_tokens >= 1. */
int llmseg_lookup_draft(const int64_t* hist, int64_t ld_hist, const int32_t* hist_len, const int32_t* count, const int32_t* unfinished, int64_t N,
                        int32_t k, int32_t max_ngram, int32_t max_new_tokens, int64_t V, int64_t pad_token, const int64_t* forced /* nullable */,
                        int64_t ld_forced, int64_t* tok, int32_t* draft_len, void* stream);
/* llmseg_lookup_accept, TWO launches (the arg-max of every step row; one thread per sequence for the rule): logits bf16 [N * Q][ldl], V entries a row.  With
 * m_j = argmax(logits[n * Q + j]) -- the lowest index among equal values, a NaN as the largest value: torch.argmax -- and d = draft_len[n] (0 without tok):
 *   a = the number of leading drafts j = 1 .. d with tok[n][j] == m_(j - 1);
 *   the row emits m_0 .. m_a (the accepted drafts and one more token), cut at max_new_tokens - count[n] tokens and after the first eos_token (-1 = none);
 *   a row with unfinished[n] == 0 or count[n] >= max_new_tokens emits nothing (a = 0).
 * In place, with e = the number of tokens emitted: they are appended to hist[n] at hist_len[n] (writes at or beyond ld_hist are dropped), hist_len[n] and count[n]
 * grow by e, unfinished[n] becomes 0 if an eos was emitted, and pos_rows[n] grows by e unless `first` -- the fed tokens that stand are the last emitted token and
 * the accepted drafts, a + 1 less what the cuts took.  `first` != 0 is the pick after the prefill: Q = 1, no drafts, nothing was fed, the position stays.
 * map (nullable, int64 [N * Q]; needs base int64 [N]): step row n * Q + j holds the state of the row's emitted token count[n] - 1 + j (count before the step); map
 * receives base[n] + count[n] + j where that token stands (j < e, not `first`), else dump_row.  rec int32 [4][N]: unfinished | count | a | d after the step, one
 * buffer for one device-to-host copy.  argmax_ws: int32 [N * Q].  Checked before the launch: non-NULL pointers and their alignment, N >= 1,
 * 1 <= Q <= LLMSEG_DECODE_CHUNK_MAX, 1 <= V < 2^31, ldl >= V, tok and draft_len as a pair (required for Q > 1), 1 <= ld_hist <= LLMSEG_LOGITS_HIST_CAP,
 * max_new_tokens >= 1. */
int llmseg_lookup_accept(const void* logits, int64_t ldl, int64_t N, int32_t Q, int64_t V, const int64_t* tok /* nullable */, const int32_t* draft_len /* nullable */,
                         int32_t first, int64_t eos_token, int32_t max_new_tokens, int64_t* hist, int64_t ld_hist, int32_t* hist_len /* in/out */,
                         int32_t* pos_rows /* in/out */, int32_t* unfinished /* in/out */, int32_t* count /* in/out */, const int64_t* base /* nullable */,
                         int64_t dump_row, int64_t* map /* nullable */, int32_t* rec, int32_t* argmax_ws, void* stream);

/* y[i] = act(x[i]), bf16, n % 8 == 0, in place allowed (the GELU between LayerNorm2d and the second transposed convolution of SAM's
 * mask decoder, mask_decoder.py:53-63: every other activation on the path rides in a GEMM epilogue) */
int llmseg_act(const void* x, void* y, int64_t n, int32_t act, void* stream);
/* Sam.postprocess_masks (model/segment_anything/modeling/sam.py:137-172), fused: low fp32 [n_masks][256*256] mask logits ->
 * F.interpolate(bilinear, align_corners=False) to img_size^2 -> crop [:in_h, :in_w] -> F.interpolate to (out_h, out_w); out fp32
 * [n_masks][out_h][out_w].  nested = 1: `low` is in the row order the GEMM-form transposed convolutions emit (see head.hip). */
int llmseg_sam_postprocess(const float* low, float* out, int32_t n_masks, int32_t img_size, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                           int32_t nested, void* stream);
/* SAM prompt encoder for point / box / mask prompts (model/segment_anything/modeling/prompt_encoder.py:56-64,78-114,203-238), what
 * `SamPredictor.predict_torch` runs in front of the mask decoder.  Every stage is fp32; the one rounding is the bf16 store.
 *   llmseg_sam_dense_prompt: keys bf16 [b][4096][256] = feats bf16 [4096][256] (one image's embedding, channels-last rows) + the dense
 *     prompt.  mask fp32 [b][65536] low-resolution logits: cell p of prompt i gets feats[p] + mask_downscaling(mask_i)[:, p] (Conv 2x2 s2 ->
 *     LayerNorm2d(4, eps 1e-6) -> erf GELU -> Conv 2x2 s2 -> LayerNorm2d(16) -> GELU -> Conv 1x1 to 256; the ten tensors bf16 in the
 *     reference's layouts [4][1][2][2], [4], [4], [4], [16][4][2][2], [16], [16], [16], [256][16], [256]).  nested = 1: `mask` is in the row
 *     order llmseg_sam_postprocess reads (the mask decoder's own output order), nested = 0: raster 256 x 256.  mask == NULL: keys = feats +
 *     no_mask bf16 [256] for every prompt, the bits of llmseg_add_rows on the repeated embedding; the ten tensors may then be NULL.
 *   llmseg_sam_prompt_tokens: out bf16 [b][n + (boxes ? 2 : 1)][256] = PromptEncoder._embed_points / _embed_boxes.  coords fp32 [b][n][2]
 *     (x, y) in the frame x frame input, labels int32 [b][n] (-1: the not_a_point vector alone, 0 / 1: + point embedding 0 / 1), boxes fp32
 *     [b][4] XYXY or NULL (NULL: one padding token is appended; else the two corners + point embeddings 2 / 3), gauss fp32 [2][128],
 *     pe0..pe3 / not_a_point bf16 [256].  n = 0 with boxes is legal.  Nothing is read on the host. */
int llmseg_sam_dense_prompt(const void* feats, const float* mask, int32_t b, int32_t nested, const void* no_mask, const void* w0, const void* b0,
                            const void* ln1_w, const void* ln1_b, const void* w3, const void* b3, const void* ln4_w, const void* ln4_b, const void* w6,
                            const void* b6, void* keys, void* stream);
int llmseg_sam_prompt_tokens(const float* coords, const int32_t* labels, const float* boxes, int32_t b, int32_t n, int32_t frame, const float* gauss,
                             const void* pe0, const void* pe1, const void* pe2, const void* pe3, const void* not_a_point, void* out, void* stream);
/* SAM "everything" mode (model/segment_anything/automatic_mask_generator.py:264-324, utils/amg.py:78-88,156-176,303-346), per candidate
 * mask at the ORIGINAL resolution without materialising the logits there.  low fp32 [n][256*256] (nested as above):
 *   llmseg_sam_mask_stats: stats int32 [n][7] += { |m > thr + off|, |m > thr - off|, |m > thr|, min x, min y, max x, max y } of the
 *     post-processed mask m; the caller initialises rows to {0, 0, 0, INT_MAX, INT_MAX, -1, -1}.  iou (optional, fp32 [n]): candidates
 *     with !(iou > iou_thresh) are skipped (pred_iou_thresh filter).  stability score = stats[0] / stats[1]; box = stats[3..6].
 *   llmseg_sam_binarize: out uint8 [n_sel][out_h][out_w] = m[sel[k]] > thr for the surviving candidates.
 *   llmseg_nms: greedy box NMS with torchvision.ops.nms semantics (one category): boxes fp32 [*][4] XYXY, order int32 [n] = candidate
 *     indices by decreasing score, keep uint8 [n] (position in `order`). */
int llmseg_sam_mask_stats(const float* low, const float* iou, float iou_thresh, int32_t* stats, int32_t n_masks, int32_t img_size, int32_t in_h,
                          int32_t in_w, int32_t out_h, int32_t out_w, int32_t nested, float mask_threshold, float offset, void* stream);
int llmseg_sam_binarize(const float* low, const int32_t* sel, uint8_t* out, int32_t n_sel, int32_t img_size, int32_t in_h, int32_t in_w, int32_t out_h,
                        int32_t out_w, int32_t nested, float mask_threshold, void* stream);
int llmseg_nms(const float* boxes, const int32_t* order, int32_t n, float iou_threshold, uint8_t* keep, void* stream);
/* SAM everything mode beyond the default single crop (SURVEY.md 8f N1 remainder; csrc/image.hip), byte work on the device:
 *   llmseg_image_resize_u8: `ResizeLongestSide.apply_image` (model/segment_anything/utils/transforms.py:27-35, called by
 *     `SamPredictor.set_image`, predictor.py:34-60) = Pillow's 8-bit BILINEAR `Image.resize`, bit-identical.  in uint8 [in_h][in_w][channels]
 *     with `in_row_stride` bytes between rows -- a crop of a crop layer (automatic_mask_generator.py:254-257) is an origin pointer + the full
 *     image's row stride; out uint8 [out_h][out_w][channels] dense.  workspace >= llmseg_image_resize_workspace(...) bytes (its layout is
 *     stated once, below llmseg_mask_union).  "Bit-identical to Pillow" holds per channel, 1 <= channels <= 4: Pillow premultiplies `LA` /
 *     `RGBA` images by their alpha before it resamples them, this kernel resamples every channel on its own and should.
 *   llmseg_sam_preprocess: `Sam.preprocess` (modeling/sam.py:174-186): in uint8 [h][w][3] -> out bf16 [3][img_size][img_size],
 *     (x - mean[c]) / std[c] inside the image, zero in the padding; mean / std are HOST pointers to 3 floats.
 *   llmseg_mask_small_regions: `remove_small_regions(mask, min_area, "holes")` then `(..., "islands")` (utils/amg.py:267-291, as
 *     `postprocess_small_regions` applies them, automatic_mask_generator.py:347-350) on masks uint8 [K][H][W] IN PLACE (0 / non-zero in,
 *     0 / 1 written where a pixel changes); changed uint8 [K] = 1 when either pass altered the mask.  8-connected components
 *     (cv2.connectedComponentsWithStats(.., 8) in the reference) by union-find; when every island is below min_area the largest is kept
 *     (first in raster order among equals).  workspace >= llmseg_mask_small_regions_workspace(K, H, W) bytes.
 *   llmseg_mask_boxes: `batched_mask_to_box` (utils/amg.py:303-346): boxes int32 [K][4] XYXY (inclusive; zeros for an empty mask),
 *     areas int32 [K] (optional); workspace >= 20 bytes per mask. */
int64_t llmseg_image_resize_workspace(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t channels);
int llmseg_image_resize_u8(const uint8_t* in, int64_t in_row_stride, uint8_t* out, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                           int32_t channels, void* workspace, int64_t workspace_bytes, void* stream);
int llmseg_sam_preprocess(const uint8_t* in, void* out, int32_t h, int32_t w, int32_t img_size, const float* mean, const float* std_, void* stream);
int64_t llmseg_mask_small_regions_workspace(int32_t K, int32_t H, int32_t W);
int llmseg_mask_small_regions(uint8_t* masks, int32_t K, int32_t H, int32_t W, int32_t min_area, uint8_t* changed, void* workspace,
                              int64_t workspace_bytes, void* stream);
int llmseg_mask_boxes(const uint8_t* masks, int32_t K, int32_t H, int32_t W, int32_t* boxes, int32_t* areas, void* workspace, int64_t workspace_bytes,
                      void* stream);
/* The raw-image front end of inference (llmseg_amd/segment.py; csrc/image.hip):
 *   llmseg_image_resize_u8_filter: llmseg_image_resize_u8 with the resampling filter as an argument.  LLMSEG_RESAMPLE_BILINEAR is that entry
 *     point itself (same bits, same limits); LLMSEG_RESAMPLE_BICUBIC is Pillow's 8-bit BICUBIC `Image.resize`, bit-identical (Resample.c:
 *     a = -0.5, support = 2 * max(scale, 1), taps in double, normalised, rounded to 22-bit fixed point with -0.5 for the negative lobes,
 *     horizontal then vertical pass with clip8 and a uint8 intermediate).  Down-scaling up to 63x per axis (255 taps).
 *     workspace >= llmseg_image_resize_filter_workspace(...) bytes.
 *   llmseg_clip_preprocess: `CLIPImageProcessor.preprocess` with the CLIP-L/14 settings the reference loads (utils/llm_seg_dataset.py:127):
 *     shortest edge -> size with BICUBIC (resized long side = int(size * long / short), transformers `get_resize_output_image_size`), centre
 *     crop size x size (origin (resized - size) / 2, rounded down), * 1/255, (x - mean[c]) / std[c].  in uint8 [h][w][3] with `in_row_stride` bytes
 *     between rows -> out bf16 [3][size][size].  Only the crop window is resampled; both passes keep Pillow's uint8 rounding, so the result is
 *     that of resizing the whole image, cropping and normalising.  mean / std are HOST pointers to 3 floats.
 *     workspace >= llmseg_clip_preprocess_workspace(h, w, size) bytes.
 *   llmseg_mask_union: out uint8 [C][H][W] = 1 where any mask k with select[c][k] != 0 is non-zero, else 0 (the union of the chosen proposals,
 *     training.py:712-733).  masks uint8 [K][H][W], select uint8 [C][K] on the DEVICE (no host synchronisation); masks that no row selects
 *     are not read.  16-byte accesses where the addresses are 16-byte aligned.
 * Workspace of llmseg_image_resize_workspace / llmseg_image_resize_filter_workspace / llmseg_clip_preprocess_workspace, as the calls leave it
 * (tests read the tap tables back and compare them with Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` integer for integer):
 *   horizontal table   at byte 0: out_w rows (`size` rows for CLIP) of ksize + 2 int32, a row = {first input index, tap count, taps zero-filled
 *                      to ksize}, ksize = 2 * ceil(support) + 1 with support = max(in / out, 1) (BILINEAR) or twice that (BICUBIC).  Written
 *                      only when the width changes.
 *   vertical table     at the next 256-byte boundary: out_h rows (`size` for CLIP) in the same form, written only when the height changes.
 *   intermediate       at the next 256-byte boundary: uint8 [in_h][out_w][channels], written only when both passes run (CLIP: the rows
 *                      the window's vertical taps reach x `size` columns, whenever the width changes).
 *   CLIP tables hold the crop window's output indices only (columns left .. left + size, rows top .. top + size of the resized image); the
 *   vertical one stores its first indices minus the first input row the call reads.
 *   A call depends on nothing the workspace held before, and ksize <= 64 (BILINEAR) / 256 (BICUBIC) on both axes or the call is refused. */
enum { LLMSEG_RESAMPLE_BILINEAR = 0, LLMSEG_RESAMPLE_BICUBIC = 1 };
int64_t llmseg_image_resize_filter_workspace(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t channels, int32_t filter);
int llmseg_image_resize_u8_filter(const uint8_t* in, int64_t in_row_stride, uint8_t* out, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                                  int32_t channels, int32_t filter, void* workspace, int64_t workspace_bytes, void* stream);
int64_t llmseg_clip_preprocess_workspace(int32_t h, int32_t w, int32_t size);
int llmseg_clip_preprocess(const uint8_t* in, int64_t in_row_stride, void* out, int32_t h, int32_t w, int32_t size, const float* mean, const float* std_,
                           void* workspace, int64_t workspace_bytes, void* stream);
int llmseg_mask_union(const uint8_t* masks, const uint8_t* select, uint8_t* out, int32_t K, int32_t C, int32_t H, int32_t W, void* stream);
/* out[r][c] = silu(gu[r][c]) * gu[r][I + c]   (HF LlamaMLP: down(silu(gate(x)) * up(x)); gu = x.[Wgate;Wup]^T) */
int llmseg_swiglu(const void* gu, void* out, int64_t rows, int64_t I, int64_t ldgu, int64_t ldo, void* stream);

/* y[r][:] = x[r][:] + add[(r % add_rows)][:]  (positional embeddings; x may alias y) */
int llmseg_add_rows(const void* x, const void* add, void* y, int64_t rows, int64_t cols, int64_t add_rows, void* stream);

/* im2col for stride==kernel patch embedding: img bf16 [B][3][H][W] -> cols bf16 [B*gh*gw][ldo], column = c*p*p + i*p + j,
 * zero-filled up to ldo.  (PatchEmbed image_encoder.py:395-426; CLIP/DINOv2 patch convs.)  out_row_offset/out_rows_per_img
 * let the caller leave a CLS row at the front of each image's block. */
int llmseg_patchify(const void* img, void* cols, int32_t B, int32_t H, int32_t W, int32_t p, int64_t ldo,
                    int64_t out_rows_per_img, int64_t out_row_offset, void* stream);

/* 3x3 / pad 1 im2col on a channels-last map: x bf16 [B][H][W][C] -> cols [B*H*W][9*C], column = (ky*3+kx)*C + c
 * (SAM neck conv, image_encoder.py:100-106; the weight is re-laid-out to match at load time). */
int llmseg_im2col3x3(const void* x, void* cols, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);

/* LLaVA splice (llava_arch.py:185-208): out[n][t][:] = embed[ids] for text positions, img_feats[n][t-img_pos] inside the
 * image span.  ids int64 [N][L] with exactly one IMAGE token (-200) per row; out [N][L-1+P][H]; sequence n's P feature
 * rows start at img_feats + n*feats_stride_n (elements), so a CLS row per image can be skipped in place. */
int llmseg_embed_splice(const int64_t* ids, const void* embed, const void* img_feats, void* out, int32_t N, int32_t L,
                        int32_t P, int32_t H, int64_t vocab, int64_t feats_stride_n, void* stream);

/* gather rows: out[i][:] = x[idx[i]][:] (bf16, cols % 8 == 0) -- [SEG] hidden-state gather (LISA.py:322-323) */
int llmseg_gather_rows(const void* x, const int64_t* idx, void* out, int64_t n, int64_t cols, int64_t ldx, void* stream);

/* Fused bilinear-upsample + mask pooling (LISA.py:350-361, 201-218):
 * pooled[k][c] = sum_p segs[k][p] * Up(feat)[c][p] / (sum_p segs[k][p] + 1e-8), Up = F.interpolate(size=S, bilinear,
 * align_corners=False) of the channels-last bf16 map feat [g*g][C].  Computed as (segs . U) . feat, i.e. the mask is
 * pulled back through the adjoint of the interpolation, so the [C][S][S] upsampled tensor is never materialised and
 * `segs` (K*S*S bf16, the only large operand) is read from HBM exactly once.  feat bf16 [g*g][C]; pooled bf16 [K][C].
 * ws: caller-provided bf16 [K][g*g] workspace (the normalised pulled-back masks; stage 2 is an MFMA GEMM over it).
 * Optional outputs for the backward pass (NULL = skip): pulled_back fp32 [K][g*g] = segs . U, wsum fp32 [K] = sum_p segs. */
/* Stage 1 of the above alone: ws[k][:] = (segs[k] . U) / (sum_p segs[k][p] + 1e-8) as bf16 [K][g*g] (+ the optional fp32 outputs),
 * so that a caller can pool several images with ONE strided-batched llmseg_gemm_bf16 (trans_w) over their feature maps. */
int llmseg_mask_pullback(const void* segs, void* ws, float* pulled_back, float* wsum, int32_t K, int32_t g, int32_t S, void* stream);
int llmseg_upsample_maskpool(const void* feat, const void* segs, void* pooled, void* ws, float* pulled_back, float* wsum, int32_t K,
                             int32_t C, int32_t g, int32_t S, void* stream);

/* Cosine scoring (LISA.py:398-403): sim[k] = <t,e_k> / (|t||e_k|); t bf16 [D], e bf16 [K][D]; sim fp32 [K]. */
int llmseg_cosine_scores(const void* t, const void* e, float* sim, int32_t K, int32_t D, void* stream);

/* ---- ABI 7: the mask-selection head with fp32 ACTIVATIONS (inference scores; weights stay the model's bf16 tensors) ------------------------
 * What these replace on the reference side: the nn.Linear / nn.LayerNorm / Attention modules of model/transformer.py:215-341 and the scoring of
 * model/LISA.py:340-408 when the reference is run in fp32 on the CPU (its own "CPU path" of north_star).  Plain fp32 FMA chains, ascending k (linear_f32: one chain per K step of 16, the steps' sums added in order). */
/* y[m][n] = act(alpha * sum_k x[m][k] * W(n,k) + bias[n]) + residual[m][n];  x fp32 [M][ldx], residual fp32 [M][ldr] or NULL, y fp32 [M][ldy];
 * W bf16: w_kn = 0 -> stored [N][ldw] (nn.Linear weight, F.linear); w_kn = 1 -> stored [K][ldw] (right operand given K-major: the channels-last
 * feature map of the mask pooling, LISA.py:201-218); bias bf16 [N] or NULL. */
int llmseg_linear_f32(const float* x, int64_t ldx, const void* W, int64_t ldw, int32_t w_kn, const void* bias, const float* residual, int64_t ldr,
                      float* y, int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t act, float alpha, void* stream);
/* nn.LayerNorm over the last dimension (transformer.py:236-283 norm1..4): x, y fp32 [rows][D] contiguous; w, b bf16 [D] (b may be NULL). */
int llmseg_layernorm_f32(const float* x, const void* w, const void* b, float* y, int64_t rows, int32_t D, float eps, void* stream);
/* softmax(q k^T * scale) v (transformer.py:319-341), all fp32; strides[12] = {q, k, v, o} x {batch, head, row} in elements; head_dim 32 or 64. */
int llmseg_attn_f32(const float* q, const float* k, const float* v, float* o, const int64_t* strides, int32_t batch, int32_t heads, int32_t Nq, int32_t Nk,
                    int32_t head_dim, float scale, void* stream);
/* llmseg_cosine_scores on fp32 operands: t fp32 [D], e fp32 [K][D] -> sim fp32 [K]. */
int llmseg_cosine_f32(const float* t, const float* e, float* sim, int32_t K, int32_t D, void* stream);

/* softmax_align_loss + iou_regression_loss (model/loss.py:50-94) for `items` (image, round) pairs with the same K, one workgroup
 * each, every operand contiguous over items (e [items][K][D], t [items][D], gt_iou / pred_iou / gt_iop [items][K]); fp32 results:
 * out[i][0] = KL(softmax(gt_iou/tau) || softmax(cos(e_k,t)/tau)) summed; out[i][1] = mean((p-g)^2 exp(g-1)) * 50.
 * Optional gradients: d_e fp32 [items][K][D], d_t fp32 [items][D], d_pred fp32 [items][K] (of out[i][0] resp. out[i][1]; NULL = skip). */
int llmseg_align_reg_loss(const void* e, const void* t, const float* gt_iou, const void* pred_iou, const float* gt_iop,
                          float* out, float* d_e, float* d_t, float* d_pred, int32_t K, int32_t D, float tau, int32_t items, void* stream);

/* dice_loss + sigmoid_ce_loss (model/loss.py:4-47; named by the north_star, no caller in the reference):
 * logits bf16/fp32-as-float [M][HW] given as fp32, targets fp32; out[0] = dice (scale 1000, eps 1e-6), out[1] = bce,
 * both summed over masks / (num_masks + 1e-8).  out must be zeroed by the caller.  workspace >= 8 M bytes (per-mask terms, folded in order). */
int llmseg_dice_bce(const float* logits, const float* targets, float* out, int32_t M, int64_t HW, float num_masks, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* gradient of g[0] * dice + g[1] * bce w.r.t. the logits (g: device fp32[2], the upstream gradients of the two losses) */
int llmseg_dice_bce_bwd(const float* logits, const float* targets, const float* g, float* dlogits, int32_t M, int64_t HW, float num_masks, void* stream);

/* Shifted cross-entropy over bf16 logits (llava_llama.py:108-118): rows = N*T positions, labels int64 [N][T] already in
 * spliced form; position (n,t) is scored against labels[n][t+1]; ignore_index -100.  acc fp32[2] += {sum nll, count}.
 * workspace >= 8 N (T - 1) bytes (per-position terms, folded in order). */
int llmseg_ce_loss(const void* logits, const int64_t* labels, float* acc, int32_t N, int32_t T, int64_t V, int64_t ldl,
                   void* workspace, int64_t workspace_bytes, void* stream);


/* gIoU / cIoU bookkeeping (reference utils/utils.py:119-132 `intersectionAndUnionGPU`, K = 2 classes): pred/target uint8 [n],
 * pixels with target == ignore_index are dropped; out int64[6] += {I0, I1, U0, U1, T0, T1} (exact integer counts). */
int llmseg_intersection_union(const uint8_t* pred, const uint8_t* target, int64_t n, int32_t ignore_index, int64_t* out, void* stream);

/* validate_threshold's per-image body (training.py:712-766) in one pass: union of the proposals with select[k] != 0 (segs uint8
 * [H][W][K], the reader's layout), nearest-resize of that union and of gt (uint8 [Hg][Wg], 255 = ignore) to out_h x out_w, 2-class I/U.
 * `validate` (arg-max of the similarity, training.py:605-687) is the same with a one-hot select and out = Hg x Wg.
 * out int64[6] += {I0, I1, U0, U1, T0, T1}. */
int llmseg_union_resize_iou(const uint8_t* segs, const uint8_t* select, const uint8_t* gt, int32_t H, int32_t W, int32_t K, int32_t Hg, int32_t Wg,
                            int32_t out_h, int32_t out_w, int32_t ignore_index, int64_t* out, void* stream);

/* ---- proposal decode + training targets on the device (the reference does this per sample on CPU workers) -----
 * rle_decode: COCO run-length proposals -> dense uint8 masks (pycocotools `mask_util.decode`, utils/sam_mask_reader.py:86-87).  run_ends =
 *   inclusive prefix sums of every mask's run lengths, concatenated; offsets int64 [K+1] delimits mask k's slice; runs alternate 0 / 1 from 0
 *   and walk the image column-major.  out uint8 [K][H][W] (hwk = 0) or [H][W][K] (hwk = 1, the reader's layout).  Pixels beyond the last run of a
 *   run list that ends before H W (malformed input) are 0, after an even or an odd number of runs.
 * mask_targets: `compute_all_iou` / `compute_all_iop` (utils/utils.py:234-272) for all K proposals: ground truth gt [Hg][Wg] resampled to the
 *   proposals' H x W grid through the nearest-neighbour index maps gy [H], gx [W] (skimage.transform.resize(order=0) rule, built on the host
 *   in float64), counts int64 [K][2] += {|seg & gt|, |seg|}, gt_area int64 [1] += |gt'| (caller zero-fills both), then
 *   iou[k] = I / (S + G - I), iop[k] = I / S as IEEE doubles (0 / 0 = nan, as numpy gives the reference).  Integer parts are exact.
 * resize_aa: proposal maps (utils/reason_seg_dataset.py:166-173): masks uint8 [K][H][W], zero-padded bottom / right to the square of side
 *   max(H, W), resampled to out_size x out_size with torch's antialiased bilinear filter, written as bf16 [K][out][out].  Tap tables per
 *   output index (first source index, tap count, float64 weights [out][taps]) come from the host (aten `_compute_indices_weights_aa`). */
/* One pass over the proposals (round 4): gt_resample writes the ground truth on the proposals' grid once (gtp uint8 [H][W] = gt[gy[y]][gx[x]] != 0);
 * proposal_targets reads every selected proposal ONCE -- proposal k is masks[order[k]] (order int64 [K] or NULL = identity: no gathered copy) --
 * and produces the bf16 [K][out][out] antialiased maps (the arithmetic of llmseg_resize_aa, evaluated separably: bit-identical) AND, for n_gt <= 4
 * ground truths gtp [n_gt][H][W], counts int64 [n_gt][K][2] = {|seg & gt'|, |seg|}, gt_area int64 [n_gt], iou / iop double [n_gt][K] (all plainly
 * written).  Limits: out_size <= 256, taps <= 28, W <= 2048; beyond them use llmseg_mask_targets + llmseg_resize_aa. */
int llmseg_gt_resample(const uint8_t* gt, const int32_t* gy, const int32_t* gx, uint8_t* out, int32_t H, int32_t W, int32_t Hg, int32_t Wg, void* stream);
int llmseg_proposal_targets(const uint8_t* masks, const int64_t* order, const uint8_t* gtp, int32_t n_gt, void* out, int32_t K, int32_t H, int32_t W,
                            int32_t out_size, const int32_t* y0, const int32_t* ny, const double* wy, const int32_t* x0, const int32_t* nx,
                            const double* wx, int32_t taps, int64_t* counts, int64_t* gt_area, double* iou, double* iop, void* stream);
int llmseg_rle_decode(const uint32_t* run_ends, const int64_t* offsets, uint8_t* out, int32_t K, int32_t H, int32_t W, int32_t hwk, void* stream);
int llmseg_mask_targets(const uint8_t* segs, const uint8_t* gt, const int32_t* gy, const int32_t* gx, int32_t K, int32_t H, int32_t W, int32_t Hg,
                        int32_t Wg, int64_t* counts, int64_t* gt_area, double* iou, double* iop, void* stream);
int llmseg_resize_aa(const uint8_t* segs, void* out, int32_t K, int32_t H, int32_t W, int32_t out_size, const int32_t* y0, const int32_t* ny,
                     const double* wy, const int32_t* x0, const int32_t* nx, const double* wx, int32_t taps, void* stream);

/* ---- the COCO RLE codec on the device: the FILE format of the proposals (prepare_datasets: pycocotools `mask.encode`; loader: rleFrString) --
 * rle_encode: dense masks uint8 [K][H][W] (row-major, non-zero = inside; 0 / 255 masks count like 0 / 1) -> maskApi rleEncode + rleToString.
 *   Runs walk the image column-major (p = x H + y), alternate 0 / 1 starting with a zero run (the first count is 0 when pixel (0, 0) is set) and
 *   continue across column boundaries; counts from the fourth on are stored as deltas against the count two back; characters are 5-bit groups,
 *   low group first, bit 5 = continuation, bit 4 of the last group = sign, + 48.  H W < 2^31.
 *   counts uint32 [K][cap_counts], chars uint8 [K][cap_chars]; n_counts[k] / n_chars[k] int32 ALWAYS hold the true sizes.  A mask that exceeds a
 *   cap has its row truncated -- counts: the first cap_counts run lengths; chars: the first cap_chars characters of the counts that were
 *   stored -- and nothing is written past either row; the caller retries with caps >= max(n_counts), max(n_chars) (a count needs at most 7
 *   characters).  Output positions come from prefix sums (no atomics on any output): the same input gives the same bytes on every run.
 *   workspace >= llmseg_rle_encode_ws_bytes(K, H, W) bytes, 16-byte aligned.
 * rle_parse: the K compressed strings, concatenated (chars [total], char_offsets int64 [K+1] on the device, char_offsets[0] = 0, total =
 *   char_offsets[K]) -> the inputs of llmseg_rle_decode: run_ends uint32 = inclusive prefix sums (mod 2^32) of each mask's counts, concatenated;
 *   run_offsets int64 [K+1] delimits the slices.  A string never has more counts than characters: run_ends needs room for `total` elements.
 *   Strings of at most 7 groups per count (every encoder's output for H W < 2^31) give the bits of the host parse; any other byte content gives
 *   unspecified VALUES, but no read leaves chars [0, total) and no write leaves run_ends [0, total) / run_offsets [0, K + 1).
 *   workspace >= llmseg_rle_parse_ws_bytes(K, total) bytes. */
int64_t llmseg_rle_encode_ws_bytes(int32_t K, int32_t H, int32_t W);
int llmseg_rle_encode(const uint8_t* masks, int32_t K, int32_t H, int32_t W, uint32_t* counts, int32_t* n_counts, int32_t cap_counts, uint8_t* chars,
                      int32_t* n_chars, int32_t cap_chars, void* workspace, int64_t workspace_bytes, void* stream);
int64_t llmseg_rle_parse_ws_bytes(int32_t K, int64_t total_chars);
int llmseg_rle_parse(const uint8_t* chars, const int64_t* char_offsets, int32_t K, uint32_t* run_ends, int64_t* run_offsets, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* ---- backward pass + optimizer (trainable part: LoRA'd Llama stack, embed/lm_head, text_hidden_fcs, mask-selection head) -----
 * GEMM-shaped gradients use llmseg_gemm_bf16 with trans_a / trans_w (dX = dY W, dW = dY^T X); the kernels below are the
 * streaming pieces.  Gradients of the loss kernels: llmseg_align_reg_loss (d_e, d_t, d_pred). */
/* out[n] += sum_m x[m][n]  (bias gradients, fp32 accumulation; caller zero-fills out).  workspace: up to 64 N floats (row slices). */
int llmseg_colsum(const void* x, float* out, int64_t M, int64_t N, int64_t ld, void* workspace, int64_t workspace_bytes, void* stream);
/* LayerNorm / RMSNorm backward (contiguous rows): dx bf16; dw/db fp32 accumulated (NULL = frozen weight).  workspace (only read when dw or
 * db is given): rows of <= 1024 columns use up to 256 x 2 cols floats of partials (NULL: one workgroup); wider rows NEED 2 rows + 2 cols
 * floats (row statistics) and use up to 64 x 2 cols more. */
int llmseg_norm_bwd(const void* dy, const void* x, const void* w, void* dx, float* dw, float* db, int64_t rows, int64_t cols,
                    float eps, int rms, void* workspace, int64_t workspace_bytes, void* stream);
/* same, dx = norm backward + dres (bf16 [rows][cols] or NULL): x of a pre-norm block also feeds the residual connection, and the
 * gradient arriving that way is added here instead of in a separate pass (HF LlamaDecoderLayer: hidden = residual + sublayer(norm(hidden))) */
int llmseg_norm_bwd_add(const void* dy, const void* x, const void* w, const void* dres, void* dx, float* dw, float* db, int64_t rows, int64_t cols,
                        float eps, int rms, void* workspace, int64_t workspace_bytes, void* stream);
/* SwiGLU backward: gu [rows][2I] (gate|up), dout [rows][I] -> dgu [rows][2I] */
int llmseg_swiglu_bwd(const void* gu, const void* dout, void* dgu, int64_t rows, int64_t I, void* stream);
/* out = dy * f'(y) computed from the OUTPUT y of a fused GEMM epilogue (act = RELU or SIGMOID) */
int llmseg_act_bwd(const void* dy, const void* y, void* out, int64_t n, int act, void* stream);
/* Backward of a SMALL trainable Linear y = act(x W^T + b) in ONE launch (ABI 10): dy, y [M][N], x [M][K], w [N][K], all bf16 and dense (row pitch = width).
 *   dpre = dy * act'(y) with llmseg_act_bwd's arithmetic, rounded to bf16 (act = NONE: dpre = dy and y may be NULL; else RELU or SIGMOID);
 *   dx [M][K] bf16 = dpre W;   dw [N][K] fp32 = dpre^T x;   db [N] fp32 = column sums of dpre.   Any of dx / dw / db may be NULL (skipped).
 * accumulate = 1: dw and db are `+=` (the fp32 gradient arena), 0: they are overwritten.  A workgroup owns a 32 x 64 tile of dw (or of dx, a second range of the
 * same grid) and walks the whole contraction (M rows, or N columns) itself: no partial sums leave the workgroup, every sum has a fixed order, no workspace.
 * Any M, N, K >= 1 (N = 1, M % 16 != 0, K % 64 != 0 are handled in the kernel; rows whose pitch is not a multiple of 8 elements are read element-wise).
 * Returns LLMSEG_NOT_TAKEN without launching when M > 2048 or N K > 2^22: there the walk is too long for one workgroup (wide Linears, lm_head). */
int llmseg_linear_bwd(const void* dy, const void* y, int act, const void* x, const void* w, void* dx, float* dw, float* db, int64_t M, int64_t N, int64_t K,
                      int accumulate, void* stream);
/* Materialised attention probabilities for the backward pass (T <= a few hundred: Llama T=319, head K<=512):
 * P[b][q][k] = softmax_k(scale * S[b][q][k] + causal/key mask), S fp32 [BH][Tq][ld], P bf16 same shape, columns >= Tk zero.
 * key_mask uint8 [BH/heads][Tk] or NULL; causal requires Tq == Tk. */
int llmseg_softmax_rows(const float* S, void* P, int64_t BH, int32_t Tq, int32_t Tk, int32_t ld, float scale, int32_t causal,
                        const uint8_t* key_mask, int32_t heads, void* stream);
/* dS[r][k] = scale * P[r][k] * (dP[r][k] - sum_k' P[r][k'] dP[r][k'])  (softmax backward; rows = BH*T) */
int llmseg_attn_ds(const void* P, const float* dP, void* dS, int64_t rows, int32_t T, int32_t ld, float scale, void* stream);
/* dlogits = coef[0] * (softmax(logits) - onehot(shifted label)); zero for ignored positions (llava_llama.py:108-118 backward) */
int llmseg_ce_bwd(const void* logits, const int64_t* labels, const float* coef, void* dlogits, int32_t N, int32_t T, int64_t V,
                  int64_t ldl, void* stream);
/* dst[idx[i]][:] += src[i][:] in fp32 (embedding / row-gather gradients; idx < 0 skipped); source rows that share a destination are added
 * in ascending source order by one workgroup (no atomics) */
int llmseg_scatter_add_rows(const void* src, const int64_t* idx, float* dst, int64_t n, int64_t cols, void* stream);
/* Rank-8 LoRA products (peft==0.4.0 Linear with r = 8, lora_dropout 0.05: training.py:91,218-226) -- skinny shapes a tiled GEMM
 * cannot fill.  Every kernel handles the q AND the v branch of one layer in one launch (second operand set NULL = one branch);
 * branch b uses dropout stream drop->stream + b:
 *   lora_down:  y[m][8b..8b+7] = alpha * drop_b(x_b)[M][K] . W_b^T  (W stored [8][K], or [K][8] when w_kr), rows of y at pitch ldy,
 *               the following zero_cols columns of each row zero-filled                            fwd drop(x).A^T, bwd dq.Bq | dv.Bv
 *   lora_outer: out_b(n,r) += alpha * sum_m drop_b(a_b)[m][n] b_b[m][r]  (fp32 [N][8], or [8][N] when out_rn; accumulates)   dB, dA
 *   lora_apply: y[M][N] += alpha * sum_b mask_b * (xa[M][8b..8b+7] . W_b^T)  (W stored [N][8], or [8][N] when w_rn)   bwd dx of the LoRA branches
 *   lora_pack:  the two [*][64] extension operands of llmseg_gemm_args (A2 / W2) for a LoRA'd q|k|v projection, from the current
 *               LoRA matrices: w2b [3H][64] = rows [s Bq | 0], 0, [0 | s Bv | 0];  w2a [H][64] = rows [Aq[:,h] | Av[:,h] | 0];
 *               bt [16][H] = Bq^T | Bv^T (K-contiguous rows: the backward's dq.Bq | dv.Bv then runs on the MFMA form of lora_down);
 *               every output is optional (NULL)
 * Dropout (NULL = none, as in eval mode) is counter-based, nothing is stored: Philox4x32-10 with key = rng_state[0] (seed), counter
 * = (element index / 8, stream, rng_state[1] (offset)); the 16-bit field j of the 128-bit output decides element 8 idx + j, kept
 * when field >= drop_thr (= round(p * 65536)) and scaled by 65536 / (65536 - drop_thr); element index = row * width + column of
 * the dense [M][width] activation.  rng_state is DEVICE memory (a captured hipGraph reads a fresh offset on every replay).
 * seg_rows > 0 (ABI 5): the M rows are consecutive SEGMENTS of seg_rows rows -- the micro-batches of a gradient-accumulation window run as
 * one pass -- and segment s = row / seg_rows draws the mask a separate pass over it would draw at offset + s: element index =
 * (row % seg_rows) * width + column, counter offset = rng_state[1] + s. */
typedef struct {
  const uint64_t* rng_state;   /* device: {seed, offset} */
  uint32_t stream;             /* which dropout module (layer * 2 + {q = 0, v = 1}) */
  uint32_t drop_thr;           /* round(p * 65536); 0 = no dropout */
  uint32_t seg_rows;           /* 0 = one segment (all rows at rng_state[1]) */
  uint32_t reserved0;          /* 0 */
} llmseg_dropout;
/* lora_down (ABI 17: one entry point with a sized argument struct; it replaces llmseg_lora_down_ws / _parts / _pack). */
typedef struct {
  uint32_t struct_size;  /* = sizeof(llmseg_lora_down_args) (ABI guard) */
  uint32_t reserved0;    /* 0 */
  const void* x0;        /* [M][K] at row pitch ldx */
  const void* x1;        /* second branch (with w1), or NULL: one branch; may equal x0 (one load feeds both, each with its own dropout stream) */
  int64_t ldx;
  const void* w0;        /* [8][K], or [K][8] when w_kr */
  const void* w1;
  void* y;               /* [M][8 nb + zero_cols] at row pitch ldy */
  int64_t ldy;
  int64_t M, K;
  int32_t w_kr;
  float alpha;
  int32_t zero_cols;     /* multiple of 8, <= 480 */
  int32_t reserved1;     /* 0 */
  const llmseg_dropout* drop;
  /* caller-owned scratch (fp32; NULL = none; >= 2 * 32 * M * 16 * 4 bytes lets every split be taken): short activations (M = 2 x 319) are split along K over
   * several workgroups per 16-row tile so that the whole chip fetches the operand, and a second launch (the finish) adds the slices in order */
  void* scratch;
  int64_t scratch_bytes;
  /* both set or both NULL.  Set: a K-sliced product is left UNFINISHED: *parts_S = slice count with the fp32 partials [S][M][16] in `scratch` and y untouched
   * (hand them to llmseg_gemm_args.nb_lora_part), or 0 when the shape took no slices and y is complete; *parts_scale = alpha * dropout scale (the finish
   * factor), written on every successful call. */
  int32_t* parts_S;
  float* parts_scale;
  /* pack_aq != NULL: llmseg_lora_pack(pack_aq, ..., pack_s) of the same layer in the same call.  The two are independent (activations vs. weights): where the
   * down projection runs as K slices the pack rides in its finish launch -- one launch fewer per LoRA'd projection -- else it is one more launch; the same
   * bits as the two calls.  Not together with parts_S (LLMSEG_EINVAL, nothing launched). */
  const void *pack_aq, *pack_bq, *pack_av, *pack_bv;
  void *pack_w2b, *pack_w2a, *pack_bt;
  int64_t pack_H;
  float pack_s;
  int32_t reserved2;     /* 0 */
} llmseg_lora_down_args;
int llmseg_lora_down(const llmseg_lora_down_args* args, void* stream);
/* workspace: row slices x nz (1 or 2 products) x 8 N floats of partials (NULL, or room for fewer than two slices: one slice, no fold launch).
 * The dispatch takes max(1, 256 / (ceil(N / 64) * nz), min(32, M / 512)) slices -- 256 for N = 8 with one product -- cut to what the
 * workspace holds; slices * nz * 8 N * 4 bytes lets every slice be taken (at most 256 * 8 * 64 * 4 = 512 KiB below M = 1024, 32 slices above). */
int llmseg_lora_outer(const void* a0, const void* a1, int64_t lda, const void* b0, const void* b1, int64_t ldb, float* out0, float* out1, int64_t M,
                      int64_t N, int32_t out_rn, float alpha, const llmseg_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream);
/* The four weight gradients of a LoRA'd q|k|v projection in ONE launch (+ one fold): with d = dqkv (dq, dv: column blocks at row pitch ldd),
 * xa = [drop_q(x) Aq^T | drop_v(x) Av^T] [M][>= 16] (the forward's extension operand), t = [s dq Bq | s dv Bv] [M][>= 16]:
 *   gbq [H][8] += s dq^T xa[:, 0:8],  gbv [H][8] += s dv^T xa[:, 8:16],  gaq [8][H] += t[:, 0:8]^T drop_q(x),  gav [8][H] += t[:, 8:16]^T drop_v(x)
 * (dropout streams drop->stream / + 1, as llmseg_lora_down uses them).  workspace: row slices x 4 x 8 H floats,
 * slices = max(1, 256 / (4 ceil(H / 64)), min(32, M / 512)) as for llmseg_lora_outer with nz = 4 (one slice at M = 638, H = 4096; 14 at M = 7656). */
int llmseg_lora_wgrads(const void* dq, const void* dv, int64_t ldd, const void* x, int64_t ldx, const void* xa, int64_t ldxa, const void* t, int64_t ldt,
                       float* gbq, float* gbv, float* gaq, float* gav, int64_t M, int64_t H, float s, const llmseg_dropout* drop, void* workspace,
                       int64_t workspace_bytes, void* stream);
int llmseg_lora_apply(void* y, int64_t ldy, const void* xa, int64_t ldxa, const void* w0, const void* w1, int64_t M, int64_t N, int32_t w_rn,
                      float alpha, const llmseg_dropout* drop, void* stream);
int llmseg_lora_pack(const void* aq, const void* bq, const void* av, const void* bv, void* w2b, void* w2a, void* bt, int64_t H, float s, void* stream);
/* out[c][r] = in[r][c] (bf16; in [rows][cols] with leading dimension ld_in, out [cols][ld_out]); rows r in [rows, rows_pad) of the
 * source are taken as zero.  Lets the weight / input gradients of a wide trainable Linear (lm_head: dX = dY.W, dW = dY^T.X) run on
 * the K-contiguous LDS-DMA GEMM kernels with the contraction dimension padded to a multiple of 64. */
int llmseg_transpose_pad(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, int64_t rows_pad, void* stream);
/* out[0] += sum x^2 (global gradient-norm clipping, training.py:301 "gradient_clipping": 1.0).  workspace: required, 8 KiB holds every
 * workgroup's partial (fewer bytes = fewer workgroups). */
int llmseg_sumsq(const void* x, int64_t n, int is_f32, float* out, void* workspace, int64_t workspace_bytes, void* stream);
/* Fused AdamW on fp32 master weights + bf16 model copy (DeepSpeed config training.py:292-332: betas (0.9, 0.95), wd 0).
 * grad is bf16 (grad_f32 = 0) or fp32; grad_scale (device fp32 scalar or NULL) carries 1/accum and the clip coefficient. */
int llmseg_adamw(void* p, float* master, const void* grad, int grad_f32, float* m, float* v, int64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, void* stream);

/* ---- per-kernel timing (bench roofline): HIP events recorded around every GEMM launch on its own stream ---------- */
int llmseg_prof_enable(int on);                 /* 1 = record events around GEMM launches */
/* syncs the events, resets; totals over every GEMM launch, and the same for the dominant kernel only
 * (gemm_bf16_tn_glds_kernel<false, 2, 1>: bf16-out 128x128 LDS-DMA variant) so that it can be compared with rocprofv3's per-kernel row */
/* name of the GEMM kernel class that took the most time in the last collected window (its totals are dom_*) */
const char* llmseg_prof_dominant_kernel(void);
/* algorithmic bytes (A + W + C read / written once, bf16) summed over that class's launches in the last collected window */
double llmseg_prof_dominant_bytes(void);
/* composition of that class in the last collected window (a timed record is one user-level llmseg_gemm_bf16 CALL): out4 = {calls, calls that ran
 * as K-slices, K-slices summed over those calls, kernel launches = calls + one splitk_reduce_kernel per K-sliced call} */
int llmseg_prof_dominant_info(int64_t* out4);
int llmseg_prof_collect(double* total_ms, double* total_flops, int64_t* launches, double* dom_ms, double* dom_flops, int64_t* dom_launches);

#ifdef __cplusplus
}
#endif
#endif
