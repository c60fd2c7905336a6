// SAM prompt encoder for point / box / mask prompts (model/segment_anything/modeling/prompt_encoder.py:56-64,78-114,203-238): the two
// launches `SamPredictor.predict_torch` needs in front of the mask decoder.
//   llmseg_sam_dense_prompt  -- the decoder's keys: image embedding + mask_downscaling(mask) (or + no_mask_embed), one launch
//   llmseg_sam_prompt_tokens -- the sparse tokens of points and box corners, one launch
// Both evaluate every stage in fp32 and round once, at the bf16 store.  This file is compiled with the compiler's default contraction
// (head.hip's tail is not): nothing here is held to another kernel bit for bit except the mask == NULL route, which only adds.
#include "common.h"

namespace {

// ---- dense prompt --------------------------------------------------------------------------------------------------------------
// Conv 2x2 s2 (1 -> 4) -> LayerNorm2d(4) -> GELU -> Conv 2x2 s2 (4 -> 16) -> LayerNorm2d(16) -> GELU -> Conv 1x1 (16 -> 256), per cell of
// the 64 x 64 grid: cell (y, x) reads the 4 x 4 logits at (4 y + 2 dy1 + dy2, 4 x + 2 dx1 + dx2) -- in the nested layout (head.hip, above
// sam_low) these are the 16 contiguous floats at 16 p, sub-index (dy1 2 + dx1) 4 + dy2 2 + dx2, so stage-1 pixel q = dy1 2 + dx1 is one
// 16-byte load.
// A workgroup owns 64 consecutive cells of one prompt.
//   phase A: thread (cell = t / 4, q = t % 4) evaluates stage-1 pixel q (4 channels), takes the other three pixels of its cell from its
//            neighbour lanes, and evaluates channels 4 q .. 4 q + 3 of stage 2; the LayerNorm(16) statistics are two xor-shuffles.  The 16
//            activations of a cell go to LDS (4 KiB per workgroup, one ds_write_b128 per thread).
//   phase B: the store phase.  Lane l of a wave owns channels 8 (l % 32) .. + 7 and holds their 8 x 16 last-stage weights in registers for
//            the whole workgroup; a wave writes two whole 512-byte rows per 16-byte store instruction, reading a cell's activations as LDS
//            broadcasts (one address per half wave) and the embedding row (L2-resident: 2 MB shared by every prompt) with 16-byte loads.
//            (Requesting a lane's eight embedding chunks ahead of phase A changed nothing measurable: the kernel is bound by instruction
//            issue, not by that latency -- profiles/sam_predictor.md.)
constexpr int DP_CELLS = 64;
constexpr float LN2D_EPS = 1e-6f;

struct DenseW {          // the ten mask_downscaling tensors, bf16 as the model stores them
  const bf16_t *w0, *b0, *g1, *e1, *w3, *b3, *g4, *e4, *w6, *b6;
};
// offsets of the small tensors inside the fp32 LDS image
constexpr int OW0 = 0, OB0 = 16, OG1 = 20, OE1 = 24, OW3 = 28, OB3 = 284, OG4 = 300, OE4 = 316, NSMALL = 332;

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

__global__ __launch_bounds__(256) void sam_dense_prompt_kernel(const bf16_t* __restrict__ feats, const float* __restrict__ mask, int nested, DenseW W,
                                                              bf16_t* __restrict__ keys) {
  __shared__ float sw[NSMALL];
  __shared__ __attribute__((aligned(16))) float sh[DP_CELLS][16];
  const int t = threadIdx.x, tile = blockIdx.x, i = blockIdx.y;
  for (int k = t; k < NSMALL; k += 256) {
    const bf16_t v = k < OB0 ? W.w0[k] : k < OG1 ? W.b0[k - OB0] : k < OE1 ? W.g1[k - OG1] : k < OW3 ? W.e1[k - OE1] : k < OB3 ? W.w3[k - OW3]
                   : k < OG4 ? W.b3[k - OB3] : k < OE4 ? W.g4[k - OG4] : W.e4[k - OE4];
    sw[k] = bf2f(v);
  }
  // last-stage weights of this lane's 8 channels: 128 contiguous bf16 of the [256][16] matrix
  const int cg = t & 31;
  float w6[8][16], b6[8];
  {
    const uint4* src = reinterpret_cast<const uint4*>(W.w6 + cg * 128);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unpack8(src[2 * j], &w6[j][0]);
      unpack8(src[2 * j + 1], &w6[j][8]);
    }
    unpack8(*reinterpret_cast<const uint4*>(W.b6 + cg * 8), b6);
  }
  __syncthreads();

  {  // ---- phase A
    const int c = t >> 2, q = t & 3;
    const int p = tile * DP_CELLS + c;
    const float* m = mask + (long)i * 65536;
    float in[4];                                            // [dy2 2 + dx2]
    if (nested) {
      const float4 v = *reinterpret_cast<const float4*>(m + 16 * p + 4 * q);
      in[0] = v.x; in[1] = v.y; in[2] = v.z; in[3] = v.w;
    } else {
      const int Y = 4 * (p >> 6) + 2 * (q >> 1), X = 4 * (p & 63) + 2 * (q & 1);
      const float2 r0 = *reinterpret_cast<const float2*>(m + Y * 256 + X), r1 = *reinterpret_cast<const float2*>(m + (Y + 1) * 256 + X);
      in[0] = r0.x; in[1] = r0.y; in[2] = r1.x; in[3] = r1.y;
    }
    float s[4], mu = 0.f, var = 0.f;
#pragma unroll
    for (int co = 0; co < 4; ++co) {
      float a = sw[OB0 + co];
#pragma unroll
      for (int k = 0; k < 4; ++k) a = fmaf(sw[OW0 + co * 4 + k], in[k], a);
      s[co] = a;
      mu += a;
    }
    mu *= 0.25f;
#pragma unroll
    for (int co = 0; co < 4; ++co) { s[co] -= mu; var = fmaf(s[co], s[co], var); }
    float rs = 1.f / sqrtf(var * 0.25f + LN2D_EPS);
#pragma unroll
    for (int co = 0; co < 4; ++co) s[co] = gelu_erf(fmaf(sw[OG1 + co], s[co] * rs, sw[OE1 + co]));
    // stage 2: out channel co = 4 q + j sums w3[co][ci][dy1][dx1] over the cell's four stage-1 pixels (lanes 4 c .. 4 c + 3) and their 4 channels
    float z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = sw[OB3 + 4 * q + j];
    const int base = (t & 63) & ~3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const float v = __shfl(s[ci], base + k, 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = fmaf(sw[OW3 + ((4 * q + j) * 4 + ci) * 4 + k], v, z[j]);
      }
    }
    mu = z[0] + z[1] + z[2] + z[3];
    mu += __shfl_xor(mu, 1, 64);
    mu += __shfl_xor(mu, 2, 64);
    mu *= 0.0625f;
    var = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { z[j] -= mu; var = fmaf(z[j], z[j], var); }
    var += __shfl_xor(var, 1, 64);
    var += __shfl_xor(var, 2, 64);
    rs = 1.f / sqrtf(var * 0.0625f + LN2D_EPS);
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = gelu_erf(fmaf(sw[OG4 + 4 * q + j], z[j] * rs, sw[OE4 + 4 * q + j]));
    *reinterpret_cast<float4*>(&sh[c][4 * q]) = make_float4(z[0], z[1], z[2], z[3]);
  }
  __syncthreads();

  // ---- phase B: wave w stores rows 16 w .. 16 w + 15 of the tile, two per instruction
  const int w = t >> 6, half = (t >> 5) & 1;
#pragma unroll 2
  for (int it = 0; it < 8; ++it) {
    const int r = w * 16 + it * 2 + half;
    const long p = (long)tile * DP_CELLS + r;
    const uint4 fv = *reinterpret_cast<const uint4*>(feats + p * 256 + cg * 8);
    float h[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(&sh[r][4 * k]);
      h[4 * k] = v.x; h[4 * k + 1] = v.y; h[4 * k + 2] = v.z; h[4 * k + 3] = v.w;
    }
    float f[8];
    unpack8(fv, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = b6[j];
#pragma unroll
      for (int k = 0; k < 16; ++k) a = fmaf(w6[j][k], h[k], a);
      f[j] += a;
    }
    *reinterpret_cast<uint4*>(keys + ((long)i * 4096 + p) * 256 + cg * 8) = pack8(f);
  }
}

// mask == NULL: keys[i][p][:] = feats[p][:] + no_mask[:], the operations of add_rows_kernel (pointwise.hip) on feats.repeat(b, 1)
__global__ __launch_bounds__(256) void sam_dense_nomask_kernel(const bf16_t* __restrict__ feats, const bf16_t* __restrict__ no_mask, bf16_t* __restrict__ keys,
                                                              long total) {
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long)gridDim.x * blockDim.x) {
    const long row = k >> 5, c = k & 31;
    float a[8], b[8];
    unpack8(*reinterpret_cast<const uint4*>(feats + (row & 4095) * 256 + c * 8), a);
    unpack8(*reinterpret_cast<const uint4*>(no_mask + c * 8), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += b[e];
    *reinterpret_cast<uint4*>(keys + row * 256 + c * 8) = pack8(a);
  }
}

// ---- sparse tokens -------------------------------------------------------------------------------------------------------------
// One thread per (token, 8 channels): channels 0..127 are sin, 128..255 cos of 2 pi ((2 cx - 1) G[0][f] + (2 cy - 1) G[1][f]) with
// c = (coordinate + 0.5) / frame.  Token t < n is point t (label -1: not_a_point alone; 0 / 1: + point_embeddings[label]); without boxes token
// n is the padding point (not_a_point alone); with boxes tokens n, n + 1 are the corners (+ point_embeddings[2], [3]).
struct TokW { const bf16_t *pe0, *pe1, *pe2, *pe3, *nap; };

__global__ __launch_bounds__(256) void sam_prompt_tokens_kernel(const float* __restrict__ coords, const int32_t* __restrict__ labels, const float* __restrict__ boxes,
                                                               const float* __restrict__ G, TokW W, float frame, int n, int T, long total,
                                                               bf16_t* __restrict__ out) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int c = (int)(k & 31);
  const long row = k >> 5;
  const long i = row / T;
  const int tk = (int)(row - i * T);
  float x = 0.f, y = 0.f;
  const bf16_t* add = nullptr;
  bool alone = false;
  if (tk < n) {
    x = coords[(i * n + tk) * 2];
    y = coords[(i * n + tk) * 2 + 1];
    const int lab = labels[i * n + tk];
    if (lab == -1) { alone = true; add = W.nap; }
    else if (lab == 0) add = W.pe0;
    else if (lab == 1) add = W.pe1;
  } else if (!boxes) {
    alone = true; add = W.nap;
  } else {
    const int j = tk - n;
    x = boxes[i * 4 + 2 * j];
    y = boxes[i * 4 + 2 * j + 1];
    add = j ? W.pe3 : W.pe2;
  }
  float e[8];
  if (alone) {
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = 0.f;
  } else {
    const float cx = 2.f * ((x + 0.5f) / frame) - 1.f, cy = 2.f * ((y + 0.5f) / frame) - 1.f;
    const int f0 = (c & 15) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float arg = 6.283185307179586f * (cx * G[f0 + j] + cy * G[128 + f0 + j]);
      e[j] = c < 16 ? sinf(arg) : cosf(arg);
    }
  }
  if (add) {
    float a[8];
    unpack8(*reinterpret_cast<const uint4*>(add + c * 8), a);
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] += a[j];
  }
  *reinterpret_cast<uint4*>(out + row * 256 + c * 8) = pack8(e);
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline bool al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

}  // namespace

extern "C" int llmseg_sam_dense_prompt(const void* feats, const float* mask, int32_t b, int32_t nested, const void* no_mask, const void* w0, const void* b0,
                                       const void* ln1_w, const void* ln1_b, const void* w3, const void* b3, const void* ln4_w, const void* ln4_b, const void* w6,
                                       const void* b6, void* keys, void* stream) {
  LL_CHECK(feats && keys && b > 0 && b <= 65535 && al16(feats) && al16(keys) && feats != keys, "sam_dense_prompt: feats / keys must be 16-byte aligned, 0 < b <= 65535");
  LL_CHECK(nested == 0 || nested == 1, "sam_dense_prompt: nested must be 0 or 1");
  if (!mask) {
    LL_CHECK(no_mask && al16(no_mask), "sam_dense_prompt: no_mask (16-byte aligned) is required when mask is NULL");
    const long total = (long)b * 4096 * 32;
    const long g = (total + 255) / 256;
    LL_LAUNCH_KERNEL(sam_dense_nomask_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)feats,
                       (const bf16_t*)no_mask, (bf16_t*)keys, total);
    LL_LAUNCH_CHECK("sam_dense_prompt");
    return LLMSEG_OK;
  }
  LL_CHECK(al16(mask), "sam_dense_prompt: mask must be 16-byte aligned");
  LL_CHECK(w0 && b0 && ln1_w && ln1_b && w3 && b3 && ln4_w && ln4_b && w6 && b6, "sam_dense_prompt: the ten mask_downscaling tensors are required with a mask");
  LL_CHECK(al16(w6) && al16(b6), "sam_dense_prompt: mask_downscaling.6 weight / bias must be 16-byte aligned");
  const DenseW W = {(const bf16_t*)w0, (const bf16_t*)b0, (const bf16_t*)ln1_w, (const bf16_t*)ln1_b, (const bf16_t*)w3, (const bf16_t*)b3,
                    (const bf16_t*)ln4_w, (const bf16_t*)ln4_b, (const bf16_t*)w6, (const bf16_t*)b6};
  LL_LAUNCH_KERNEL(sam_dense_prompt_kernel, dim3(4096 / DP_CELLS, (unsigned)b), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)feats, mask, nested, W,
                     (bf16_t*)keys);
  LL_LAUNCH_CHECK("sam_dense_prompt");
  return LLMSEG_OK;
}

extern "C" int llmseg_sam_prompt_tokens(const float* coords, const int32_t* labels, const float* boxes, int32_t b, int32_t n, int32_t frame, const float* gauss,
                                        const void* pe0, const void* pe1, const void* pe2, const void* pe3, const void* not_a_point, void* out, void* stream) {
  LL_CHECK(b > 0 && n >= 0 && frame > 0 && gauss && out && al16(out) && al4(gauss), "sam_prompt_tokens: bad sizes or output");
  LL_CHECK(n == 0 || (coords && labels && al4(coords) && al4(labels)), "sam_prompt_tokens: n > 0 needs coords and labels");
  LL_CHECK(n > 0 || boxes, "sam_prompt_tokens: no points and no boxes");
  LL_CHECK(!boxes || al4(boxes), "sam_prompt_tokens: boxes must be 4-byte aligned");
  LL_CHECK(pe0 && pe1 && pe2 && pe3 && not_a_point && al16(pe0) && al16(pe1) && al16(pe2) && al16(pe3) && al16(not_a_point),
           "sam_prompt_tokens: the four point embeddings and not_a_point must be 16-byte aligned");
  const int T = n + (boxes ? 2 : 1);
  const long total = (long)b * T * 32;
  LL_CHECK((total + 255) / 256 <= 0x7fffffffL, "sam_prompt_tokens: too many tokens");
  const TokW W = {(const bf16_t*)pe0, (const bf16_t*)pe1, (const bf16_t*)pe2, (const bf16_t*)pe3, (const bf16_t*)not_a_point};
  LL_LAUNCH_KERNEL(sam_prompt_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coords, labels, boxes, gauss, W,
                     (float)frame, (int)n, T, total, (bf16_t*)out);
  LL_LAUNCH_CHECK("sam_prompt_tokens");
  return LLMSEG_OK;
}
