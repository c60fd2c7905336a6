// int8 weight-only decode (generate(weight_bits=8)): a per-row quantiser and the skinny GEMM that streams the quantised rows.
// The decode step of generation is a weight stream (gemm_skinny_kernel, gemm.hip): HBM-bound, so the only lever is fewer bytes.  A W row
// [K] bf16 becomes K int8 and one fp32 scale; the model that generation then runs is the one whose matrices are W^ = q * scale.
#include "common.h"

namespace {

// ---- llmseg_quantize_rows_i8: one workgroup per row of W [N][ldw] bf16 ---------------------------------------------------------------
// amax = max_k |w|, scale = amax / 127, inv = 127 / amax (0 for an all-zero row; both divisions IEEE), q = clamp(rint(w * inv), +-127)
// (the product rounded once, ties to even), w^ = bf16_rne(q * scale).  Pass 1 reads the row for amax, pass 2 reads it again (from L2: a
// row is at most 22 KiB) and writes q and, when asked, w^: the prefill operand costs no third read of W.
__global__ __launch_bounds__(256) void quantize_rows_i8_kernel(const bf16_t* __restrict__ w, long ldw, int K, int8_t* __restrict__ q, long ldq,
                                                               float* __restrict__ scale, bf16_t* __restrict__ w_hat, long ldh) {
  __shared__ float red[16];
  const long n = blockIdx.x;
  const bf16_t* wr = w + n * ldw;
  float amax = 0.f, f[16];
  for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
    unpack8(*reinterpret_cast<const uint4*>(wr + k), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
  }
  amax = block_max(amax, red);
  const float sc = __fdiv_rn(amax, 127.0f), inv = amax > 0.f ? __fdiv_rn(127.0f, amax) : 0.f;
  if (threadIdx.x == 0) scale[n] = sc;
  for (int k = threadIdx.x * 16; k < K; k += 256 * 16) {
    unpack8(*reinterpret_cast<const uint4*>(wr + k), f);
    unpack8(*reinterpret_cast<const uint4*>(wr + k + 8), f + 8);
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
    float h[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float r = fminf(fmaxf(rintf(__fmul_rn(f[e], inv)), -127.f), 127.f);
      pk[e >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (e & 3));
      h[e] = __fmul_rn(r, sc);
    }
    *reinterpret_cast<uint4*>(q + n * ldq + k) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    if (w_hat) {
      *reinterpret_cast<uint4*>(w_hat + n * ldh + k) = pack8(h);
      *reinterpret_cast<uint4*>(w_hat + n * ldh + k + 8) = pack8(h + 8);
    }
  }
}

// ---- llmseg_gemm_w8: C[m][n] = residual[m][n] + scale[n] * sum_k A[m][k] q[n][k], M <= 8 ---------------------------------------------
// gemm_skinny_kernel's structure on half the bytes: a wave owns 4 consecutive q rows, its 64 lanes walk K in 16-byte chunks -- now 16
// weights (1024 columns per row per instruction) against two 16-byte A chunks per A row -- with the loads of the next trip issued before
// the FMAs of this one, fp32 accumulators, a butterfly at the end; lane (r, m) applies the scale ONCE, adds the residual and stores.  a * q
// is exact in fp32 (8 + 7 significant bits), so the only roundings are the accumulation's.  The FMA count per weight is the row count:
// the accumulators are pairs (even k, odd k) updated by packed FMAs (v_pk_fma_f32), and a weight costs one conversion (a sign-extending
// byte select feeding v_cvt_f32_i32).  (Measured, profiles/w8_decode.md: unpacked FMAs are no slower at any row count; at 8 rows the
// kernel takes as long as the bf16 one.)
// SK (few q rows: N <= 8192 at K >= 4096): the 4 waves of a workgroup share 4 rows and interleave the trips, as the bf16 kernel's do.
// Tails are branch-free: past the end of K a valid chunk is re-read against zeroed A; rows clamp to N - 1 / M - 1 and are not stored.
struct W8P {
  const bf16_t* A; const int8_t* Q; const float* scale; const bf16_t* res; void* C;
  int M, N, K;
  long lda, ldq, ldc, ldr;
};

template <int MT, bool SK>
__global__ __launch_bounds__(256) void gemm_w8_kernel(W8P p, int out_f32) {
  constexpr int KS = (MT >= 4 || SK) ? 1 : 2;        // K-steps (1024 columns) per trip
  constexpr int STEP = KS * 1024;
  constexpr int ADV = SK ? 4 * STEP : STEP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = SK ? blockIdx.x * 4 : (blockIdx.x * 4 + wave) * 4;
  if (n0 >= p.N) return;
  const int8_t* qr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) qr[r] = p.Q + (long)min(n0 + r, p.N - 1) * p.ldq;
  f32x2_t acc[4][MT];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = f32x2_t{0.f, 0.f};
  const int K = p.K;
  auto loadw = [&](uint4 (&w)[KS][4], int k) {
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) w[t][r] = *reinterpret_cast<const uint4*>(qr[r] + min(k + t * 1024, K - 16));
  };
  auto loadx = [&](uint4 (&x)[KS][MT][2], int k) {
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int kk = k + t * 1024, kc = min(kk, K - 16);
      const bool ok = kk < K;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const bf16_t* ar = p.A + (long)min(m, p.M - 1) * p.lda + kc;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4 v = *reinterpret_cast<const uint4*>(ar + 8 * h);
          x[t][m][h] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
        }
      }
    }
  };
  auto word = [](const uint4& v, int j) -> uint32_t { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; };
  auto compute = [&](const uint4 (&w)[KS][4], const uint4 (&x)[KS][MT][2]) {
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {                    // dword j of the chunk: weights 4 j .. 4 j + 3 of every row, as two (even, odd) pairs
        f32x2_t wf[4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int32_t d = (int32_t)word(w[t][r], j);
          wf[r][0] = f32x2_t{(float)(int8_t)d, (float)(int8_t)(d >> 8)};
          wf[r][1] = f32x2_t{(float)(int8_t)(d >> 16), (float)(d >> 24)};
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const uint32_t a0 = word(x[t][m][j >> 1], 2 * (j & 1)), a1 = word(x[t][m][j >> 1], 2 * (j & 1) + 1);
          const f32x2_t af0 = {__uint_as_float(a0 << 16), __uint_as_float(a0 & 0xffff0000u)};
          const f32x2_t af1 = {__uint_as_float(a1 << 16), __uint_as_float(a1 & 0xffff0000u)};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[r][m] = __builtin_elementwise_fma(wf[r][0], af0, acc[r][m]);
            acc[r][m] = __builtin_elementwise_fma(wf[r][1], af1, acc[r][m]);
          }
        }
      }
  };
  uint4 wA[KS][4], wB[KS][4], xA[KS][MT][2];
  int k = lane * 16 + (SK ? wave * STEP : 0);
  loadw(wA, k);
  const int trips_all = (K + STEP - 1) / STEP;
  const int trips = SK ? (trips_all - wave + 3) / 4 : trips_all;          // wave-uniform
  for (int t = 0; t < trips; t += 2) {                // A chunks (cache hits) single-buffered, requested ahead of the next q rows
    loadx(xA, k);                                     // (loads return in order: a later request would wait for the prefetch)
    loadw(wB, k + ADV);
    compute(wA, xA);
    k += ADV;
    if (t + 1 >= trips) break;
    loadx(xA, k);
    loadw(wA, k + ADV);
    compute(wB, xA);
    k += ADV;
  }
  float mine = 0.f;                                   // lane r * MT + m keeps C[m][n0 + r]
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float t = wave_sum(acc[r][m].x + acc[r][m].y);
      if (lane == r * MT + m) mine = t;
    }
  if constexpr (SK) {
    __shared__ float red[4][4 * MT];
    if (lane < 4 * MT) red[wave][lane] = mine;
    __syncthreads();
    if (wave != 0) return;
    if (lane < 4 * MT) mine = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  }
  if (lane < 4 * MT) {
    const int r = lane / MT, m = lane - r * MT, n = n0 + r;
    if (n < p.N && m < p.M) {
      float v = mine * p.scale[n];
      if (p.res) v += bf2f(p.res[(long)m * p.ldr + n]);
      if (out_f32) reinterpret_cast<float*>(p.C)[(long)m * p.ldc + n] = v;
      else reinterpret_cast<bf16_t*>(p.C)[(long)m * p.ldc + n] = f2bf(v);
    }
  }
}

#define LL_W8_4(SK) {gemm_w8_kernel<1, SK>, gemm_w8_kernel<2, SK>, gemm_w8_kernel<4, SK>, gemm_w8_kernel<8, SK>}
void (*const w8_kernel[2][4])(W8P, int) = {LL_W8_4(false), LL_W8_4(true)};      // [K split among the waves][rows 1, 2, 4, 8]
#undef LL_W8_4

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int llmseg_quantize_rows_i8(const void* w, int64_t ldw, int64_t N, int64_t K, void* q, int64_t ldq, float* scale, void* w_hat, int64_t ldh,
                                       void* stream) {
  LL_CHECK(w && q && scale, "quantize_rows_i8: null pointer");
  LL_CHECK(N >= 1 && N <= 0x7fffffffL && K >= 16 && K <= 0x3fffffffL && K % 16 == 0, "quantize_rows_i8: need N >= 1 and K >= 16 with K %% 16 == 0 (N = %ld, K = %ld)", (long)N, (long)K);
  LL_CHECK(ldw >= K && ldw % 8 == 0 && ldq >= K && ldq % 16 == 0 && aligned16(w) && aligned16(q), "quantize_rows_i8: rows must be 16-byte aligned (ldw %% 8, ldq %% 16 == 0) and ld >= K");
  LL_CHECK(!w_hat || (ldh >= K && ldh % 8 == 0 && aligned16(w_hat)), "quantize_rows_i8: w_hat rows must be 16-byte aligned with ldh >= K");
  LL_LAUNCH_KERNEL(quantize_rows_i8_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (long)ldw, (int)K, (int8_t*)q, (long)ldq, scale,
                   (bf16_t*)w_hat, (long)ldh);
  LL_LAUNCH_CHECK("quantize_rows_i8");
  return LLMSEG_OK;
}

extern "C" int llmseg_gemm_w8(const llmseg_gemm_w8_args* a, void* stream) {
  LL_CHECK(a && a->struct_size == sizeof(*a), "%s: ABI mismatch: caller's struct_size %u != %zu (bind against include/llmseg_hip.h version %d)",
           "gemm_w8", a ? a->struct_size : 0u, sizeof(*a), LLMSEG_ABI_VERSION);
  LL_CHECK(a->A && a->Q && a->scale && a->C, "gemm_w8: null pointer");
  LL_CHECK(a->M >= 1 && a->M <= 8 && a->N >= 1 && a->N <= 0x7ffffff0L && a->K >= 16 && a->K <= 0x3fffffffL && a->K % 16 == 0,
           "gemm_w8: need 1 <= M <= 8, N >= 1, K >= 16 with K %% 16 == 0 (M = %ld, N = %ld, K = %ld)", (long)a->M, (long)a->N, (long)a->K);
  LL_CHECK(a->lda >= a->K && a->lda % 8 == 0 && a->ldq >= a->K && a->ldq % 16 == 0 && aligned16(a->A) && aligned16(a->Q),
           "gemm_w8: rows of A and q must be 16-byte aligned (lda %% 8, ldq %% 16 == 0) and ld >= K");
  LL_CHECK(a->ldc >= a->N && (!a->residual || a->ldr >= a->N), "gemm_w8: ldc / ldr < N");
  W8P p;
  p.A = (const bf16_t*)a->A; p.Q = (const int8_t*)a->Q; p.scale = a->scale; p.res = (const bf16_t*)a->residual; p.C = a->C;
  p.M = (int)a->M; p.N = (int)a->N; p.K = (int)a->K;
  p.lda = a->lda; p.ldq = a->ldq; p.ldc = a->ldc; p.ldr = a->ldr;
  const bool sk = a->N <= 8192 && a->K >= 4096;      // fewer than 2 waves per SIMD otherwise: the workgroup's waves split K instead
  const int ti = a->M == 1 ? 0 : a->M == 2 ? 1 : a->M <= 4 ? 2 : 3;
  LL_LAUNCH_KERNEL(w8_kernel[sk][ti], dim3((unsigned)(sk ? (a->N + 3) / 4 : (a->N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, p, a->out_f32 ? 1 : 0);
  LL_LAUNCH_CHECK("gemm_w8");
  return LLMSEG_OK;
}
