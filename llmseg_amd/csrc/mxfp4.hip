// MXFP4 weight-only decode (generate(weight_format="mxfp4")): the per-32-block quantiser and the skinny GEMM that streams the packed rows.
// OCP Microscaling FP4: 4-bit E2M1 elements {0, 0.5, 1, 1.5, 2, 3, 4, 6} with a sign, one E8M0 (power-of-two) scale byte per 32 of them, 4.25 bits
// per weight.  W^ = element * 2^e has one mantissa bit: exact in bf16, and a * w^ is exact in fp32 -- the GEMM's only roundings are its sums'.
// The arithmetic is stated bit for bit in include/llmseg_hip.h.
#include "common.h"

namespace {

// ---- llmseg_quantize_rows_mxfp4: one workgroup per row of W [N][ldw] bf16, FOUR lanes per block of 32 columns ------------------------
// A lane loads 16 bytes (8 weights); the block's amax is two xor-shuffles away (K % 32 == 0: the four lanes of a block are in the loop together).
// The scale is integer work on amax's bf16 bits: byte = max(0, E - 2 + (mantissa > 0x40)) for the biased exponent E (0 for zero and
// denormal amax).  x = |w| * 2^-e is exact; the code is the number of the seven thresholds x passes (`>` where the tie goes down to an even code,
// `>=` where it goes up to one).  The lane stores its 4 packed bytes, its 8 w^ and, as lane 0 of the block, the scale byte.
__device__ __forceinline__ uint32_t fp4_code(float w, float inv) {
  const float x = fabsf(w) * inv;
  const uint32_t c = (uint32_t)(x > 0.25f) + (uint32_t)(x >= 0.75f) + (uint32_t)(x > 1.25f) + (uint32_t)(x >= 1.75f) + (uint32_t)(x > 2.5f) + (uint32_t)(x >= 3.5f) +
                     (uint32_t)(x > 5.0f);
  return c ? c | ((__float_as_uint(w) >> 28) & 8u) : 0u;
}
// the value of a 4-bit code: codes 2 .. 7 are (1 + m / 2) * 2^(ex - 1), fp32 bits (code << 22) + 0x3f000000
__device__ __forceinline__ float fp4_value(uint32_t code) {
  const uint32_t c = code & 7u;
  const float v = c >= 2u ? __uint_as_float((c << 22) + 0x3f000000u) : c ? 0.5f : 0.f;
  return (code & 8u) ? -v : v;
}

__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(const bf16_t* __restrict__ w, long ldw, int K, uint8_t* __restrict__ packed, long ldq,
                                                                  uint8_t* __restrict__ scale, long lds, bf16_t* __restrict__ w_hat, long ldh) {
  const long n = blockIdx.x;
  const bf16_t* wr = w + n * ldw;
  for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(wr + k);
    // |bf16| bits order like the values: the integer maximum is amax
    uint32_t am = max(max(max(v.x & 0x7fffu, (v.x >> 16) & 0x7fffu), max(v.y & 0x7fffu, (v.y >> 16) & 0x7fffu)),
                      max(max(v.z & 0x7fffu, (v.z >> 16) & 0x7fffu), max(v.w & 0x7fffu, (v.w >> 16) & 0x7fffu)));
    am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
    am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
    const int E = (int)(am >> 7), byte = E ? max(0, E - 2 + (int)((am & 0x7fu) > 0x40u)) : 0;
    const float inv = __uint_as_float((uint32_t)(254 - byte) << 23);          // 2^-e, a normal fp32 for every byte 0 .. 253
    float f[8], h[8];
    unpack8(v, f);
    uint32_t pk = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t c = fp4_code(f[e], inv);
      pk |= c << (4 * e);
      h[e] = ldexpf(fp4_value(c), byte - 127);
    }
    *reinterpret_cast<uint32_t*>(packed + n * ldq + (k >> 1)) = pk;
    if ((threadIdx.x & 3) == 0) scale[n * lds + (k >> 5)] = (uint8_t)byte;
    if (w_hat) *reinterpret_cast<uint4*>(w_hat + n * ldh + k) = pack8(h);
  }
}

// ---- llmseg_gemm_mxfp4: C[m][n] = residual[m][n] + sum_k A[m][k] w^[n][k], M <= 8 ----------------------------------------------------
// One and two rows (MT = 1, 2): a weight stream on the vector ALU.
// gemm_w8_kernel's structure (quant.hip) on half its bytes: a wave owns 4 consecutive packed rows, its 64 lanes walk K in 16-byte chunks -- now 32
// weights, exactly one scale block, 2048 columns per row per instruction -- against four 16-byte A chunks per A row, with the weight and scale
// loads of the next trip issued before the FMAs of this one, fp32 accumulators, a butterfly at the end; lane (r, m) adds the residual and stores.
// A byte of two elements becomes two fp32 with the block's scale applied by ONE v_cvt_scalef32_pk_f32_fp4 (low nibble first; the scale
// operand is the fp32 2^e, bits byte << 23); the accumulators are (even k, odd k) pairs updated by packed FMAs, as the int8 kernel's are.
// SK (few rows over a long K: N <= 8192 at K >= 8192): the 4 waves of a workgroup share 4 rows and interleave the trips.
// Tails are branch-free: past the end of K a valid chunk is re-read against zeroed A; rows clamp to N - 1 / M - 1 and are not stored.
struct FP4P {
  const bf16_t* A; const uint8_t* Q; const uint8_t* scale; const bf16_t* res; void* C;
  int M, N, K;
  long lda, ldq, lds, ldc, ldr;
};

constexpr int FP4_MFMA_ROWS = 3;                       // from this many rows on the product runs on the matrix cores (below); measured, profiles/mxfp4_decode.md
constexpr int FP4_STEP = 2048;                         // columns of a wave's trip (tests/mxfp4_checks.py: STEP)

template <int MT, bool SK>
__global__ __launch_bounds__(256) void gemm_mxfp4_kernel(FP4P p, int out_f32) {
  constexpr int ADV = SK ? 4 * FP4_STEP : FP4_STEP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = SK ? blockIdx.x * 4 : (blockIdx.x * 4 + wave) * 4;
  if (n0 >= p.N) return;
  const uint8_t *qr[4], *sr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long n = min(n0 + r, p.N - 1);
    qr[r] = p.Q + n * p.ldq;
    sr[r] = p.scale + n * p.lds;
  }
  f32x2_t acc[4][MT];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = f32x2_t{0.f, 0.f};
  const int K = p.K;
  auto loadw = [&](uint4 (&w)[4], uint32_t (&s)[4], int k) {
    const int kc = min(k, K - 32);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      w[r] = *reinterpret_cast<const uint4*>(qr[r] + (kc >> 1));
      s[r] = sr[r][kc >> 5];
    }
  };
  auto loadx = [&](uint4 (&x)[MT][4], int k) {
    const int kc = min(k, K - 32);
    const bool ok = k < K;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const bf16_t* ar = p.A + (long)min(m, p.M - 1) * p.lda + kc;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const uint4 v = *reinterpret_cast<const uint4*>(ar + 8 * h);
        x[m][h] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
      }
    }
  };
  auto word = [](const uint4& v, int j) -> uint32_t { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; };
  auto compute = [&](const uint4 (&w)[4], const uint32_t (&s)[4], const uint4 (&x)[MT][4]) {
    float sc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = __uint_as_float(s[r] << 23);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                      // dword j of the chunk: weights 8 j .. 8 j + 7 of every row, as four (even, odd) pairs
      f32x2_t wf[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t d = word(w[r], j);
        wf[r][0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 0);
        wf[r][1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 1);
        wf[r][2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 2);
        wf[r][3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 3);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int b = 0; b < 4; ++b) {                  // byte b of the dword against dword b of A's chunk j: columns 8 j + 2 b, + 1
          const uint32_t a = word(x[m][j], b);
          const f32x2_t af = {__uint_as_float(a << 16), __uint_as_float(a & 0xffff0000u)};
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r][m] = __builtin_elementwise_fma(wf[r][b], af, acc[r][m]);
        }
    }
  };
  uint4 wA[4], wB[4], xA[MT][4];
  uint32_t sA[4], sB[4];
  int k = lane * 32 + (SK ? wave * FP4_STEP : 0);
  loadw(wA, sA, k);
  const int trips_all = (K + FP4_STEP - 1) / FP4_STEP;
  const int trips = SK ? (trips_all - wave + 3) / 4 : trips_all;          // wave-uniform
  for (int t = 0; t < trips; t += 2) {                // A chunks (cache hits) single-buffered, requested ahead of the next packed rows
    loadx(xA, k);
    loadw(wB, sB, k + ADV);
    compute(wA, sA, xA);
    k += ADV;
    if (t + 1 >= trips) break;
    loadx(xA, k);
    loadw(wA, sA, k + ADV);
    compute(wB, sB, xA);
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
      float v = mine;
      if (p.res) v += bf2f(p.res[(long)m * p.ldr + n]);
      if (out_f32) reinterpret_cast<float*>(p.C)[(long)m * p.ldc + n] = v;
      else reinterpret_cast<bf16_t*>(p.C)[(long)m * p.ldc + n] = f2bf(v);
    }
  }
}

// ---- three rows and more: the same product on the matrix cores ------------------------------------------------------------------------
// Every wave of the FMA kernel above reads all M rows of A for its 4 weight rows and spends M FMAs per weight: with more rows that, not the weight
// bytes, is its time (at 8 rows it took as long as the int8 and the bf16 kernel; profiles/mxfp4_decode.md).  Here a wave owns 16 weight rows and its
// unit of work is 128 columns = 4 scale blocks, one per 16-lane quarter q: lane (r, q) loads the 16 bytes of block 4 u + q of weight row r, its scale byte and the block's 32 columns of A row r (zero for
// r >= M), and dword i of the weights against A's chunk i is one v_mfma_f32_16x16x32_bf16 -- the instruction sums over (quarter, element), and which
// column sits in which slot is free as long as both operands agree.  v_cvt_scalef32_pk_bf16_fp4 turns a byte into two bf16 with the scale applied:
// w^ is exact in bf16, the products are exact in fp32, the sums are the instruction's fp32 sums.  A costs 16 bytes per lane per MFMA whatever M is.
// The NW waves of a workgroup take the units in turn (wave v: v, v + NW, ...) and add their tiles through LDS in a fixed tree; NW = 16 where N alone
// would leave SIMDs empty.  Tails as above: a clamped block against zeroed A.
constexpr int FP4_UNIT = 128;                          // columns of a wave's unit (tests/mxfp4_checks.py: UNIT)

template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_mxfp4_mfma_kernel(FP4P p, int out_f32) {
  __shared__ f32x4_t red[NW][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const long n = min(n0 + r, p.N - 1);
  const uint8_t* qr = p.Q + n * p.ldq;
  const uint8_t* sr = p.scale + n * p.lds;
  const bf16_t* ar = p.A + (long)min(r, p.M - 1) * p.lda;
  const bool arow = r < p.M;
  const int nb = p.K >> 5;                             // scale blocks of a row
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](uint4& w, uint32_t& s, uint4 (&x)[4], int u) {
    const int b = 4 * u + q, bc = min(b, nb - 1);
    const bool ok = arow && b < nb;
    w = *reinterpret_cast<const uint4*>(qr + (long)bc * 16);
    s = sr[bc];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint4 v = *reinterpret_cast<const uint4*>(ar + (long)bc * 32 + 8 * i);
      x[i] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
    }
  };
  auto compute = [&](const uint4& w, uint32_t s, const uint4 (&x)[4]) {
    const float sc = __uint_as_float(s << 23);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t d = i == 0 ? w.x : i == 1 ? w.y : i == 2 ? w.z : w.w;
      const bf16x2_t c0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0), c1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1);
      const bf16x2_t c2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2), c3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3);
      const bf16x8_t wf = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y, c3.x, c3.y};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8_t, x[i]), acc, 0, 0, 0);
    }
  };
  const int units = (p.K + FP4_UNIT - 1) / FP4_UNIT;
  const int mine = (units - wave + NW - 1) / NW;      // wave-uniform, may be 0
  uint4 wA, wB, xA[4], xB[4];
  uint32_t sA, sB;
  int u = wave;
  if (mine > 0) load(wA, sA, xA, u);
  for (int t = 0; t < mine; t += 2) {
    load(wB, sB, xB, u + NW);                          // one unit ahead; past the end it is a clamped block against zeroed A, never used
    compute(wA, sA, xA);
    u += NW;
    if (t + 1 >= mine) break;
    load(wA, sA, xA, u + NW);
    compute(wB, sB, xB);
    u += NW;
  }
  red[wave][lane] = acc;                               // lane (m, q) holds C[m][n0 + 4 q + i], i = 0 .. 3
  __syncthreads();
  if (wave != 0) return;
  f32x4_t t[NW / 4];
#pragma unroll
  for (int g = 0; g < NW / 4; ++g) t[g] = (red[4 * g][lane] + red[4 * g + 1][lane]) + (red[4 * g + 2][lane] + red[4 * g + 3][lane]);
  if constexpr (NW == 16) t[0] = (t[0] + t[1]) + (t[2] + t[3]);
  if (r < p.M) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nn = n0 + 4 * q + i;
      if (nn < p.N) {
        float v = t[0][i];
        if (p.res) v += bf2f(p.res[(long)r * p.ldr + nn]);
        if (out_f32) reinterpret_cast<float*>(p.C)[(long)r * p.ldc + nn] = v;
        else reinterpret_cast<bf16_t*>(p.C)[(long)r * p.ldc + nn] = f2bf(v);
      }
    }
  }
}

void (*const mxfp4_kernel[2][2])(FP4P, int) = {{gemm_mxfp4_kernel<1, false>, gemm_mxfp4_kernel<2, false>},
                                               {gemm_mxfp4_kernel<1, true>, gemm_mxfp4_kernel<2, true>}};      // [K split among the waves][rows 1, 2]

}  // namespace

extern "C" int llmseg_quantize_rows_mxfp4(const void* w, int64_t ldw, int64_t N, int64_t K, void* packed, int64_t ldq, void* scale, int64_t lds, void* w_hat,
                                          int64_t ldh, void* stream) {
  LL_CHECK(w && packed && scale, "quantize_rows_mxfp4: null pointer");
  LL_CHECK(N >= 1 && N <= 0x7fffffffL && K >= 32 && K <= 0x3fffffffL && K % 32 == 0, "quantize_rows_mxfp4: need N >= 1 and K >= 32 with K %% 32 == 0 (N = %ld, K = %ld)", (long)N,
           (long)K);
  LL_CHECK(ldw >= K && ldw % 8 == 0 && ldq >= K / 2 && ldq % 16 == 0 && lds >= K / 32 && AL16(w) && AL16(packed),
           "quantize_rows_mxfp4: rows must be 16-byte aligned (ldw %% 8, ldq %% 16 == 0) with ldw >= K, ldq >= K / 2, lds >= K / 32");
  LL_CHECK(!w_hat || (ldh >= K && ldh % 8 == 0 && AL16(w_hat)), "quantize_rows_mxfp4: w_hat rows must be 16-byte aligned with ldh >= K");
  LL_LAUNCH_KERNEL(quantize_rows_mxfp4_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (long)ldw, (int)K, (uint8_t*)packed, (long)ldq,
                   (uint8_t*)scale, (long)lds, (bf16_t*)w_hat, (long)ldh);
  LL_LAUNCH_CHECK("quantize_rows_mxfp4");
  return LLMSEG_OK;
}

extern "C" int llmseg_gemm_mxfp4(const llmseg_gemm_mxfp4_args* a, void* stream) {
  LL_CHECK(a && a->struct_size == sizeof(*a), "%s: ABI mismatch: caller's struct_size %u != %zu (bind against include/llmseg_hip.h version %d)",
           "gemm_mxfp4", a ? a->struct_size : 0u, sizeof(*a), LLMSEG_ABI_VERSION);
  LL_CHECK(a->A && a->Q && a->scale && a->C, "gemm_mxfp4: null pointer");
  LL_CHECK(a->M >= 1 && a->M <= 8 && a->N >= 1 && a->N <= 0x7ffffff0L && a->K >= 32 && a->K <= 0x3fffffffL && a->K % 32 == 0,
           "gemm_mxfp4: need 1 <= M <= 8, N >= 1, K >= 32 with K %% 32 == 0 (M = %ld, N = %ld, K = %ld)", (long)a->M, (long)a->N, (long)a->K);
  LL_CHECK(a->lda >= a->K && a->lda % 8 == 0 && a->ldq >= a->K / 2 && a->ldq % 16 == 0 && a->lds >= a->K / 32 && AL16(a->A) && AL16(a->Q),
           "gemm_mxfp4: rows of A and Q must be 16-byte aligned (lda %% 8, ldq %% 16 == 0) with lda >= K, ldq >= K / 2, lds >= K / 32");
  LL_CHECK(a->ldc >= a->N && (!a->residual || a->ldr >= a->N), "gemm_mxfp4: ldc / ldr < N");
  FP4P p;
  p.A = (const bf16_t*)a->A; p.Q = (const uint8_t*)a->Q; p.scale = (const uint8_t*)a->scale; p.res = (const bf16_t*)a->residual; p.C = a->C;
  p.M = (int)a->M; p.N = (int)a->N; p.K = (int)a->K;
  p.lda = a->lda; p.ldq = a->ldq; p.lds = a->lds; p.ldc = a->ldc; p.ldr = a->ldr;
  if (a->M >= FP4_MFMA_ROWS) {
    if (a->N <= 8192) LL_LAUNCH_KERNEL(gemm_mxfp4_mfma_kernel<16>, dim3((unsigned)((a->N + 15) / 16)), dim3(1024), 0, (hipStream_t)stream, p, a->out_f32 ? 1 : 0);
    else LL_LAUNCH_KERNEL(gemm_mxfp4_mfma_kernel<4>, dim3((unsigned)((a->N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, p, a->out_f32 ? 1 : 0);
    LL_LAUNCH_CHECK("gemm_mxfp4");
    return LLMSEG_OK;
  }
  const bool sk = a->N <= 8192 && a->K >= 8192;      // a trip is 2048 columns: fewer rows than fill the machine over a long K, the workgroup's waves split K
  LL_LAUNCH_KERNEL(mxfp4_kernel[sk][a->M - 1], dim3((unsigned)(sk ? (a->N + 3) / 4 : (a->N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, p, a->out_f32 ? 1 : 0);
  LL_LAUNCH_CHECK("gemm_mxfp4");
  return LLMSEG_OK;
}
