// Quantised weight-only decode (generate(weight_bits=8), generate(weight_format="mxfp4")): the two row quantisers and the skinny GEMMs that stream
// the quantised rows.  The decode step of generation is a weight stream (gemm_skinny_kernel, gemm.hip): HBM-bound, so the only lever is fewer bytes.
//   int8:  a W row [K] bf16 becomes K int8 and one fp32 scale; the model that generation then runs is the one whose matrices are W^ = q * scale.
//   MXFP4: OCP Microscaling FP4, 4-bit E2M1 elements {0, 0.5, 1, 1.5, 2, 3, 4, 6} with a sign, one E8M0 (power-of-two) scale byte per 32 of them, 4.25
//          bits per weight.  W^ = element * 2^e has one mantissa bit: exact in bf16.
// Either way a * w^ (a * q) is exact in fp32 -- the GEMMs' only roundings are their sums'.  The arithmetic is stated bit for bit in include/llmseg_hip.h.
// (gemm_skinny_kernel stays in gemm.hip: scalar accumulators fed by 8 sequential FMAs, A-row transforms, the full epilogue, a double-buffered A -- not this skeleton.)
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
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, __builtin_fabsf(f[e]));      // (the builtin: with a second caller of the device library's fabsf in this
    //                                                                             file, hipcc compiles the sign test of fp4_value below to other instructions)
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

// ---- the GEMMs: C[m][n] = residual[m][n] + sum_k A[m][k] w^[n][k], M <= 8 --------------------------------------------------------------
struct QP {                                            // Q: the packed rows, ldq in bytes; scale: fp32 [N] (int8), uint8 [N][lds] (MXFP4)
  const bf16_t* A; const uint8_t* Q; const void* scale; const bf16_t* res; void* C;
  int M, N, K;
  long lda, ldq, lds, ldc, ldr;
};

__device__ __forceinline__ void store_c(const QP& p, int out_f32, int m, int n, float v) {      // + residual, fp32 or bf16 out
  if (p.res) v += bf2f(p.res[(long)m * p.ldr + n]);
  if (out_f32) reinterpret_cast<float*>(p.C)[(long)m * p.ldc + n] = v;
  else reinterpret_cast<bf16_t*>(p.C)[(long)m * p.ldc + n] = f2bf(v);
}

__device__ __forceinline__ uint32_t dword(const uint4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// What differs between the formats of the weight stream below: W weights in a 16-byte chunk (byte_offset: where column k of a packed row lies), what
// travels with a chunk (MXFP4: its block's E8M0 scale byte; int8: nothing, the row has one fp32 scale for the finished sum), the K-steps of a trip, the
// row counts instantiated (the powers of two up to ROWS), and `fma_trip`: the chunks of a trip (per K-step one of each of the 4 weight rows) against the
// W columns x[t][m][..] of the MT rows of A.  Every accumulator acc[r][m] takes its (even k, odd k) pairs in ascending order; in which order the FMAs of DIFFERENT accumulators are
// written moves no bit but decides registers (the other format's order costs int8 at 4 rows 132 VGPRs for 128, MXFP4 at 2 rows 84 for 80, an
// occupancy step each) and the schedule, so each format keeps the loop it was measured with.  `fma_trip` is plain `inline`, called from the kernel's
// `compute` lambda: always-inlined, the int8 instances come out in another instruction order (profiles/decode_gemm_refactor.md).
struct I8 {
  static constexpr int W = 16, ROWS = 8;
  static constexpr bool BLOCK_SCALE = false;
  struct scale_t {};
  static constexpr int ks(int MT, bool SK) { return (MT >= 4 || SK) ? 1 : 2; }
  static __device__ __forceinline__ int byte_offset(int k) { return k; }
  // a weight costs one conversion: a sign-extending byte select feeding v_cvt_f32_i32
  template <int KS, int MT>
  static __device__ inline void fma_trip(const uint4 (&w)[KS][4], const scale_t (&)[KS][4], const uint4 (&x)[KS][MT][2], f32x2_t (&acc)[4][MT]) {
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {                    // dword j of the chunk: weights 4 j .. 4 j + 3 of every row, as two (even, odd) pairs
        f32x2_t wf[4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int32_t d = (int32_t)dword(w[t][r], j);
          wf[r][0] = f32x2_t{(float)(int8_t)d, (float)(int8_t)(d >> 8)};
          wf[r][1] = f32x2_t{(float)(int8_t)(d >> 16), (float)(d >> 24)};
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const uint32_t a0 = dword(x[t][m][j >> 1], 2 * (j & 1)), a1 = dword(x[t][m][j >> 1], 2 * (j & 1) + 1);
          const f32x2_t af0 = {__uint_as_float(a0 << 16), __uint_as_float(a0 & 0xffff0000u)};
          const f32x2_t af1 = {__uint_as_float(a1 << 16), __uint_as_float(a1 & 0xffff0000u)};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[r][m] = __builtin_elementwise_fma(wf[r][0], af0, acc[r][m]);
            acc[r][m] = __builtin_elementwise_fma(wf[r][1], af1, acc[r][m]);
          }
        }
      }
  }
};
struct MXFP4 {
  static constexpr int W = 32, ROWS = 2;               // from 3 rows on the product runs on the matrix cores (below)
  static constexpr bool BLOCK_SCALE = true;
  typedef uint32_t scale_t;
  static constexpr int ks(int, bool) { return 1; }
  static __device__ __forceinline__ int byte_offset(int k) { return k >> 1; }
  // a byte of two elements becomes two fp32 with the block's scale applied by ONE v_cvt_scalef32_pk_f32_fp4 (low nibble first; the scale operand is
  // the fp32 2^e, bits byte << 23)
  template <int KS, int MT>
  static __device__ inline void fma_trip(const uint4 (&w)[KS][4], const scale_t (&s)[KS][4], const uint4 (&x)[KS][MT][4], f32x2_t (&acc)[4][MT]) {
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      float sc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = __uint_as_float(s[t][r] << 23);
#pragma unroll
      for (int j = 0; j < 4; ++j) {                    // dword j of the chunk: weights 8 j .. 8 j + 7 of every row, as four (even, odd) pairs
        f32x2_t wf[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t d = dword(w[t][r], j);
          wf[r][0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 0);
          wf[r][1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 1);
          wf[r][2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 2);
          wf[r][3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d, sc[r], 3);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int b = 0; b < 4; ++b) {                // byte b of the dword against dword b of A's chunk j: columns 8 j + 2 b, + 1
            const uint32_t a = dword(x[t][m][j], b);
            const f32x2_t af = {__uint_as_float(a << 16), __uint_as_float(a & 0xffff0000u)};
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r][m] = __builtin_elementwise_fma(wf[r][b], af, acc[r][m]);
          }
      }
    }
  }
};

// ---- one to ROWS rows: a weight stream on the vector ALU --------------------------------------------------------------------------------
// gemm_skinny_kernel's structure on fewer bytes: a wave owns 4 consecutive packed rows, its 64 lanes walk K in 16-byte chunks -- W weights (64 W
// columns per row per instruction: 1024 int8, 2048 MXFP4) against W / 8 16-byte A chunks per A row -- with the weight (and scale-byte) loads of the
// next trip issued before the FMAs of this one, fp32 accumulators, a butterfly at the end; lane (r, m) applies the int8 row scale ONCE, adds the
// residual and stores.  The FMA count per weight is the row count: the accumulators are pairs (even k, odd k) updated by packed FMAs
// (v_pk_fma_f32), in ascending pair order within a chunk and ascending chunk order within a trip.  (Measured, profiles/w8_decode.md: unpacked FMAs
// are no slower at any row count; at 8 rows the kernels take as long as the bf16 one -- hence the matrix cores for MXFP4, profiles/mxfp4_decode.md.)
// SK (few rows over a long K: N <= 8192 at K >= 4 trips): the 4 waves of a workgroup share 4 rows and interleave the trips, as the bf16 kernel's do.
// Tails are branch-free: past the end of K a valid chunk is re-read against zeroed A; rows clamp to N - 1 / M - 1 and are not stored.
template <class F, int MT, bool SK>
__global__ __launch_bounds__(256) void gemm_stream_kernel(QP p, int out_f32) {
  constexpr int KS = F::ks(MT, SK);                  // K-steps (64 W columns) per trip
  constexpr int W = F::W, AC = W / 8;                // A chunks per weight chunk
  constexpr int STEP = KS * 64 * W;                  // (tests/w8_checks.py, tests/mxfp4_checks.py: STEP)
  constexpr int ADV = SK ? 4 * STEP : STEP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = SK ? blockIdx.x * 4 : (blockIdx.x * 4 + wave) * 4;
  if (n0 >= p.N) return;
  const uint8_t *qr[4], *sr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long n = min(n0 + r, p.N - 1);
    qr[r] = p.Q + n * p.ldq;
    if constexpr (F::BLOCK_SCALE) sr[r] = reinterpret_cast<const uint8_t*>(p.scale) + n * p.lds;
  }
  f32x2_t acc[4][MT];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = f32x2_t{0.f, 0.f};
  const int K = p.K;
  using scale_t = typename F::scale_t;
  auto loadw = [&](uint4 (&w)[KS][4], scale_t (&s)[KS][4], int k) {
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int kc = min(k + t * 64 * W, K - W);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        w[t][r] = *reinterpret_cast<const uint4*>(qr[r] + F::byte_offset(kc));
        if constexpr (F::BLOCK_SCALE) s[t][r] = sr[r][kc >> 5];
      }
    }
  };
  auto loadx = [&](uint4 (&x)[KS][MT][AC], int k) {
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int kk = k + t * 64 * W, kc = min(kk, K - W);
      const bool ok = kk < K;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const bf16_t* ar = p.A + (long)min(m, p.M - 1) * p.lda + kc;
#pragma unroll
        for (int h = 0; h < AC; ++h) {
          const uint4 v = *reinterpret_cast<const uint4*>(ar + 8 * h);
          x[t][m][h] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
        }
      }
    }
  };
  auto compute = [&](const uint4 (&w)[KS][4], const scale_t (&s)[KS][4], const uint4 (&x)[KS][MT][AC]) { F::template fma_trip<KS, MT>(w, s, x, acc); };
  uint4 wA[KS][4], wB[KS][4], xA[KS][MT][AC];
  scale_t sA[KS][4], sB[KS][4];
  int k = lane * W + (SK ? wave * STEP : 0);
  loadw(wA, sA, k);
  const int trips_all = (K + STEP - 1) / STEP;
  const int trips = SK ? (trips_all - wave + 3) / 4 : trips_all;          // wave-uniform
  for (int t = 0; t < trips; t += 2) {                // A chunks (cache hits) single-buffered, requested ahead of the next packed rows
    loadx(xA, k);                                     // (loads return in order: a later request would wait for the prefetch)
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
      if constexpr (!F::BLOCK_SCALE) mine *= reinterpret_cast<const float*>(p.scale)[n];
      store_c(p, out_f32, m, n, mine);
    }
  }
}

// ---- MXFP4, three rows and more: the same product on the matrix cores -----------------------------------------------------------------
// Every wave of the FMA kernel above reads all M rows of A for its 4 weight rows and spends M FMAs per weight: with more rows that, not the weight
// bytes, is its time (at 8 rows it took as long as the int8 and the bf16 kernel; profiles/mxfp4_decode.md).  Here a wave owns 16 weight rows and its
// unit of work is 128 columns = 4 scale blocks, one per 16-lane quarter q: lane (r, q) loads the 16 bytes of block 4 u + q of weight row r, its scale byte and the block's 32 columns of A row r (zero for
// r >= M), and dword i of the weights against A's chunk i is one v_mfma_f32_16x16x32_bf16 -- the instruction sums over (quarter, element), and which
// column sits in which slot is free as long as both operands agree.  v_cvt_scalef32_pk_bf16_fp4 turns a byte into two bf16 with the scale applied:
// w^ is exact in bf16, the products are exact in fp32, the sums are the instruction's fp32 sums.  A costs 16 bytes per lane per MFMA whatever M is.
// The NW waves of a workgroup take the units in turn (wave v: v, v + NW, ...) and add their tiles through LDS in a fixed tree; NW = 16 where N alone
// would leave SIMDs empty.  Tails as above: a clamped block against zeroed A.
constexpr int FP4_MFMA_ROWS = MXFP4::ROWS + 1;         // measured, profiles/mxfp4_decode.md
constexpr int FP4_UNIT = 128;                          // columns of a wave's unit (tests/mxfp4_checks.py: UNIT)

template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_mxfp4_mfma_kernel(QP p, int out_f32) {
  __shared__ f32x4_t red[NW][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const long n = min(n0 + r, p.N - 1);
  const uint8_t* qr = p.Q + n * p.ldq;
  const uint8_t* sr = reinterpret_cast<const uint8_t*>(p.scale) + n * p.lds;
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
      if (nn < p.N) store_c(p, out_f32, r, nn, t[0][i]);
    }
  }
}

// ---- host side: one argument check, one launch of the stream kernel ------------------------------------------------------------------
// a: llmseg_gemm_w8_args or llmseg_gemm_mxfp4_args (the first has no lds: its caller passes 0).  The format sets the K granule (a chunk's W columns),
// the bytes of a packed row (16 per chunk) and the scale bytes of a row (one per 32 columns, or none); the checked arguments become the kernels' QP.
template <class F, class Args>
int gemm_params(const char* name, const Args* a, int64_t lds, QP& p) {
  LL_CHECK(a && a->struct_size == sizeof(*a), "%s: ABI mismatch: caller's struct_size %u != %zu (bind against include/llmseg_hip.h version %d)", name,
           a ? a->struct_size : 0u, sizeof(*a), LLMSEG_ABI_VERSION);
  LL_CHECK(a->A && a->Q && a->scale && a->C, "%s: null pointer", name);
  LL_CHECK(a->M >= 1 && a->M <= 8 && a->N >= 1 && a->N <= 0x7ffffff0L && a->K >= F::W && a->K <= 0x3fffffffL && a->K % F::W == 0,
           "%s: need 1 <= M <= 8, N >= 1, K >= %d with K %% %d == 0 (M = %ld, N = %ld, K = %ld)", name, F::W, F::W, (long)a->M, (long)a->N, (long)a->K);
  const int64_t ldq_min = a->K * 16 / F::W, lds_min = F::BLOCK_SCALE ? a->K / 32 : 0;      // bytes of a packed row, scale bytes of a row
  LL_CHECK(a->lda >= a->K && a->lda % 8 == 0 && a->ldq >= ldq_min && a->ldq % 16 == 0 && lds >= lds_min && AL16(a->A) && AL16(a->Q),
           F::BLOCK_SCALE ? "%s: rows of A and Q must be 16-byte aligned (lda %% 8, ldq %% 16 == 0) with lda >= K, ldq >= K / 2, lds >= K / 32"
                          : "%s: rows of A and q must be 16-byte aligned (lda %% 8, ldq %% 16 == 0) and ld >= K", name);
  LL_CHECK(a->ldc >= a->N && (!a->residual || a->ldr >= a->N), "%s: ldc / ldr < N", name);
  p.A = (const bf16_t*)a->A; p.Q = (const uint8_t*)a->Q; p.scale = a->scale; p.res = (const bf16_t*)a->residual; p.C = a->C;
  p.M = (int)a->M; p.N = (int)a->N; p.K = (int)a->K;
  p.lda = a->lda; p.ldq = a->ldq; p.lds = lds; p.ldc = a->ldc; p.ldr = a->ldr;
  return LLMSEG_OK;
}

template <class F, bool SK>
auto stream_kernel(int M) -> void (*)(QP, int) {      // the instance for M <= F::ROWS rows: 1, 2 (, 4, 8)
  if (M == 1) return gemm_stream_kernel<F, 1, SK>;
  if constexpr (F::ROWS >= 8)
    if (M > 2) return M <= 4 ? gemm_stream_kernel<F, 4, SK> : gemm_stream_kernel<F, 8, SK>;
  return gemm_stream_kernel<F, 2, SK>;
}

template <class F>
int launch_stream(const char* name, const QP& p, int out_f32, void* stream) {
  // fewer rows than fill the machine over a long K (4 trips of 64 W columns: 4096 int8, 8192 MXFP4): the workgroup's waves split K instead
  const bool sk = p.N <= 8192 && p.K >= 4 * F::ks(1, true) * 64 * F::W;
  const auto kernel = sk ? stream_kernel<F, true>(p.M) : stream_kernel<F, false>(p.M);
  LL_LAUNCH_KERNEL(kernel, dim3((unsigned)(sk ? (p.N + 3) / 4 : (p.N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, p, out_f32);
  LL_LAUNCH_CHECK(name);
  return LLMSEG_OK;
}

}  // namespace

extern "C" int llmseg_quantize_rows_i8(const void* w, int64_t ldw, int64_t N, int64_t K, void* q, int64_t ldq, float* scale, void* w_hat, int64_t ldh,
                                       void* stream) {
  LL_CHECK(w && q && scale, "quantize_rows_i8: null pointer");
  LL_CHECK(N >= 1 && N <= 0x7fffffffL && K >= 16 && K <= 0x3fffffffL && K % 16 == 0, "quantize_rows_i8: need N >= 1 and K >= 16 with K %% 16 == 0 (N = %ld, K = %ld)", (long)N, (long)K);
  LL_CHECK(ldw >= K && ldw % 8 == 0 && ldq >= K && ldq % 16 == 0 && AL16(w) && AL16(q), "quantize_rows_i8: rows must be 16-byte aligned (ldw %% 8, ldq %% 16 == 0) and ld >= K");
  LL_CHECK(!w_hat || (ldh >= K && ldh % 8 == 0 && AL16(w_hat)), "quantize_rows_i8: w_hat rows must be 16-byte aligned with ldh >= K");
  LL_LAUNCH_KERNEL(quantize_rows_i8_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (long)ldw, (int)K, (int8_t*)q, (long)ldq, scale,
                   (bf16_t*)w_hat, (long)ldh);
  LL_LAUNCH_CHECK("quantize_rows_i8");
  return LLMSEG_OK;
}

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

extern "C" int llmseg_gemm_w8(const llmseg_gemm_w8_args* a, void* stream) {
  QP p;
  if (const int e = gemm_params<I8>("gemm_w8", a, 0, p)) return e;
  return launch_stream<I8>("gemm_w8", p, a->out_f32 ? 1 : 0, stream);
}

extern "C" int llmseg_gemm_mxfp4(const llmseg_gemm_mxfp4_args* a, void* stream) {
  QP p;
  if (const int e = gemm_params<MXFP4>("gemm_mxfp4", a, a ? a->lds : 0, p)) return e;
  if (p.M < FP4_MFMA_ROWS) return launch_stream<MXFP4>("gemm_mxfp4", p, a->out_f32 ? 1 : 0, stream);
  if (p.N <= 8192) LL_LAUNCH_KERNEL(gemm_mxfp4_mfma_kernel<16>, dim3((unsigned)((p.N + 15) / 16)), dim3(1024), 0, (hipStream_t)stream, p, a->out_f32 ? 1 : 0);
  else LL_LAUNCH_KERNEL(gemm_mxfp4_mfma_kernel<4>, dim3((unsigned)((p.N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, p, a->out_f32 ? 1 : 0);
  LL_LAUNCH_CHECK("gemm_mxfp4");
  return LLMSEG_OK;
}
