// Rank-8 LoRA kernels (peft Linear, r = 8) of the LoRA'd q|k|v projection, forward and backward: the skinny products a 128x128-tile GEMM wastes
// > 90 % of its tile on.  down (per-row and MFMA form, K-slice finish), outer / wgrads (weight gradients), apply (dX of the branches), pack (the
// [*][64] extension operands of the q|k|v GEMM), finish + pack in one launch.  The dropout parameter block (DropP) and LR are in common.h; the
// norm-backward tail that also applies the branches' dX (reduce_lora_normbwd_kernel) is in backward.hip, next to the norm backward it instantiates.
// No mutable file-scope state: what a call does follows from its arguments (and the LLMSEG_LORA_DOWN tuning knob, read once).
#include <algorithm>
#include <cstdlib>
#include "common.h"
#include "llmseg_hip.h"

namespace {

// Two rank-8 down-projections in ONE launch (q and v branches of a LoRA'd q|k|v projection):
//   y[m][0..7] = alpha * drop0(x0)[m][:] . W0^T,   y[m][8..15] = alpha * drop1(x1)[m][:] . W1^T,   y[m][16..16+zero_cols) = 0
// rows of y at pitch ldy (the [M][64] extension operand of the qkv GEMM is [x Aq^T | x Av^T | 0]); x0 == x1 in the forward pass (one
// load feeds both branches, each with its own dropout stream), two column blocks of dY in the backward pass.  w_kr = 0: W stored
// [8][K]; 1: W stored [K][8].  drop(x) = x * mask / (1 - p), mask element index m K + k.  nb = 1 computes the first branch only.
// RW rows per wave: 4 for tall activations (each W chunk is loaded once for four rows), 1 for short ones (M = 2 x 319: four times the
// waves in flight -- the kernel is latency-bound there).
template <int RW>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ x0, const bf16_t* __restrict__ x1, long ldx, const bf16_t* __restrict__ w0,
                                                       const bf16_t* __restrict__ w1, bf16_t* __restrict__ y, long ldy, long M, int K, int w_kr, float alpha,
                                                       int zero_cols, int nb, DropP dp) {
  const int lane = threadIdx.x & 63;
  const long m0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  if (m0 >= M) return;
  float acc[2][RW][LR];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
      for (int r = 0; r < LR; ++r) acc[b][i][r] = 0.f;
  const bool same = x0 == x1;
#pragma unroll 2
  for (int k = lane * 8; k < K; k += 64 * 8) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (b >= nb) break;
      const bf16_t* xb = b == 0 ? x0 : x1;
      const bf16_t* wb = b == 0 ? w0 : w1;
      float xv[RW][8], wv[8];
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const long m = min(m0 + i, M - 1);
        unpack8(*reinterpret_cast<const uint4*>(xb + m * ldx + k), xv[i]);
        if (dp.thr) {
          uint32_t oa;
          const unsigned long di = drop_index(dp, (unsigned long)m, (unsigned long)K, (unsigned long)k, oa);
          dropout8(xv[i], di, dp.stream + b, dp.rng, dp.thr, dp.scale, oa);
        }
      }
      (void)same;
      if (w_kr) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          unpack8(*reinterpret_cast<const uint4*>(wb + (long)(k + j) * LR), wv);
#pragma unroll
          for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int r = 0; r < LR; ++r) acc[b][i][r] += xv[i][j] * wv[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < LR; ++r) {
          unpack8(*reinterpret_cast<const uint4*>(wb + (long)r * K + k), wv);
#pragma unroll
          for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[b][i][r] += xv[i][j] * wv[j];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RW; ++i) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < LR; ++r) acc[b][i][r] = wave_sum(acc[b][i][r]) * alpha;
    if (m0 + i < M) {
      bf16_t* yr = y + (m0 + i) * ldy;
      if (lane == 0) *reinterpret_cast<uint4*>(yr) = pack8(acc[0][i]);
      else if (lane == 1 && nb > 1) *reinterpret_cast<uint4*>(yr + 8) = pack8(acc[1][i]);
      else if (lane >= nb && (lane - nb) * 8 < zero_cols) *reinterpret_cast<uint4*>(yr + lane * 8) = make_uint4(0, 0, 0, 0);
    }
  }
}

// The same product on the matrix cores (W stored [8][K]).  What bounds this product at M = 638 is the operand fetch rate of a CU
// (~16 B/clk): the per-row kernel above spreads over 160 CUs but re-reads both 8 x K weight blocks for every row (82 MB through L2:
// 20 us), a 16-row MFMA tile per workgroup reads every byte once but keeps only 40 CUs busy (20 us again).  So the 16-row tile is
// ALSO split along K over gridDim.y workgroups (320 workgroups at M = 638, K = 4096): a wave's v_mfma_f32_16x16x32_bf16 computes
// D[rank][m] += W[rank][k..k+32] . X[m][k..k+32]^T for the 16 rows (rows 8..15 of the W operand are zero), the 4 waves of a workgroup
// are folded through LDS, and a K-slice's fp32 partial goes to the caller's scratch [slice][M][16]; lora_down_finish_kernel adds the
// slices in order (deterministic), scales and writes the bf16 rows.  With gridDim.y == 1 (tall activations: enough row tiles to fill
// the chip) the first kernel writes the bf16 rows itself.  Dropout: the Philox mask zeroes elements of the bf16 X fragment (exact), the
// 1 / (1 - p) scale is folded into alpha -- no extra rounding.  Branches with different dropout streams need their own MFMA (X differs).
__global__ __launch_bounds__(256) void lora_down_mfma_kernel(const bf16_t* __restrict__ x0, const bf16_t* __restrict__ x1, long ldx, const bf16_t* __restrict__ w0,
                                                            const bf16_t* __restrict__ w1, bf16_t* __restrict__ y, long ldy, long M, int K, float alpha,
                                                            int zero_cols, int nb, DropP dp, float* __restrict__ part) {
  __shared__ float red[4][2][8][16];                   // [wave][branch][rank][row]
  __shared__ float fin[16][16];                        // [row][branch * 8 + rank]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kc = lane >> 4;
  const long m0 = (long)blockIdx.x * 16;
  const long m = min(m0 + r, M - 1);
  const int kq = K / (4 * (int)gridDim.y);             // K-range of one wave (a multiple of 32)
  const int kbeg = ((int)blockIdx.y * 4 + wave) * kq;
  const bool same = x0 == x1;
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  auto masked = [&](uint4 v, unsigned long idx, uint32_t stream, uint32_t off_add) {
    const unsigned long seed = dp.rng[0], off = dp.rng[1] + off_add;
    const Philox8 ph = philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), stream, (uint32_t)off, (uint32_t)seed, (uint32_t)(seed >> 32));
    uint32_t* u = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo = (ph.w[j] & 0xffffu) >= dp.thr ? 0x0000ffffu : 0u, hi = (ph.w[j] >> 16) >= dp.thr ? 0xffff0000u : 0u;
      u[j] &= lo | hi;
    }
    return v;
  };
#pragma unroll 4
  for (int k = kbeg + kc * 8; k < kbeg + kq; k += 32) {
    uint4 xa = *reinterpret_cast<const uint4*>(x0 + m * ldx + k);
    uint4 xb = (nb > 1 && !same) ? *reinterpret_cast<const uint4*>(x1 + m * ldx + k) : xa;
    const uint4 wa = r < LR ? *reinterpret_cast<const uint4*>(w0 + (long)r * K + k) : make_uint4(0, 0, 0, 0);
    const uint4 wb = (nb > 1 && r < LR) ? *reinterpret_cast<const uint4*>(w1 + (long)r * K + k) : make_uint4(0, 0, 0, 0);
    if (dp.thr) {
      uint32_t oa;
      const unsigned long idx = drop_index(dp, (unsigned long)m, (unsigned long)K, (unsigned long)k, oa);
      xa = masked(xa, idx, dp.stream, oa);
      if (nb > 1) xb = masked(xb, idx, dp.stream + 1, oa);
    }
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wa), __builtin_bit_cast(bf16x8_t, xa), acc0, 0, 0, 0);
    if (nb > 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wb), __builtin_bit_cast(bf16x8_t, xb), acc1, 0, 0, 0);
  }
  if (kc < 2) {                                        // acc[e] = D[rank 4 kc + e][row r]
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[wave][0][4 * kc + e][r] = acc0[e]; red[wave][1][4 * kc + e][r] = acc1[e]; }
  }
  __syncthreads();
  {
    const int b = threadIdx.x >> 7, rank = (threadIdx.x >> 4) & 7, mm = threadIdx.x & 15;
    const float sum = (red[0][b][rank][mm] + red[1][b][rank][mm]) + (red[2][b][rank][mm] + red[3][b][rank][mm]);
    if (part) {                                        // K-slice partial: [slice][M][16]
      if (m0 + mm < M) part[((long)blockIdx.y * M + m0 + mm) * 16 + b * 8 + rank] = sum;
    } else fin[mm][b * 8 + rank] = sum * alpha * (dp.thr ? dp.scale : 1.f);
  }
  if (part) return;
  __syncthreads();
  const int nch = nb + zero_cols / 8;                  // 16-byte chunks per output row
  for (int t = threadIdx.x; t < 16 * nch; t += blockDim.x) {
    const int mm = t / nch, ch = t - mm * nch;
    if (m0 + mm >= M) continue;
    uint4 o = make_uint4(0, 0, 0, 0);
    if (ch < nb) o = pack8(&fin[mm][ch * 8]);
    *reinterpret_cast<uint4*>(y + (m0 + mm) * ldy + ch * 8) = o;
  }
}

__device__ __forceinline__ void lora_down_finish_body(const float* __restrict__ part, int S, bf16_t* __restrict__ y, long ldy, long M, float scale,
                                                      int zero_cols, int nb, long bid, long nblocks) {
  const int nch = nb + zero_cols / 8;
  const long total = M * nch;
  for (long t = bid * blockDim.x + threadIdx.x; t < total; t += nblocks * blockDim.x) {
    const long mm = t / nch;
    const int ch = (int)(t - mm * nch);
    uint4 o = make_uint4(0, 0, 0, 0);
    if (ch < nb) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      for (int s2 = 0; s2 < S; ++s2) {
        const float* pp = part + ((long)s2 * M + mm) * 16 + ch * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += pp[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= scale;
      o = pack8(v);
    }
    *reinterpret_cast<uint4*>(y + mm * ldy + ch * 8) = o;
  }
}
__global__ __launch_bounds__(256) void lora_down_finish_kernel(const float* __restrict__ part, int S, bf16_t* __restrict__ y, long ldy, long M, float scale,
                                                              int zero_cols, int nb) {
  lora_down_finish_body(part, S, y, ldy, M, scale, zero_cols, nb, blockIdx.x, gridDim.x);
}

// out(n,r) += alpha * sum_m drop(a)[m][n] * b[m][r]  (the caller zero-fills `out` or accumulates into a gradient arena; no atomics:
// with several row slices a workgroup's 512 sums go to part[slice][branch][N * 8] and fold_slices_kernel adds the slices in order).  out_rn = 0: out [N][8]; 1: out [8][N].  b has row pitch ldb.  blockIdx.z selects one of up to two independent
// products that share the shapes (the q and v branches of one layer: dAq / dAv read the same activation with their own dropout streams,
// dBq / dBv two column blocks of dY).
// Workgroup = 64 columns x one slice of rows, split again over its 4 waves: lane = (row-lane 0..7, column chunk 0..7), a wave reads 8
// rows x 128 contiguous bytes per step (16 B per lane, three steps in flight); the 8 row-lanes are folded with shuffles, the 4 waves in
// LDS, so ONE partial per output cell per workgroup.
// Up to FOUR products per launch (blockIdx.z), each with its own operands, pitches, output layout, scale and dropout stream (drop[z] = 0: no
// mask, else stream id + 1): the whole weight-gradient work of a LoRA'd q|k|v projection -- dBq, dBv, dAq, dAv -- is one launch + one fold.
struct OuterP { const bf16_t* a[4]; const bf16_t* b[4]; float* out[4]; long lda[4], ldb[4]; int out_rn[4]; float alpha[4]; uint32_t drop[4]; };
__global__ __launch_bounds__(256) void lora_outer_kernel(OuterP q, long M, long N, DropP dp, float* __restrict__ part) {
  __shared__ float red[4][8][8 * LR];                  // [wave][column chunk][8 columns x 8 ranks]
  const int z = blockIdx.z;
  const bf16_t* __restrict__ a = q.a[z];
  const bf16_t* __restrict__ b = q.b[z];
  float* __restrict__ out = q.out[z];
  const long lda = q.lda[z], ldb = q.ldb[z];
  const int out_rn = q.out_rn[z];
  const float alpha = q.alpha[z];
  if (q.drop[z] == 0) dp.thr = 0;
  const uint32_t dstream = q.drop[z] - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cl = lane & 7, rl = lane >> 3;
  const long n = ((long)blockIdx.x * 8 + cl) * 8;      // the workgroup's 4 waves cover the SAME 64 columns, each its own quarter of the row slice
  const long per = (M + gridDim.y * 4 - 1) / (gridDim.y * 4);
  const long m0 = ((long)blockIdx.y * 4 + wave) * per, m1 = min(M, m0 + per);
  const bool on = n < N;
  float acc[8][LR];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int r = 0; r < LR; ++r) acc[j][r] = 0.f;
  if (on) {
    long m = m0 + rl;
    for (; m + 16 < m1; m += 24) {
      uint4 av[3], bv[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        av[u] = *reinterpret_cast<const uint4*>(a + (m + 8 * u) * lda + n);
        bv[u] = *reinterpret_cast<const uint4*>(b + (m + 8 * u) * ldb);
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        float x[8], y[8];
        unpack8(av[u], x); unpack8(bv[u], y);
        if (dp.thr) {
          uint32_t oa;
          const unsigned long di = drop_index(dp, (unsigned long)(m + 8 * u), (unsigned long)N, (unsigned long)n, oa);
          dropout8(x, di, dstream, dp.rng, dp.thr, dp.scale, oa);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int r = 0; r < LR; ++r) acc[j][r] = fmaf(x[j], y[r], acc[j][r]);
      }
    }
    for (; m < m1; m += 8) {
      float x[8], y[8];
      unpack8(*reinterpret_cast<const uint4*>(a + m * lda + n), x);
      unpack8(*reinterpret_cast<const uint4*>(b + m * ldb), y);
      if (dp.thr) {
        uint32_t oa;
        const unsigned long di = drop_index(dp, (unsigned long)m, (unsigned long)N, (unsigned long)n, oa);
        dropout8(x, di, dstream, dp.rng, dp.thr, dp.scale, oa);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < LR; ++r) acc[j][r] = fmaf(x[j], y[r], acc[j][r]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int r = 0; r < LR; ++r) {
      float v = acc[j][r];
      v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
      acc[j][r] = v * alpha;
    }
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < LR; ++r) red[wave][cl][j * LR + r] = acc[j][r];
  }
  __syncthreads();
  // 512 outputs (64 columns x 8 ranks) per workgroup: two per thread (row slices of other workgroups hold the other terms of the same cell)
  float* __restrict__ dstp = part ? part + ((long)blockIdx.y * gridDim.z + z) * N * LR : out;
  for (int idx = threadIdx.x; idx < 8 * 8 * LR; idx += blockDim.x) {
    const int c = idx / (8 * LR), jr = idx % (8 * LR), j = jr / LR, r = jr % LR;
    const long nn = ((long)blockIdx.x * 8 + c) * 8 + j;
    if (nn < N) {
      const float v = (red[0][c][jr] + red[1][c][jr]) + (red[2][c][jr] + red[3][c][jr]);
      const long cell = out_rn ? (long)r * N + nn : nn * LR + r;
      if (part) dstp[cell] = v;
      else dstp[cell] += v;
    }
  }
}

// y[m][n..n+7] += alpha * sum over nb branches of mask_b(m, n..) * sum_r xa[m][8 b + r] * W_b(n,r).  w_rn = 0: W stored [N][8]; 1: W
// stored [8][N].  xa row pitch ldxa (branch b reads columns 8 b .. 8 b + 7).  With dropout the product is masked like the forward input
// was (dX of the LoRA branches: ((dq Bq) Aq) * mask_q / (1 - p) + ((dv Bv) Av) * mask_v / (1 - p)) -- one pass over y for both.
__global__ __launch_bounds__(256) void lora_apply_kernel(bf16_t* __restrict__ y, long ldy, const bf16_t* __restrict__ xa, long ldxa,
                                                        const bf16_t* __restrict__ w0, const bf16_t* __restrict__ w1, long M, long N, int w_rn,
                                                        float alpha, int nb, DropP dp) {
  const long nch = N >> 3, total = M * nch;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / nch, c = i % nch;
    float yv[8], wv[8];
    unpack8(*reinterpret_cast<const uint4*>(y + m * ldy + c * 8), yv);
    for (int b = 0; b < nb; ++b) {
      const bf16_t* w = b == 0 ? w0 : w1;
      float xv[8], dv[8];
      unpack8(*reinterpret_cast<const uint4*>(xa + m * ldxa + 8 * b), xv);
      if (w_rn) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dv[j] = 0.f;
#pragma unroll
        for (int r = 0; r < LR; ++r) {
          unpack8(*reinterpret_cast<const uint4*>(w + (long)r * N + c * 8), wv);
#pragma unroll
          for (int j = 0; j < 8; ++j) dv[j] += xv[r] * wv[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          unpack8(*reinterpret_cast<const uint4*>(w + (c * 8 + j) * LR), wv);
          float s = 0.f;
#pragma unroll
          for (int r = 0; r < LR; ++r) s += xv[r] * wv[r];
          dv[j] = s;
        }
      }
      if (dp.thr) {
        uint32_t oa;
        const unsigned long di = drop_index(dp, (unsigned long)m, (unsigned long)N, (unsigned long)(c * 8), oa);     // == i without segments
        dropout8(dv, di, dp.stream + b, dp.rng, dp.thr, dp.scale, oa);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) yv[j] += alpha * dv[j];
    }
    *reinterpret_cast<uint4*>(y + m * ldy + c * 8) = pack8(yv);
  }
}

// The two [*, 64] extension operands of a LoRA'd q|k|v projection (llmseg_gemm_args.A2 / W2), rebuilt from the CURRENT LoRA
// matrices on every call (no cache to go stale when the optimizer updates them in place):
//   w2b [3H][64]: rows of the q block = [s Bq | 0], k block = 0, v block = [0 | s Bv | 0]     (forward: qkv += [xAq | xAv | 0] . w2b^T)
//   w2a [H][64]:  row h = [Aq[:, h] | Av[:, h] | 0]                                             (backward: dx += [tq | tv | 0] . w2a^T)
__device__ __forceinline__ void lora_pack_body(const bf16_t* __restrict__ aq, const bf16_t* __restrict__ bq, const bf16_t* __restrict__ av,
                                               const bf16_t* __restrict__ bv, bf16_t* __restrict__ w2b, bf16_t* __restrict__ w2a, bf16_t* __restrict__ bt,
                                               long H, float s, long bid, long nblocks) {
  const long total = 4 * H * 8 + (bt ? 2 * H : 0);                   // (3H + H) rows x 8 chunks of 8 columns (+ the B^T copies: 16 rows x H / 8 chunks)
  for (long i = bid * blockDim.x + threadIdx.x; i < total; i += nblocks * blockDim.x) {
    if (i >= 4 * H * 8) {                                            // bt [16][H]: rows 0..7 = Bq^T, 8..15 = Bv^T (the backward's rank-8 down projection wants K-contiguous rows)
      const long j = i - 4 * H * 8;
      const int row16 = (int)(j / (H >> 3));
      const long h0 = (j - (long)row16 * (H >> 3)) * 8;
      const bf16_t* src = row16 < 8 ? bq : bv;
      uint32_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (uint32_t)src[(h0 + 2 * e) * LR + (row16 & 7)] | ((uint32_t)src[(h0 + 2 * e + 1) * LR + (row16 & 7)] << 16);
      *reinterpret_cast<uint4*>(bt + (long)row16 * H + h0) = make_uint4(o[0], o[1], o[2], o[3]);
      continue;
    }
    const long row = i >> 3;
    const int ch = (int)(i & 7);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < 3 * H) {
      if (w2b == nullptr) continue;
      if (row < H && ch == 0) { unpack8(*reinterpret_cast<const uint4*>(bq + row * LR), v); }
      else if (row >= 2 * H && ch == 1) { unpack8(*reinterpret_cast<const uint4*>(bv + (row - 2 * H) * LR), v); }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= s;
      *reinterpret_cast<uint4*>(w2b + row * 64 + ch * 8) = pack8(v);
    } else {
      if (w2a == nullptr) continue;
      const long h = row - 3 * H;
      if (ch < 2) {
        const bf16_t* src = ch == 0 ? aq : av;
#pragma unroll
        for (int r = 0; r < LR; ++r) v[r] = bf2f(src[(long)r * H + h]);
      }
      *reinterpret_cast<uint4*>(w2a + h * 64 + ch * 8) = pack8(v);
    }
  }
}
__global__ __launch_bounds__(256) void lora_pack_kernel(const bf16_t* __restrict__ aq, const bf16_t* __restrict__ bq, const bf16_t* __restrict__ av,
                                                       const bf16_t* __restrict__ bv, bf16_t* __restrict__ w2b, bf16_t* __restrict__ w2a, bf16_t* __restrict__ bt,
                                                       long H, float s) {
  lora_pack_body(aq, bq, av, bv, w2b, w2a, bt, H, s, blockIdx.x, gridDim.x);
}
// lora_down's K-slice finish and lora_pack in ONE launch (round 6: the two are independent -- activations vs. weights -- and each is a ~4 us grid-stride pass):
// workgroups [0, gf) add the slices, [gf, gridDim.x) build the extension operands.  Same arithmetic as the two kernels.
__global__ __launch_bounds__(256) void lora_finish_pack_kernel(const float* __restrict__ part, int S, bf16_t* __restrict__ y, long ldy, long M, float scale, int zero_cols,
                                                              int nb, int gf, const bf16_t* __restrict__ aq, const bf16_t* __restrict__ bq,
                                                              const bf16_t* __restrict__ av, const bf16_t* __restrict__ bv, bf16_t* __restrict__ w2b,
                                                              bf16_t* __restrict__ w2a, bf16_t* __restrict__ bt, long H, float s) {
  if ((int)blockIdx.x < gf) lora_down_finish_body(part, S, y, ldy, M, scale, zero_cols, nb, blockIdx.x, gf);
  else lora_pack_body(aq, bq, av, bv, w2b, w2a, bt, H, s, (long)blockIdx.x - gf, (long)gridDim.x - gf);
}

}  // namespace

// What follows the first launch of a down projection; llmseg_lora_down decides it from its arguments before anything is launched.
enum DownTail {
  DOWN_FINISH,          // y is complete on return: lora_down_finish_kernel where the product ran as K slices, nothing more where it did not
  DOWN_PARTS,           // K slices: the fp32 partials stay in `scratch` for llmseg_gemm_args.nb_lora_part, no finish launch
  DOWN_FINISH_PACK,     // K slices: the pack job rides in the finish launch (lora_finish_pack_kernel)
  DOWN_PACK_ALONE       // no K slices, so no finish launch to ride in: the pack job is a launch of its own
};

// -> 0: the per-row kernels (W stored [K][8], or K no multiple of 128); S >= 1: the MFMA form as S K-slices (1: every workgroup writes its y rows itself)
static int lora_down_slices(const llmseg_lora_down_args& a) {
  static const int force = getenv("LLMSEG_LORA_DOWN") ? atoi(getenv("LLMSEG_LORA_DOWN")) : 0;      // tuning / bisecting: 1 = per-row kernel, 2 = MFMA without K slices
  if (a.w_kr || (a.K & 127) != 0 || force == 1) return 0;
  // MFMA form: 16-row tiles; K slices so that the launch has >= ~256 workgroups (each slice a multiple of 4 waves x 32 columns)
  const bool scratch = a.scratch && force != 2;
  const long tiles = (a.M + 15) / 16;
  int S = 1;
  while (tiles * S < 256 && (a.K % (4 * 32 * S * 2)) == 0 && scratch && (int64_t)S * 2 * a.M * 16 * 4 <= a.scratch_bytes && S < 32) S *= 2;
  return S;
}

// scale: the finish factor alpha * dropout scale
static int lora_down_launch(const llmseg_lora_down_args& a, int S, DownTail tail, const DropP& dp, float scale, hipStream_t stream) {
  const int nb = (a.x1 && a.w1) ? 2 : 1, zero_cols = a.zero_cols;
  const long M = a.M, ldx = a.ldx, ldy = a.ldy;
  const bf16_t *X0 = (const bf16_t*)a.x0, *X1 = (const bf16_t*)(a.x1 ? a.x1 : a.x0), *W0 = (const bf16_t*)a.w0, *W1 = (const bf16_t*)(a.w1 ? a.w1 : a.w0);
  bf16_t* y = (bf16_t*)a.y;
  if (S >= 1) {
    float* part = S > 1 ? (float*)a.scratch : nullptr;
    LL_LAUNCH_KERNEL(lora_down_mfma_kernel, dim3((unsigned)((M + 15) / 16), (unsigned)S), dim3(256), 0, stream, X0, X1, ldx, W0, W1, y, ldy, M, (int)a.K, a.alpha,
                     zero_cols, nb, dp, part);
    const unsigned gf = grid_for(M * (nb + zero_cols / 8));
    if (tail == DOWN_FINISH_PACK)
      LL_LAUNCH_KERNEL(lora_finish_pack_kernel, dim3(gf + grid_for(4 * a.pack_H * 8 + 2 * a.pack_H)), dim3(256), 0, stream, (const float*)part, S, y, ldy, M, scale,
                       zero_cols, nb, (int)gf, (const bf16_t*)a.pack_aq, (const bf16_t*)a.pack_bq, (const bf16_t*)a.pack_av, (const bf16_t*)a.pack_bv,
                       (bf16_t*)a.pack_w2b, (bf16_t*)a.pack_w2a, (bf16_t*)a.pack_bt, (long)a.pack_H, a.pack_s);
    else if (tail == DOWN_FINISH && S > 1)
      LL_LAUNCH_KERNEL(lora_down_finish_kernel, dim3(gf), dim3(256), 0, stream, (const float*)part, S, y, ldy, M, scale, zero_cols, nb);
  } else if (M <= 2048)
    LL_LAUNCH_KERNEL(lora_down_kernel<1>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, X0, X1, ldx, W0, W1, y, ldy, M, (int)a.K, a.w_kr, a.alpha, zero_cols,
                     nb, dp);
  else
    LL_LAUNCH_KERNEL(lora_down_kernel<4>, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, stream, X0, X1, ldx, W0, W1, y, ldy, M, (int)a.K, a.w_kr, a.alpha, zero_cols,
                     nb, dp);
  if (tail == DOWN_PACK_ALONE)
    LL_LAUNCH_KERNEL(lora_pack_kernel, dim3(grid_for(4 * a.pack_H * 8 + 2 * a.pack_H)), dim3(256), 0, stream, (const bf16_t*)a.pack_aq, (const bf16_t*)a.pack_bq,
                     (const bf16_t*)a.pack_av, (const bf16_t*)a.pack_bv, (bf16_t*)a.pack_w2b, (bf16_t*)a.pack_w2a, (bf16_t*)a.pack_bt, (long)a.pack_H, a.pack_s);
  LL_LAUNCH_CHECK("lora_down");
  return LLMSEG_OK;
}

extern "C" int llmseg_lora_down(const llmseg_lora_down_args* a, void* stream) {
  LL_CHECK(a && a->struct_size == sizeof(*a), "%s: ABI mismatch: caller's struct_size %u != %zu (bind against include/llmseg_hip.h version %d)",
           "lora_down", a ? a->struct_size : 0u, sizeof(*a), LLMSEG_ABI_VERSION);
  const bool parts = a->parts_S != nullptr, pack = a->pack_aq != nullptr;
  LL_CHECK((!a->parts_S) == (!a->parts_scale), "lora_down: parts_S and parts_scale are both set or both NULL");
  LL_CHECK(!(parts && pack), "lora_down: a call leaves its K-slice partials or carries a pack job, not both");
  const int nb = (a->x1 && a->w1) ? 2 : 1;
  LL_CHECK(a->x0 && a->w0 && a->y && (!a->x1) == (!a->w1) && a->M > 0 && a->K > 0 && (a->K & 7) == 0 && (a->ldx & 7) == 0 && (a->ldy & 7) == 0 &&
               a->ldy >= 8 * nb + a->zero_cols && a->zero_cols >= 0 && (a->zero_cols & 7) == 0 && a->zero_cols <= 480 && AL16(a->x0) && AL16(a->x1) &&
               AL16(a->w0) && AL16(a->w1) && AL16(a->y) && LL_DROP_OK(a->drop),
           "lora_down: bad arguments");
  LL_CHECK(!pack || (a->pack_bq && a->pack_av && a->pack_bv && (a->pack_w2b || a->pack_w2a || a->pack_bt) && a->pack_H > 0 && (a->pack_H & 7) == 0 &&
                     AL16(a->pack_aq) && AL16(a->pack_bq) && AL16(a->pack_av) && AL16(a->pack_bv) && AL16(a->pack_w2b) && AL16(a->pack_w2a) && AL16(a->pack_bt)),
           "lora_down: bad pack arguments");
  const int S = lora_down_slices(*a);
  const DownTail tail = S > 1 ? (parts ? DOWN_PARTS : pack ? DOWN_FINISH_PACK : DOWN_FINISH) : (pack ? DOWN_PACK_ALONE : DOWN_FINISH);
  const DropP dp = make_drop(a->drop);
  const float scale = a->alpha * (dp.thr ? dp.scale : 1.f);
  const int rc = lora_down_launch(*a, S, tail, dp, scale, (hipStream_t)stream);
  if (rc == LLMSEG_OK && parts) {
    *a->parts_S = tail == DOWN_PARTS ? S : 0;
    *a->parts_scale = scale;
  }
  return rc;
}

static int lora_outer_launch(const OuterP& q, int nz, int64_t M, int64_t N, const DropP& dp, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  // 64 columns per workgroup (its 4 waves split the rows): enough row slices to put >= 2 workgroups on every CU, each wave >= 24 rows
  const long colwg = (N + 63) / 64;
  long gy = max(max((long)1, 256 / (colwg * nz)), min((long)32, M / 512));
  gy = min(gy, workspace ? (long)(workspace_bytes / (nz * N * LR * 4)) : 0L);          // row slices the scratch can hold; <= 1: one slice, no scratch
  float* part = gy > 1 ? (float*)workspace : nullptr;
  if (gy < 1) gy = 1;
  LL_LAUNCH_KERNEL(lora_outer_kernel, dim3((unsigned)colwg, (unsigned)gy, (unsigned)nz), dim3(256), 0, stream, q, (long)M, (long)N, dp, part);
  if (part)
    LL_LAUNCH_KERNEL(fold_slices_kernel, dim3(fold_grid(nz * N * LR)), dim3(256), 0, stream, (const float*)part, (int)gy, (long)(nz * N * LR),
                     (long)(nz * N * LR), (long)(N * LR), FoldOut{{q.out[0], q.out[1], q.out[2], q.out[3]}});
  LL_LAUNCH_CHECK("lora_outer");
  return LLMSEG_OK;
}

extern "C" int llmseg_lora_outer(const void* a0, const void* a1, int64_t lda, const void* b0, const void* b1, int64_t ldb, float* out0, float* out1, int64_t M,
                                 int64_t N, int32_t out_rn, float alpha, const llmseg_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream) {
  const int nz = (a1 && b1 && out1) ? 2 : 1;
  LL_CHECK(a0 && b0 && out0 && ((!a1) == (!b1)) && ((!a1) == (!out1)) && M > 0 && N > 0 && (N & 7) == 0 && (lda & 7) == 0 && (ldb & 7) == 0 && AL16(a0) &&
               AL16(a1) && AL16(b0) && AL16(b1) && LL_DROP_OK(drop), "lora_outer: bad arguments (N, lda, ldb multiples of 8)");
  OuterP q{};
  const DropP dp = make_drop(drop);
  for (int z = 0; z < nz; ++z) {
    q.a[z] = (const bf16_t*)(z ? a1 : a0); q.b[z] = (const bf16_t*)(z ? b1 : b0); q.out[z] = z ? out1 : out0;
    q.lda[z] = lda; q.ldb[z] = ldb; q.out_rn[z] = out_rn; q.alpha[z] = alpha; q.drop[z] = dp.thr ? dp.stream + z + 1 : 0;
  }
  return lora_outer_launch(q, nz, M, N, dp, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int llmseg_lora_wgrads(const void* dq, const void* dv, int64_t ldd, const void* x, int64_t ldx, const void* xa, int64_t ldxa, const void* t,
                                  int64_t ldt, float* gbq, float* gbv, float* gaq, float* gav, int64_t M, int64_t H, float s, const llmseg_dropout* drop,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  LL_CHECK(dq && dv && x && xa && t && gbq && gbv && gaq && gav && M > 0 && H > 0 && (H & 7) == 0 && (ldd & 7) == 0 && (ldx & 7) == 0 && (ldxa & 7) == 0 &&
               (ldt & 7) == 0 && ldxa >= 16 && ldt >= 16 && AL16(dq) && AL16(dv) && AL16(x) && AL16(xa) && AL16(t) && LL_DROP_OK(drop),
           "lora_wgrads: bad arguments");
  const DropP dp = make_drop(drop);
  OuterP q{};
  // dBq [H][8] += s dq^T (drop_q(x) Aq^T),  dBv likewise;  dAq [8][H] += (s dq Bq)^T drop_q(x),  dAv likewise (streams: q = drop->stream, v = + 1)
  q.a[0] = (const bf16_t*)dq; q.b[0] = (const bf16_t*)xa;     q.out[0] = gbq; q.lda[0] = ldd; q.ldb[0] = ldxa; q.out_rn[0] = 0; q.alpha[0] = s;   q.drop[0] = 0;
  q.a[1] = (const bf16_t*)dv; q.b[1] = (const bf16_t*)xa + 8; q.out[1] = gbv; q.lda[1] = ldd; q.ldb[1] = ldxa; q.out_rn[1] = 0; q.alpha[1] = s;   q.drop[1] = 0;
  q.a[2] = (const bf16_t*)x;  q.b[2] = (const bf16_t*)t;      q.out[2] = gaq; q.lda[2] = ldx; q.ldb[2] = ldt;  q.out_rn[2] = 1; q.alpha[2] = 1.f; q.drop[2] = dp.thr ? dp.stream + 1 : 0;
  q.a[3] = (const bf16_t*)x;  q.b[3] = (const bf16_t*)t + 8;  q.out[3] = gav; q.lda[3] = ldx; q.ldb[3] = ldt;  q.out_rn[3] = 1; q.alpha[3] = 1.f; q.drop[3] = dp.thr ? dp.stream + 2 : 0;
  return lora_outer_launch(q, 4, M, H, dp, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int llmseg_lora_apply(void* y, int64_t ldy, const void* xa, int64_t ldxa, const void* w0, const void* w1, int64_t M, int64_t N, int32_t w_rn,
                                 float alpha, const llmseg_dropout* drop, void* stream) {
  LL_CHECK(y && xa && w0 && M > 0 && N > 0 && (N & 7) == 0 && (ldy & 7) == 0 && (ldxa & 7) == 0 && ldxa >= (w1 ? 16 : 8) && AL16(y) && AL16(xa) && AL16(w0) &&
               AL16(w1) && LL_DROP_OK(drop), "lora_apply: bad arguments");
  LL_CHECK(!(drop && drop->drop_thr) || ldy == N, "lora_apply: the dropout mask indexes y as a dense [M][N] matrix");
  LL_LAUNCH_KERNEL(lora_apply_kernel, dim3(grid_for(M * (N >> 3))), dim3(256), 0, (hipStream_t)stream, (bf16_t*)y, (long)ldy, (const bf16_t*)xa,
                     (long)ldxa, (const bf16_t*)w0, (const bf16_t*)w1, (long)M, (long)N, w_rn, alpha, w1 ? 2 : 1, make_drop(drop));
  LL_LAUNCH_CHECK("lora_apply");
  return LLMSEG_OK;
}

extern "C" int llmseg_lora_pack(const void* aq, const void* bq, const void* av, const void* bv, void* w2b, void* w2a, void* bt, int64_t H, float s, void* stream) {
  LL_CHECK(aq && bq && av && bv && (w2b || w2a || bt) && H > 0 && (H & 7) == 0 && AL16(aq) && AL16(bq) && AL16(av) && AL16(bv) && AL16(w2b) && AL16(w2a) && AL16(bt),
           "lora_pack: bad arguments");
  LL_LAUNCH_KERNEL(lora_pack_kernel, dim3(grid_for(4 * H * 8 + 2 * H)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)aq, (const bf16_t*)bq, (const bf16_t*)av,
                     (const bf16_t*)bv, (bf16_t*)w2b, (bf16_t*)w2a, (bf16_t*)bt, (long)H, s);
  LL_LAUNCH_CHECK("lora_pack");
  return LLMSEG_OK;
}

// library-internal (gemm.hip: the two-launch route of llmseg_gemm_args.nb_lora_part)
extern "C" __attribute__((visibility("hidden"))) int llmseg_lora_down_finish(const float* part, int S, void* y, int64_t ldy, int64_t M, float scale, int zero_cols, int nb, void* stream) {
  LL_LAUNCH_KERNEL(lora_down_finish_kernel, dim3(grid_for(M * (nb + zero_cols / 8))), dim3(256), 0, (hipStream_t)stream, part, S, (bf16_t*)y, (long)ldy, (long)M, scale,
                     zero_cols, nb);
  LL_LAUNCH_CHECK("lora_down_finish");
  return LLMSEG_OK;
}
