// Backward-pass and optimizer kernels for the trainable part of the LLM-Seg hot path (LoRA'd Llama stack, embed/lm_head,
// text_hidden_fcs, mask-selection head).  All HBM-bound streaming kernels; GEMM-shaped gradients go through
// llmseg_gemm_bf16 with trans_a / trans_w.  See include/llmseg_hip.h for the reference ops each one differentiates.
// The rank-8 LoRA kernels are in lora.hip; the norm backward's K-slice tail that also applies their dX (reduce_lora_normbwd_kernel) is here.
#include <algorithm>
#include <cstdlib>
#include "common.h"
#include "llmseg_hip.h"

namespace {

// out[n] += sum_m x[m][n]   (bias gradients); block = 64 columns x 4 row-lanes, grid.y splits the rows.  part != NULL: the row slice's
// sum goes to part[slice][N] (folded in slice order by fold_slices_kernel); part == NULL (one slice): the column's only writer adds it.
__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, float* __restrict__ part, long M, long N, long ld) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const long col = (long)blockIdx.x * 64 + c;
  const long rows_per = (M + gridDim.y - 1) / gridDim.y;
  const long r0 = (long)blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  float s = 0.f;
  if (col < N)
    for (long r = r0 + rl; r < r1; r += 4) s += bf2f(x[r * ld + col]);
  red[rl][c] = s;
  __syncthreads();
  if (rl == 0 && col < N) {
    const float v = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    if (part) part[(long)blockIdx.y * N + col] = v;
    else out[col] += v;
  }
}

// LayerNorm / RMSNorm backward, one wave per row.  CPL > 0: x and dy (<= 64*CPL 16-byte chunks per row) are read once and kept
// in registers; CPL == 0: multi-pass fallback.  Weight / bias gradients (fp32, dw may be NULL), no atomics (fixed summation order):
// ACC = true (narrow rows, CPL <= 2) walks rows grid-stride with per-lane register partial sums, folds the workgroup's 4 waves in LDS
// and writes ONE partial per column per workgroup to part[workgroup][2][cols] (fold_slices_kernel adds them in workgroup order; a
// single workgroup adds to dw / db itself); ACC = false (wide rows) stores the row's (mean, rstd) to `stats` and leaves the column
// sums to norm_dwdb_kernel.
template <int CPL, bool ACC>
__global__ __launch_bounds__(256, 2) void norm_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                         bf16_t* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db, long rows, int cols,
                                                         float eps, int rms, const bf16_t* __restrict__ dres, float* __restrict__ part,
                                                         float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int nch = cols >> 3;
  constexpr int NR = CPL > 0 ? CPL : 1;
  float aw[ACC ? NR : 1][8], ab[ACC ? NR : 1][8];
  if constexpr (ACC) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) { aw[i][e] = 0.f; ab[i][e] = 0.f; }
  }
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {
    const bf16_t* xr = x + row * cols;
    const bf16_t* gr = dy + row * cols;
    uint4 xc[NR], gc[NR];
    if constexpr (CPL > 0) {
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int c = lane + 64 * i;
        const bool on = c < nch;
        xc[i] = on ? *reinterpret_cast<const uint4*>(xr + c * 8) : make_uint4(0, 0, 0, 0);
        gc[i] = on ? *reinterpret_cast<const uint4*>(gr + c * 8) : make_uint4(0, 0, 0, 0);
      }
    }
    // the body sees chunk index c, cache slot i and the cached / freshly loaded 16-byte pieces xv (x) and gv (dy)
#define LL_FOR_CHUNKS(...)                                                                       \
  if constexpr (CPL > 0) {                                                                       \
    _Pragma("unroll") for (int i = 0; i < NR; ++i) {                                             \
      const int c = lane + 64 * i;                                                               \
      if (c < nch) { const uint4 xv = xc[i], gv = gc[i]; __VA_ARGS__ }                           \
    }                                                                                            \
  } else {                                                                                       \
    for (int c = lane; c < nch; c += 64) {                                                       \
      constexpr int i = 0;                                                                       \
      const uint4 xv = *reinterpret_cast<const uint4*>(xr + c * 8), gv = *reinterpret_cast<const uint4*>(gr + c * 8); \
      __VA_ARGS__                                                                                \
    }                                                                                            \
  }
    float f[8], g[8], ww[8];
    float s = 0.f;
    if (!rms) {
      LL_FOR_CHUNKS({ (void)gv; (void)i; unpack8(xv, f); _Pragma("unroll") for (int e = 0; e < 8; ++e) s += f[e]; })
      s = wave_sum(s);
    }
    const float mean = rms ? 0.f : s / (float)cols;
    float v = 0.f;
    LL_FOR_CHUNKS({ (void)gv; (void)i; unpack8(xv, f); _Pragma("unroll") for (int e = 0; e < 8; ++e) { const float d = f[e] - mean; v += d * d; } })
    v = wave_sum(v);
    const float rstd = rsqrtf(v / (float)cols + eps);
    if constexpr (!ACC) { if (stats && lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; } }
    // c1 = mean(g), c2 = mean(g * xhat) with g = dy * w
    float c1 = 0.f, c2 = 0.f;
    LL_FOR_CHUNKS({
      (void)i;
      unpack8(xv, f); unpack8(gv, g);
      unpack8(*reinterpret_cast<const uint4*>(w + c * 8), ww);
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {
        const float xh = (f[e] - mean) * rstd, gg = g[e] * ww[e];
        c1 += gg; c2 += gg * xh;
      }
    })
    c1 = wave_sum(c1) / (float)cols; c2 = wave_sum(c2) / (float)cols;
    if (rms) c1 = 0.f;
    LL_FOR_CHUNKS({
      float o[8];
      unpack8(xv, f); unpack8(gv, g);
      unpack8(*reinterpret_cast<const uint4*>(w + c * 8), ww);
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {
        const float xh = (f[e] - mean) * rstd;
        o[e] = rstd * (g[e] * ww[e] - c1 - xh * c2);
        if constexpr (ACC) { aw[i][e] += g[e] * xh; ab[i][e] += g[e]; }
      }
      if (dres) {                                            // + the gradient that reaches x through the residual connection
        float rr[8];
        unpack8(*reinterpret_cast<const uint4*>(dres + row * cols + c * 8), rr);
        _Pragma("unroll") for (int e = 0; e < 8; ++e) o[e] += rr[e];
      }
      *reinterpret_cast<uint4*>(dx + row * cols + c * 8) = pack8(o);
    })
#undef LL_FOR_CHUNKS
  }
  if constexpr (ACC) {
    // fold the workgroup's 4 waves in LDS, then ONE partial per column per workgroup
    __shared__ float red[2][4][NR * 64 * 8];
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[0][wv][(i * 64 + lane) * 8 + e] = aw[i][e];
        red[1][wv][(i * 64 + lane) * 8 + e] = ab[i][e];
      }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NR * 64 * 8; idx += blockDim.x) {
      const int i = idx / (64 * 8), ln = (idx / 8) % 64, e = idx % 8;
      const int c = ln + 64 * i;
      if (c < nch) {
        const float sw = (red[0][0][idx] + red[0][1][idx]) + (red[0][2][idx] + red[0][3][idx]);
        const float sb = (red[1][0][idx] + red[1][1][idx]) + (red[1][2][idx] + red[1][3][idx]);
        if (part) {
          part[((long)blockIdx.x * 2 + 0) * cols + c * 8 + e] = sw;
          part[((long)blockIdx.x * 2 + 1) * cols + c * 8 + e] = sb;
        } else {
          if (dw) dw[c * 8 + e] += sw;
          if (db) db[c * 8 + e] += sb;
        }
      }
    }
  }
}

// Norm backward for a FROZEN weight (no dw / db) with a WORKGROUP per row: short, wide activations (Llama at two images per step: 638 rows x
// 4096 columns) leave most of the chip idle with one wave per row (14 us for 21 MB); 4 waves per row keep 4 x the loads in flight.
// the row arithmetic of norm_bwd_wg_kernel, shared with the fused split-K tail (reduce_lora_normbwd_kernel) so that both produce the same bits:
// xc / gc / wc = this thread's 8-element chunks (c = thread + 256 i) of x, dy and the norm weight; writes dx = norm backward + dres
template <int CPT>
__device__ __forceinline__ void normbwd_row(const uint4 (&xc)[CPT], const uint4 (&gc)[CPT], const uint4 (&wc)[CPT], float* red, bf16_t* __restrict__ dx, long row,
                                            int cols, float eps, int rms, const bf16_t* __restrict__ dres) {
  const int nch = cols >> 3;
  float f[8], g[8], ww[8];
  float s = 0.f;
  if (!rms) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) { unpack8(xc[i], f); _Pragma("unroll") for (int e = 0; e < 8; ++e) s += f[e]; }
    s = block_sum(s, red);
  }
  const float mean = rms ? 0.f : s / (float)cols;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i)
    if (threadIdx.x + 256 * i < nch) { unpack8(xc[i], f); _Pragma("unroll") for (int e = 0; e < 8; ++e) { const float d = f[e] - mean; v += d * d; } }
  v = block_sum(v, red);
  const float rstd = rsqrtf(v / (float)cols + eps);
  float c1 = 0.f, c2 = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i)
    if (threadIdx.x + 256 * i < nch) {
      unpack8(xc[i], f); unpack8(gc[i], g); unpack8(wc[i], ww);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float xh = (f[e] - mean) * rstd, gg = g[e] * ww[e]; c1 += gg; c2 += gg * xh; }
    }
  c1 = rms ? 0.f : block_sum(c1, red) / (float)cols;
  c2 = block_sum(c2, red) / (float)cols;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = threadIdx.x + 256 * i;
    if (c < nch) {
      float o[8];
      unpack8(xc[i], f); unpack8(gc[i], g); unpack8(wc[i], ww);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float xh = (f[e] - mean) * rstd; o[e] = rstd * (g[e] * ww[e] - c1 - xh * c2); }
      if (dres) {
        float rr[8];
        unpack8(*reinterpret_cast<const uint4*>(dres + row * cols + c * 8), rr);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += rr[e];
      }
      *reinterpret_cast<uint4*>(dx + row * cols + c * 8) = pack8(o);
    }
  }
}

template <int CPT>
__global__ __launch_bounds__(256) void norm_bwd_wg_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                         bf16_t* __restrict__ dx, long rows, int cols, float eps, int rms, const bf16_t* __restrict__ dres) {
  __shared__ float red[16];
  const long row = blockIdx.x;
  const int nch = cols >> 3;
  const bf16_t* xr = x + row * cols;
  const bf16_t* gr = dy + row * cols;
  uint4 xc[CPT], gc[CPT], wc[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = threadIdx.x + 256 * i;
    const bool on = c < nch;
    xc[i] = on ? *reinterpret_cast<const uint4*>(xr + c * 8) : make_uint4(0, 0, 0, 0);
    gc[i] = on ? *reinterpret_cast<const uint4*>(gr + c * 8) : make_uint4(0, 0, 0, 0);
    wc[i] = on ? *reinterpret_cast<const uint4*>(w + c * 8) : make_uint4(0, 0, 0, 0);
  }
  normbwd_row<CPT>(xc, gc, wc, red, dx, row, cols, eps, rms, dres);
}

// Column sums of a wide norm's backward from the stored row statistics: dw[c] = sum_r dy[r][c] (x[r][c] - mean_r) rstd_r, db[c] = sum_r dy[r][c].
// Block = 64 columns x 4 row-lanes, grid.y = row slices -> part[slice][2][cols] (slices folded in order), or straight into dw / db for one slice.
__global__ __launch_bounds__(256) void norm_dwdb_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ stats,
                                                       float* __restrict__ dw, float* __restrict__ db, float* __restrict__ part, long rows, long cols) {
  __shared__ float red[2][4][64];
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const long col = (long)blockIdx.x * 64 + c;
  const long rows_per = (rows + gridDim.y - 1) / gridDim.y;
  const long r0 = (long)blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
  float sw = 0.f, sb = 0.f;
  if (col < cols)
    for (long r = r0 + rl; r < r1; r += 4) {
      const float g = bf2f(dy[r * cols + col]);
      sw += g * (bf2f(x[r * cols + col]) - stats[2 * r]) * stats[2 * r + 1];
      sb += g;
    }
  red[0][rl][c] = sw; red[1][rl][c] = sb;
  __syncthreads();
  if (rl == 0 && col < cols) {
    const float vw = (red[0][0][c] + red[0][1][c]) + (red[0][2][c] + red[0][3][c]);
    const float vb = (red[1][0][c] + red[1][1][c]) + (red[1][2][c] + red[1][3][c]);
    if (part) { part[((long)blockIdx.y * 2 + 0) * cols + col] = vw; part[((long)blockIdx.y * 2 + 1) * cols + col] = vb; }
    else { if (dw) dw[col] += vw; if (db) db[col] += vb; }
  }
}

// d_gu[r][c] = d_out * up * silu'(gate), d_gu[r][I+c] = d_out * silu(gate)
// dout rows have stride ld_dout; dout may ALIAS the up half of dgu's rows (the two-launch route of the GEMM's fused swiglu-backward epilogue): every
// thread reads its own 8 elements of dout before it overwrites them, so no restrict on those two
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const bf16_t* __restrict__ gu, const bf16_t* dout, bf16_t* dgu,
                                                        long rows, long I, long ld_dout) {
  const long ich = I >> 3, total = rows * ich;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / ich, c = i % ich;
    float g[8], u[8], d[8], og[8], ou[8];
    unpack8(*reinterpret_cast<const uint4*>(gu + row * 2 * I + c * 8), g);
    unpack8(*reinterpret_cast<const uint4*>(gu + row * 2 * I + I + c * 8), u);
    unpack8(*reinterpret_cast<const uint4*>(dout + row * ld_dout + c * 8), d);
#pragma unroll
    for (int e = 0; e < 8; ++e) swiglu_bwd1(d[e], g[e], u[e], og[e], ou[e]);
    *reinterpret_cast<uint4*>(dgu + row * 2 * I + c * 8) = pack8(og);
    *reinterpret_cast<uint4*>(dgu + row * 2 * I + I + c * 8) = pack8(ou);
  }
}

// dpre = dy * f'(y) from the OUTPUT y: relu -> (y > 0), sigmoid -> y (1 - y)
__global__ __launch_bounds__(256) void act_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y, bf16_t* __restrict__ out, long n, int act) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float g = bf2f(dy[i]), yy = bf2f(y[i]);
    out[i] = f2bf(act == LLMSEG_ACT_RELU ? (yy > 0.f ? g : 0.f) : g * yy * (1.f - yy));
  }
}

// P[b][q][k] = softmax_k(scale * S[b][q][k] + mask), one wave per (b, q) row; columns >= T are written as zero
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, bf16_t* __restrict__ P, long BH, int Tq, int T, int ld,
                                                          float scale, int causal, const uint8_t* __restrict__ key_mask, int heads) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= BH * Tq) return;
  const long bh = row / Tq;
  const int q = (int)(row % Tq);
  const float* s = S + row * ld;
  bf16_t* p = P + row * ld;
  const uint8_t* km = key_mask ? key_mask + (bh / heads) * T : nullptr;
  float mx = -1e30f;
  for (int k = lane; k < T; k += 64) {
    const bool ok = (!causal || k <= q) && (!km || km[k]);
    if (ok) mx = fmaxf(mx, s[k] * scale);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < T; k += 64) {
    const bool ok = (!causal || k <= q) && (!km || km[k]);
    if (ok) sum += __expf(s[k] * scale - mx);
  }
  sum = wave_sum(sum);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  for (int k = lane; k < ld; k += 64) {
    const bool ok = k < T && (!causal || k <= q) && (!km || km[k]);
    p[k] = f2bf(ok ? __expf(s[k] * scale - mx) * inv : 0.f);
  }
}

// dS = scale * P * (dP - sum_k P dP), one wave per row; pad columns written as zero
__global__ __launch_bounds__(256) void attn_ds_kernel(const bf16_t* __restrict__ P, const float* __restrict__ dP, bf16_t* __restrict__ dS, long rows, int T,
                                                     int ld, float scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* p = P + row * ld;
  const float* d = dP + row * ld;
  float dl = 0.f;
  for (int k = lane; k < T; k += 64) dl += bf2f(p[k]) * d[k];
  dl = wave_sum(dl);
  for (int k = lane; k < ld; k += 64) dS[row * ld + k] = f2bf(k < T ? scale * bf2f(p[k]) * (d[k] - dl) : 0.f);
}

// dlogits[n][t][:] = coef * (softmax(logits[n][t]) - onehot(labels[n][t+1])), zero rows where the label is ignored / t == T-1
__global__ __launch_bounds__(256) void ce_bwd_kernel(const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ coef,
                                                    bf16_t* __restrict__ dl, int T, long V, long ldl) {
  __shared__ float red[16];
  const int n = blockIdx.x / T, t = blockIdx.x % T;
  const bf16_t* row = logits + ((long)n * T + t) * ldl;
  bf16_t* out = dl + ((long)n * T + t) * ldl;
  const long lab = t + 1 < T ? labels[(long)n * T + t + 1] : -100;
  if (lab < 0 || lab >= V) {
    for (long i = threadIdx.x; i < V; i += blockDim.x) out[i] = 0;
    return;
  }
  if (ce_row_fast(row, V, ldl) && (((uintptr_t)out) & 7) == 0) {      // one read of the row (registers), one 8-byte write per quad
    CeRow r;
    r.load(row, V);
    float mx, s;
    r.stats(red, mx, s);
    const float c = coef[0], inv = 1.f / s;
    const long nq = V >> 2;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const long k = threadIdx.x + 256L * i;
      if (k < nq) {
        const long e0 = 4 * k;
        const float g0 = c * (__expf(__uint_as_float(r.q[i].x << 16) - mx) * inv - (e0 == lab ? 1.f : 0.f));
        const float g1 = c * (__expf(__uint_as_float(r.q[i].x & 0xffff0000u) - mx) * inv - (e0 + 1 == lab ? 1.f : 0.f));
        const float g2 = c * (__expf(__uint_as_float(r.q[i].y << 16) - mx) * inv - (e0 + 2 == lab ? 1.f : 0.f));
        const float g3 = c * (__expf(__uint_as_float(r.q[i].y & 0xffff0000u) - mx) * inv - (e0 + 3 == lab ? 1.f : 0.f));
        *reinterpret_cast<uint2*>(out + e0) = make_uint2(pack2bf(g0, g1), pack2bf(g2, g3));
      }
    }
    return;
  }
  float mx = -1e30f;
  for (long i = threadIdx.x; i < V; i += blockDim.x) mx = fmaxf(mx, bf2f(row[i]));
  mx = block_max(mx, red);
  float s = 0.f;
  for (long i = threadIdx.x; i < V; i += blockDim.x) s += __expf(bf2f(row[i]) - mx);
  s = block_sum(s, red);
  const float c = coef[0], inv = 1.f / s;
  for (long i = threadIdx.x; i < V; i += blockDim.x) out[i] = f2bf(c * (__expf(bf2f(row[i]) - mx) * inv - (i == lab ? 1.f : 0.f)));
}

// dst[idx[i]][:] += src[i][:]  (fp32 accumulation; embedding / gather gradients).  idx < 0 rows are skipped.
// No atomics: workgroup i handles source row i and is the OWNER of destination row d = idx[i] iff no earlier source row has the same
// destination (a scan of idx[0 .. i), 256 entries per step); the owner walks idx[i ..) in chunks of 1024, collects the source rows that
// hit d IN ASCENDING ORDER (one ballot per wave, prefix over the 4 waves) and adds them column by column -- the sum of a destination
// row is formed by one workgroup in source-row order, so the result does not depend on scheduling.
__global__ __launch_bounds__(256) void scatter_add_rows_kernel(const bf16_t* __restrict__ src, const int64_t* __restrict__ idx, float* __restrict__ dst,
                                                              long n, long cols) {
  __shared__ int s_list[1024];
  __shared__ int s_cnt[4];
  const long i = blockIdx.x;
  const long d = idx[i];
  if (d < 0) return;
  for (long j0 = 0; j0 < i; j0 += 256) {
    const long j = j0 + threadIdx.x;
    if (__syncthreads_or(j < i && idx[j] == d)) return;          // an earlier source row owns this destination
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long base = i; base < n; base += 1024) {
    // matches of this chunk, ascending: wave w scans rows base + 256 w + lane + 64 q (q = 0..3) -> per-thread 4 candidates out of order;
    // simpler and ordered: four sub-steps of 256 consecutive rows each
    int total = 0;
    for (int q = 0; q < 4; ++q) {
      const long j = base + 256 * q + threadIdx.x;
      const bool hit = j < n && idx[j] == d;
      const unsigned long long bal = __ballot(hit);
      if (lane == 0) s_cnt[wave] = __popcll(bal);
      __syncthreads();
      int off = total;
      for (int w2 = 0; w2 < wave; ++w2) off += s_cnt[w2];
      if (hit) s_list[off + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(j - base);
      total += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      __syncthreads();
    }
    if (total == 0) continue;
    for (long c = threadIdx.x; c < cols; c += 256) {
      float sacc = 0.f;
      for (int t = 0; t < total; ++t) sacc += bf2f(src[(base + s_list[t]) * cols + c]);
      dst[d * cols + c] += sacc;
    }
    __syncthreads();
  }
}

// sum of squares of a bf16 or fp32 buffer: one partial per workgroup -> part[blockIdx.x] (fold_column_kernel adds them in a fixed order)
__global__ __launch_bounds__(256) void sumsq_kernel(const void* __restrict__ x, long n, int is_f32, float* __restrict__ part) {
  __shared__ float red[16];
  float s = 0.f;
  if (is_f32 && (((uintptr_t)x) & 15) == 0) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
      const float4 v = x4[i];
      s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    if (blockIdx.x == 0)
      for (long i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) { const float v = reinterpret_cast<const float*>(x)[i]; s += v * v; }
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      const float v = is_f32 ? reinterpret_cast<const float*>(x)[i] : bf2f(reinterpret_cast<const bf16_t*>(x)[i]);
      s += v * v;
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Fused AdamW on fp32 master weights with bf16 model copy (DeepSpeed bf16 + AdamW(beta=(0.9,0.95), wd) semantics restated):
// g = grad * gscale[0];  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  master -= lr * (mhat / (sqrt(vhat) + eps) + wd * master)
__global__ __launch_bounds__(256) void adamw_kernel(bf16_t* __restrict__ p, float* __restrict__ master, const void* __restrict__ grad, int grad_f32,
                                                   float* __restrict__ m, float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2, const float* __restrict__ gscale) {
  const float gs = gscale ? gscale[0] : 1.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float g = gs * (grad_f32 ? reinterpret_cast<const float*>(grad)[i] : bf2f(reinterpret_cast<const bf16_t*>(grad)[i]));
    const float mi = b1 * m[i] + (1.f - b1) * g;
    const float vi = b2 * v[i] + (1.f - b2) * g * g;
    m[i] = mi; v[i] = vi;
    float w = master[i];
    w -= lr * ((mi / bc1) / (sqrtf(vi / bc2) + eps) + wd * w);
    master[i] = w;
    p[i] = f2bf(w);
  }
}

}  // namespace

extern "C" int llmseg_colsum(const void* x, float* out, int64_t M, int64_t N, int64_t ld, void* workspace, int64_t workspace_bytes, void* stream) {
  LL_CHECK(x && out && M > 0 && N > 0 && ld >= N, "colsum: bad arguments");
  // row slices: >= 32 rows each (8 per row-lane) and enough of them that the launch reaches ~256 workgroups -- the head's bias gradients are 512 rows
  // x 256..2048 columns, and with 256-row slices every thread walked 64 rows one dependent load after the other (10-22 us per call)
  const long colwg = (N + 63) / 64;
  long gy = min((long)64, max((long)1, min((long)((M + 31) / 32), (long)((256 + colwg - 1) / colwg))));
  gy = min(gy, workspace ? (long)(workspace_bytes / (N * 4)) : 0L);          // row slices the scratch can hold; <= 1: one slice, no scratch
  float* part = gy > 1 ? (float*)workspace : nullptr;
  if (gy < 1) gy = 1;
  LL_LAUNCH_KERNEL(colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, out, part, (long)M,
                     (long)N, (long)ld);
  if (part)
    LL_LAUNCH_KERNEL(fold_slices_kernel, dim3(fold_grid(N)), dim3(256), 0, (hipStream_t)stream, (const float*)part, (int)gy, (long)N, (long)N, (long)N,
                       FoldOut{{out, nullptr, nullptr, nullptr}});
  LL_LAUNCH_CHECK("colsum");
  return LLMSEG_OK;
}

extern "C" int llmseg_norm_bwd(const void* dy, const void* x, const void* w, void* dx, float* dw, float* db, int64_t rows, int64_t cols, float eps,
                               int rms, void* workspace, int64_t workspace_bytes, void* stream) {
  return llmseg_norm_bwd_add(dy, x, w, nullptr, dx, dw, db, rows, cols, eps, rms, workspace, workspace_bytes, stream);
}

extern "C" int llmseg_norm_bwd_add(const void* dy, const void* x, const void* w, const void* dres, void* dx, float* dw, float* db, int64_t rows, int64_t cols,
                                   float eps, int rms, void* workspace, int64_t workspace_bytes, void* stream) {
  LL_CHECK(dy && x && w && dx && rows > 0 && cols > 0 && (cols & 7) == 0 && AL16(dy) && AL16(x) && AL16(w) && AL16(dx) && AL16(dres), "norm_bwd: bad arguments");
  const int cpl = (int)(((cols >> 3) + 63) / 64);
  const bool wgrad = dw || db;
  if (!wgrad && rows >= 64 && cols >= 2048 && cols <= 8192) {        // wide rows, frozen weight: a workgroup per row (also for tall activations: the
    // wave-per-row kernel holds x and dy of a 4096-wide row in 64 VGPRs per lane under a 128-VGPR bound and its counters showed 1.48 x the algorithmic bytes)
    const int cpt = (int)(((cols >> 3) + 255) / 256);
#define LL_NORMBW(C)                                                                                                                                    \
  LL_LAUNCH_KERNEL(norm_bwd_wg_kernel<C>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, \
                   (bf16_t*)dx, (long)rows, (int)cols, eps, rms, (const bf16_t*)dres)
    if (cpt <= 1) LL_NORMBW(1); else if (cpt <= 2) LL_NORMBW(2); else LL_NORMBW(4);
#undef LL_NORMBW
    LL_LAUNCH_CHECK("norm_bwd");
    return LLMSEG_OK;
  }
  const bool acc = wgrad && cpl <= 2;
  const long wgs = (rows + 3) / 4;
  const long ws_floats = workspace ? workspace_bytes / 4 : 0;
  long G = acc ? std::min<long>(std::max<long>(1, (rows + 31) / 32), 256) : wgs;                          // ACC: every wave walks >= 8 rows
  float *part = nullptr, *stats = nullptr;
  if (acc) {
    G = std::min<long>(G, ws_floats / (2 * cols));                                                         // partial slots the scratch can hold
    if (G > 1) part = (float*)workspace; else G = 1;
  } else if (wgrad) {
    LL_CHECK(ws_floats >= 2 * rows + 2 * cols, "norm_bwd: weight gradients of a wide norm need workspace >= (2 rows + 2 cols) floats (row statistics)");
    stats = (float*)workspace;
  }
  const dim3 grid((unsigned)G);
#define LL_NORMB(C, A)                                                                                                                       \
  LL_LAUNCH_KERNEL((norm_bwd_kernel<C, A>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, \
                     (bf16_t*)dx, dw, db, (long)rows, (int)cols, eps, rms, (const bf16_t*)dres, part, stats)
  if (acc) { if (cpl <= 1) LL_NORMB(1, true); else LL_NORMB(2, true); }
  else if (cpl <= 1) LL_NORMB(1, false); else if (cpl <= 2) LL_NORMB(2, false); else if (cpl <= 4) LL_NORMB(4, false);
  else if (cpl <= 8) LL_NORMB(8, false); else LL_NORMB(0, false);
#undef LL_NORMB
  if (acc && part)
    LL_LAUNCH_KERNEL(fold_slices_kernel, dim3(fold_grid(2 * cols)), dim3(256), 0, (hipStream_t)stream, (const float*)part, (int)G, (long)(2 * cols),
                       (long)(2 * cols), (long)cols, FoldOut{{dw, db, nullptr, nullptr}});
  if (stats) {                                                     // wide rows: column sums from the stored (mean, rstd), row slices folded in order
    float* p2 = stats + ((2 * rows + 63) / 64) * 64;
    long gy = std::min<long>(64, (rows + 255) / 256);
    gy = std::min<long>(gy, (ws_floats - (p2 - stats)) / (2 * cols));
    if (gy <= 1) { gy = 1; p2 = nullptr; }
    LL_LAUNCH_KERNEL(norm_dwdb_kernel, dim3((unsigned)((cols + 63) / 64), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x,
                       (const float*)stats, dw, db, p2, (long)rows, (long)cols);
    if (p2)
      LL_LAUNCH_KERNEL(fold_slices_kernel, dim3(fold_grid(2 * cols)), dim3(256), 0, (hipStream_t)stream, (const float*)p2, (int)gy, (long)(2 * cols),
                         (long)(2 * cols), (long)cols, FoldOut{{dw, db, nullptr, nullptr}});
  }
  LL_LAUNCH_CHECK("norm_bwd");
  return LLMSEG_OK;
}

extern "C" int llmseg_swiglu_bwd(const void* gu, const void* dout, void* dgu, int64_t rows, int64_t I, void* stream) {
  LL_CHECK(gu && dout && dgu && rows > 0 && I > 0 && (I & 7) == 0 && AL16(gu) && AL16(dout) && AL16(dgu), "swiglu_bwd: bad arguments");
  LL_LAUNCH_KERNEL(swiglu_bwd_kernel, dim3(grid_for(rows * (I >> 3))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)gu, (const bf16_t*)dout,
                     (bf16_t*)dgu, (long)rows, (long)I, (long)I);
  LL_LAUNCH_CHECK("swiglu_bwd");
  return LLMSEG_OK;
}

// library-internal (gemm.hip, the two-launch route of llmseg_gemm_args.fx = LLMSEG_FX_SWIGLU_BWD): d(out) rows of stride ld_dout, possibly inside dgu's own rows
extern "C" __attribute__((visibility("hidden"))) int llmseg_swiglu_bwd_ld(const void* gu, const void* dout, void* dgu, int64_t rows, int64_t I, int64_t ld_dout, void* stream) {
  LL_CHECK(gu && dout && dgu && rows > 0 && I > 0 && (I & 7) == 0 && (ld_dout & 7) == 0 && AL16(gu) && AL16(dout) && AL16(dgu), "swiglu_bwd: bad arguments");
  LL_LAUNCH_KERNEL(swiglu_bwd_kernel, dim3(grid_for(rows * (I >> 3))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)gu, (const bf16_t*)dout,
                     (bf16_t*)dgu, (long)rows, (long)I, (long)ld_dout);
  LL_LAUNCH_CHECK("swiglu_bwd");
  return LLMSEG_OK;
}

extern "C" int llmseg_act_bwd(const void* dy, const void* y, void* out, int64_t n, int act, void* stream) {
  LL_CHECK(dy && y && out && n > 0 && (act == LLMSEG_ACT_RELU || act == LLMSEG_ACT_SIGMOID), "act_bwd: only relu/sigmoid are differentiated");
  LL_LAUNCH_KERNEL(act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)y, (bf16_t*)out, (long)n, act);
  LL_LAUNCH_CHECK("act_bwd");
  return LLMSEG_OK;
}

extern "C" int llmseg_softmax_rows(const float* S, void* P, int64_t BH, int32_t Tq, int32_t Tk, int32_t ld, float scale, int32_t causal,
                                   const uint8_t* key_mask, int32_t heads, void* stream) {
  LL_CHECK(S && P && BH > 0 && Tq > 0 && Tk > 0 && ld >= Tk && heads > 0 && (!causal || Tq == Tk), "softmax_rows: bad arguments");
  LL_LAUNCH_KERNEL(softmax_rows_kernel, dim3((unsigned)((BH * Tq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, S, (bf16_t*)P, (long)BH, Tq, Tk, ld,
                     scale, causal, key_mask, heads);
  LL_LAUNCH_CHECK("softmax_rows");
  return LLMSEG_OK;
}

extern "C" int llmseg_attn_ds(const void* P, const float* dP, void* dS, int64_t rows, int32_t T, int32_t ld, float scale, void* stream) {
  LL_CHECK(P && dP && dS && rows > 0 && T > 0 && ld >= T, "attn_ds: bad arguments");
  LL_LAUNCH_KERNEL(attn_ds_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)P, dP, (bf16_t*)dS, (long)rows, T,
                     ld, scale);
  LL_LAUNCH_CHECK("attn_ds");
  return LLMSEG_OK;
}

extern "C" int llmseg_ce_bwd(const void* logits, const int64_t* labels, const float* coef, void* dlogits, int32_t N, int32_t T, int64_t V, int64_t ldl,
                             void* stream) {
  LL_CHECK(logits && labels && coef && dlogits && N > 0 && T > 1 && V > 0 && ldl >= V, "ce_bwd: bad arguments");
  LL_LAUNCH_KERNEL(ce_bwd_kernel, dim3((unsigned)(N * T)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, labels, coef, (bf16_t*)dlogits, T,
                     (long)V, (long)ldl);
  LL_LAUNCH_CHECK("ce_bwd");
  return LLMSEG_OK;
}

extern "C" int llmseg_scatter_add_rows(const void* src, const int64_t* idx, float* dst, int64_t n, int64_t cols, void* stream) {
  LL_CHECK(src && idx && dst && n > 0 && cols > 0, "scatter_add_rows: bad arguments");
  LL_CHECK(n < (1L << 31), "scatter_add_rows: too many source rows");
  LL_LAUNCH_KERNEL(scatter_add_rows_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, idx, dst, (long)n, (long)cols);
  LL_LAUNCH_CHECK("scatter_add_rows");
  return LLMSEG_OK;
}

extern "C" int llmseg_sumsq(const void* x, int64_t n, int is_f32, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  LL_CHECK(x && out && n > 0, "sumsq: bad arguments");
  LL_CHECK(workspace && workspace_bytes >= 4, "sumsq: workspace (>= 4 bytes, 8 KiB for every partial) is required");
  long g = std::min<long>(2048, (n + 2047) / 2048);                       // >= 8 elements per thread
  g = std::max<long>(1, std::min<long>(g, workspace_bytes / 4));
  LL_LAUNCH_KERNEL(sumsq_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, (long)n, is_f32, (float*)workspace);
  LL_LAUNCH_KERNEL(fold_column_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, (long)g, out, 1.f);
  LL_LAUNCH_CHECK("sumsq");
  return LLMSEG_OK;
}

extern "C" int llmseg_adamw(void* p, float* master, const void* grad, int grad_f32, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int64_t step, const float* grad_scale, void* stream) {
  LL_CHECK(p && master && grad && m && v && n > 0 && step > 0, "adamw: bad arguments");
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  LL_LAUNCH_KERNEL(adamw_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, master, grad, grad_f32, m, v, (long)n, lr, beta1, beta2,
                     eps, weight_decay, bc1, bc2, grad_scale);
  LL_LAUNCH_CHECK("adamw");
  return LLMSEG_OK;
}

// ---- the norm backward's K-slice tail (with the LoRA branches' dX, lora.hip) and transpose_pad --------------------------------------------------
namespace {
// Split-K tail of a dX product that feeds a pre-norm's backward (llmseg_gemm_args.nb_x, round 6): a workgroup per row sums the row's S fp32 slab rows and
// rounds to bf16 (splitk_reduce_kernel's arithmetic: alpha = 1, no bias / activation / residual), optionally adds the LoRA branches' dX to it with
// lora_apply_kernel's arithmetic and rounds again (LORA: y += alpha * mask_b * (xa[:, 8b..] . W_b), W stored [8][N]), and -- holding that row as dy -- writes
// the norm backward + dres with norm_bwd_wg_kernel's arithmetic and thread -> column mapping: three launches and two round trips of the [M][N] gradient
// (reduce 6.9 + lora_apply 10.9 + norm_bwd 7.6 us per Llama layer at 2 images) in one pass.  Same bits as the three launches.
// lp != NULL (LORA only): the LoRA operand t = [s dq Bq | s dv Bv] arrives as the K-slice PARTIALS of llmseg_lora_down (fp32 [lS][rows][16]): threads 0..15 add
// the row's slices in order, scale and round to bf16 (lora_down_finish_kernel's arithmetic), hand the 16 values to the workgroup through LDS and store them (+ zero
// columns) into xa for the weight-gradient kernel -- the finish launch of the backward's rank-8 down projection rides here.
template <int CPT, bool LORA>
__global__ __launch_bounds__(256) void reduce_lora_normbwd_kernel(const float* __restrict__ slab, int S, long slab_sz, const bf16_t* __restrict__ x,
                                                                 const bf16_t* __restrict__ w, bf16_t* __restrict__ dx, long rows, int cols, float eps, int rms,
                                                                 const bf16_t* __restrict__ dres, bf16_t* __restrict__ xa, long ldxa,
                                                                 const bf16_t* __restrict__ w0, const bf16_t* __restrict__ w1, float alpha, int nb, DropP dp,
                                                                 const float* __restrict__ lp, int lS, float lscale, int lzero) {
  __shared__ float red[16];
  __shared__ float tl[16];
  const long row = blockIdx.x;
  const int nch = cols >> 3;
  const long N = cols;
  if (LORA && lp != nullptr) {
    if (threadIdx.x < 16) {
      float v = 0.f;
      if ((int)threadIdx.x < 8 * nb) {
        for (int s2 = 0; s2 < lS; ++s2) v += lp[((long)s2 * rows + row) * 16 + threadIdx.x];
        v *= lscale;
      }
      const bf16_t vb = f2bf(v);
      tl[threadIdx.x] = bf2f(vb);
      xa[row * ldxa + threadIdx.x] = vb;
    } else if ((int)threadIdx.x < 16 + lzero) xa[row * ldxa + threadIdx.x] = 0;
    __syncthreads();
  }
  uint4 xc[CPT], gc[CPT], wc[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = threadIdx.x + 256 * i;
    xc[i] = gc[i] = wc[i] = make_uint4(0, 0, 0, 0);
    if (c < nch) {
      xc[i] = *reinterpret_cast<const uint4*>(x + row * cols + c * 8);
      wc[i] = *reinterpret_cast<const uint4*>(w + c * 8);
      const float* sp = slab + row * N + c * 8;
      float4 a0 = *reinterpret_cast<const float4*>(sp), a1 = *reinterpret_cast<const float4*>(sp + 4);
      for (int s2 = 1; s2 < S; ++s2) {
        const float4 b0 = *reinterpret_cast<const float4*>(sp + s2 * slab_sz), b1 = *reinterpret_cast<const float4*>(sp + s2 * slab_sz + 4);
        a0.x += b0.x; a0.y += b0.y; a0.z += b0.z; a0.w += b0.w;
        a1.x += b1.x; a1.y += b1.y; a1.z += b1.z; a1.w += b1.w;
      }
      const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      gc[i] = pack8(v);                                   // the bf16 product row the reduce launch would have stored
      if (LORA) {
        float yv[8], wv[8];
        unpack8(gc[i], yv);
        for (int b = 0; b < nb; ++b) {
          const bf16_t* wl = b == 0 ? w0 : w1;
          float xv[8], dv[8];
          if (lp != nullptr) {
#pragma unroll
            for (int r = 0; r < 8; ++r) xv[r] = tl[8 * b + r];
          } else unpack8(*reinterpret_cast<const uint4*>(xa + row * ldxa + 8 * b), xv);
#pragma unroll
          for (int j = 0; j < 8; ++j) dv[j] = 0.f;
#pragma unroll
          for (int r = 0; r < LR; ++r) {
            unpack8(*reinterpret_cast<const uint4*>(wl + (long)r * N + c * 8), wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) dv[j] += xv[r] * wv[j];
          }
          if (dp.thr) {
            uint32_t oa;
            const unsigned long di = drop_index(dp, (unsigned long)row, (unsigned long)N, (unsigned long)(c * 8), oa);
            dropout8(dv, di, dp.stream + b, dp.rng, dp.thr, dp.scale, oa);
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) yv[j] += alpha * dv[j];
        }
        gc[i] = pack8(yv);                                // ... and the bf16 row lora_apply would have left
      }
    }
  }
  normbwd_row<CPT>(xc, gc, wc, red, dx, row, cols, eps, rms, dres);
}

// out[c][r] = in[r][c] for r < rows (zero for rows <= r < rows_pad): 64 x 64 tiles through LDS, 16-byte global accesses both ways.
__global__ __launch_bounds__(256) void transpose_pad_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, long rows, long cols, long ld_in,
                                                           long ld_out, long rows_pad) {
  __shared__ bf16_t tile[64][66];
  const long r0 = (long)blockIdx.y * 64, c0 = (long)blockIdx.x * 64;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = threadIdx.x + i * 256;
    const int r = idx >> 3, ch = idx & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r0 + r < rows && c0 + ch * 8 < cols) v = *reinterpret_cast<const uint4*>(in + (r0 + r) * ld_in + c0 + ch * 8);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&tile[r][ch * 8]);
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = threadIdx.x + i * 256;
    const int c = idx >> 3, rh = idx & 7;
    if (c0 + c >= cols || r0 + rh * 8 >= rows_pad) continue;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)tile[rh * 8 + 2 * j][c] | ((uint32_t)tile[rh * 8 + 2 * j + 1][c] << 16);
    *reinterpret_cast<uint4*>(out + (c0 + c) * ld_out + r0 + rh * 8) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

// library-internal (gemm.hip: the K-sliced route of llmseg_gemm_args.nb_x).  slab: fp32 [S][M][N]; la_t == NULL: no LoRA term.
extern "C" __attribute__((visibility("hidden"))) int llmseg_reduce_lora_normbwd(const float* slab, int S, int64_t M, int64_t N, const void* x, const void* w, void* dx, float eps,
                                                                                int rms, const void* dres, void* la_t, int64_t la_ldt, const void* la_w0,
                                                                                const void* la_w1, float la_alpha, const llmseg_dropout* la_drop, const float* la_part,
                                                                                int la_S, float la_scale, int la_zero, void* stream) {
  LL_CHECK(slab && S >= 1 && M > 0 && N >= 2048 && N <= 8192 && (N & 7) == 0 && x && w && dx && AL16(x) && AL16(w) && AL16(dx) && AL16(dres) && AL16(slab),
           "reduce_lora_normbwd: bad arguments");
  LL_CHECK(!la_t || (la_w0 && AL16(la_t) && AL16(la_w0) && AL16(la_w1) && (la_ldt & 7) == 0), "reduce_lora_normbwd: bad LoRA operands");
  LL_CHECK(!la_part || (la_t && la_S >= 1 && la_zero >= 0 && la_zero <= 240 && la_ldt >= 16 + la_zero), "reduce_lora_normbwd: bad LoRA partials");
  const DropP dp = make_drop(la_drop);
  const int cpt = (int)(((N >> 3) + 255) / 256), nb = la_w1 ? 2 : 1;
#define LL_RLN(C, L)                                                                                                                                     \
  LL_LAUNCH_KERNEL((reduce_lora_normbwd_kernel<C, L>), dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, slab, S, (long)(M * N), (const bf16_t*)x,    \
                   (const bf16_t*)w, (bf16_t*)dx, (long)M, (int)N, eps, rms, (const bf16_t*)dres, (bf16_t*)la_t, (long)la_ldt, (const bf16_t*)la_w0, \
                   (const bf16_t*)la_w1, la_alpha, nb, dp, la_part, la_S, la_scale, la_zero)
  if (la_t) { if (cpt <= 1) LL_RLN(1, true); else if (cpt <= 2) LL_RLN(2, true); else LL_RLN(4, true); }
  else { if (cpt <= 1) LL_RLN(1, false); else if (cpt <= 2) LL_RLN(2, false); else LL_RLN(4, false); }
#undef LL_RLN
  LL_LAUNCH_CHECK("reduce_lora_normbwd");
  return LLMSEG_OK;
}

extern "C" int llmseg_transpose_pad(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, int64_t rows_pad, void* stream) {
  LL_CHECK(in && out && rows > 0 && cols > 0 && rows_pad >= rows && ld_out >= rows_pad && ld_in >= cols, "transpose_pad: bad arguments");
  LL_CHECK((cols & 7) == 0 && (ld_in & 7) == 0 && (ld_out & 7) == 0 && (rows_pad & 7) == 0 && AL16(in) && AL16(out),
           "transpose_pad: cols, rows_pad and leading dimensions must be multiples of 8, pointers 16-byte aligned");
  LL_LAUNCH_KERNEL(transpose_pad_kernel, dim3((unsigned)((cols + 63) / 64), (unsigned)((rows_pad + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)in, (bf16_t*)out, (long)rows, (long)cols, (long)ld_in, (long)ld_out, (long)rows_pad);
  LL_LAUNCH_CHECK("transpose_pad");
  return LLMSEG_OK;
}

// ---- small trainable Linear y = act(x W^T + b): dX, dW += and db += in ONE launch (llmseg_linear_bwd) ------------------------------------------
// The head's Linears (a few hundred rows, weights of 256 x 256 .. 256 x 2048) used to cost five to seven launches each: act_bwd, the dX product, the dW product as
// K-slices + their reduce, colsum as row slices + their fold.  Here a workgroup owns a 32 x 64 tile of an OUTPUT and walks the whole contraction itself:
//   range W of the grid:  dW[n][k] = sum_m dpre[m][n] x[m][k]    (tile rows = n, contraction = m; the k-tile 0 workgroups also form db[n] = sum_m dpre[m][n])
//   range X of the grid:  dX[m][k] = sum_n dpre[m][n] w[n][k]    (tile rows = m, contraction = n)
// Both are C[i][k] = sum_c A[i][c] B[c][k] with B stored [c][k] (k contiguous) and A stored [c][i] (range W) or [i][c] (range X).  The contraction runs in chunks of
// 256: the chunk of A and of B goes to LDS with c contiguous (AT[i][c], BT[k][c]: a transposition for B and for range W's A, two c per 32-bit LDS store), wave w takes
// c in [64 w, 64 w + 64) of every chunk with v_mfma_f32_16x16x32_bf16 (2 x 4 blocks of 16 x 16), and the four waves' accumulators are folded through LDS in wave order.
// dpre = dy * act'(y) is formed while the chunk is staged, with act_bwd_kernel's expression and its bf16 rounding.  Everything outside the matrices reads as zero.
namespace {
constexpr int LB_TI = 32, LB_TK = 64, LB_CC = 256, LB_LD = LB_CC + 8;        // tile rows, tile columns, contraction chunk, LDS row pitch (elements)

struct LinBwd {
  const bf16_t *dy, *y, *x, *w;
  bf16_t* dx;
  float *dw, *db;
  int M, N, K, act, accumulate;
  int w_it, w_kt, x_kt;          // tiles of range W (rows, columns; columns = 1 when only db is wanted), column tiles of range X
  int vec_n, vec_k;              // 16-byte loads are legal on the [.][N] matrices (dy, y) / on the [.][K] matrices (x, w)
};

// 8 consecutive elements of row r from column c of a dense [rows][cols] bf16 matrix; zero outside the matrix
__device__ __forceinline__ uint4 lb_load8(const bf16_t* __restrict__ p, int r, int c, int rows, int cols, bool vec) {
  if (r >= rows || c >= cols) return make_uint4(0, 0, 0, 0);
  const bf16_t* q = p + (long)r * cols + c;
  if (vec) return *reinterpret_cast<const uint4*>(q);                        // cols % 8 == 0 and c % 8 == 0: the 8 elements are inside the row
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = c + j < cols ? (uint32_t)q[j] : 0u;
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// act_bwd_kernel on 8 elements
__device__ __forceinline__ uint4 lb_act8(const uint4& g, const uint4& yv, int act) {
  if (act == LLMSEG_ACT_NONE) return g;
  float gf[8], yf[8];
  uint32_t o[8];
  unpack8(g, gf); unpack8(yv, yf);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(act == LLMSEG_ACT_RELU ? (yf[e] > 0.f ? gf[e] : 0.f) : gf[e] * yf[e] * (1.f - yf[e]));
  return make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
}

__device__ __forceinline__ uint32_t lb_elem(const uint4& v, int j) {         // element j (0..7) of a packed row piece
  const uint32_t wd = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
  return (j & 1) ? (wd >> 16) : (wd & 0xffffu);
}

// rows c and c + 1 (pieces lo, hi: 8 columns each) -> T[col0 + j][c .. c + 1], j = 0..7
__device__ __forceinline__ void lb_store_t(bf16_t* T, int col0, int c, const uint4& lo, const uint4& hi) {
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<uint32_t*>(T + (col0 + j) * LB_LD + c) = lb_elem(lo, j) | (lb_elem(hi, j) << 16);
}

__global__ __launch_bounds__(256) void linear_bwd_kernel(const LinBwd p) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[(LB_TI + LB_TK) * LB_LD];          // 50688 bytes; the fold below re-uses the first 32 KiB
  bf16_t* AT = lds;
  bf16_t* BT = lds + LB_TI * LB_LD;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nW = p.w_it * p.w_kt;
  const bool roleW = (int)blockIdx.x < nW;
  const int bi = roleW ? (int)blockIdx.x : (int)blockIdx.x - nW;
  const int nkt = roleW ? p.w_kt : p.x_kt;
  const int i0 = (bi / nkt) * LB_TI, k0 = (bi % nkt) * LB_TK;
  const int C = roleW ? p.M : p.N;                                            // contraction length
  const bf16_t* __restrict__ B = roleW ? p.x : p.w;                          // [C][K]
  const bool vn = p.vec_n != 0, vk = p.vec_k != 0, has_act = p.act != LLMSEG_ACT_NONE;
  const bool want_db = roleW && (bi % nkt) == 0 && p.db != nullptr;

  uint4 ra[4], ry[4], rb[8];
  // A: range W reads row pairs (c, c + 1) x 8 columns i (512 pairs, two per thread); range X reads 32 rows i x 32 pieces of 8 c (four per thread)
  // B: row pairs (c, c + 1) x 8 columns k (1024 pairs, four per thread)
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int r, c;
      if (roleW) { const int pr = t + 256 * (q >> 1); r = c0 + 2 * (pr >> 2) + (q & 1); c = i0 + 8 * (pr & 3); }
      else { const int v = t + 256 * q; r = i0 + (v >> 5); c = c0 + 8 * (v & 31); }
      ra[q] = lb_load8(p.dy, r, c, p.M, p.N, vn);
      if (has_act) ry[q] = lb_load8(p.y, r, c, p.M, p.N, vn);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int pr = t + 256 * (q >> 1);
      rb[q] = lb_load8(B, c0 + 2 * (pr >> 3) + (q & 1), k0 + 8 * (pr & 7), C, p.K, vk);
    }
  };
  auto store_chunk = [&]() {
    if (has_act) {
#pragma unroll
      for (int q = 0; q < 4; ++q) ra[q] = lb_act8(ra[q], ry[q], p.act);
    }
    if (roleW) {
#pragma unroll
      for (int q = 0; q < 2; ++q) { const int pr = t + 256 * q; lb_store_t(AT, 8 * (pr & 3), 2 * (pr >> 2), ra[2 * q], ra[2 * q + 1]); }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int v = t + 256 * q; *reinterpret_cast<uint4*>(AT + (v >> 5) * LB_LD + 8 * (v & 31)) = ra[q]; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int pr = t + 256 * q; lb_store_t(BT, 8 * (pr & 7), 2 * (pr >> 3), rb[2 * q], rb[2 * q + 1]); }
  };

  f32x4_t acc[2][4];
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) acc[ib][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;

  const int nch = (C + LB_CC - 1) / LB_CC;
  load_chunk(0);
  for (int ch = 0; ch < nch; ++ch) {
    if (ch) __syncthreads();                                                  // the previous chunk has been read by every wave
    store_chunk();
    __syncthreads();
    if (ch + 1 < nch) load_chunk((ch + 1) * LB_CC);                           // in flight during this chunk's MFMAs
    if (want_db) {                                                            // thread = (row i = t / 8, c in [32 (t % 8), + 32) of the chunk), one term after the other
      const bf16_t* row = AT + (t >> 3) * LB_LD + 32 * (t & 7);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(row + 8 * v), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) dbacc += f[e];
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cw = wave * 64 + ks * 32;
      if (ch * LB_CC + cw >= C) break;                                        // nothing but zeros from here on (wave-uniform)
      const int cb = cw + 8 * (lane >> 4);
      bf16x8_t af[2], bf[4];
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) af[ib] = *reinterpret_cast<const bf16x8_t*>(AT + (16 * ib + (lane & 15)) * LB_LD + cb);
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) bf[kb] = *reinterpret_cast<const bf16x8_t*>(BT + (16 * kb + (lane & 15)) * LB_LD + cb);
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) acc[ib][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ib], bf[kb], acc[ib][kb], 0, 0, 0);
    }
  }

  if (want_db) {                                                              // the row's 8 threads are 8 consecutive lanes: a fixed tree
    dbacc += __shfl_xor(dbacc, 4, 64);
    dbacc += __shfl_xor(dbacc, 2, 64);
    dbacc += __shfl_xor(dbacc, 1, 64);
    const int n = i0 + (t >> 3);
    if ((t & 7) == 0 && n < p.N) p.db[n] = p.accumulate ? p.db[n] + dbacc : dbacc;
  }
  if (roleW && !p.dw) return;                                                 // db only (block-uniform)

  // fold the four waves' partial tiles in wave order: fold[w][i][k], C/D layout of the MFMA: column k = lane % 16, row i = 4 (lane / 16) + e
  float* fold = reinterpret_cast<float*>(lds);
  __syncthreads();
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 4; ++e) fold[(wave * LB_TI + 16 * ib + 4 * (lane >> 4) + e) * LB_TK + 16 * kb + (lane & 15)] = acc[ib][kb][e];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int idx = t + 256 * q, i = idx >> 6, k = idx & 63;
    float s = fold[idx];
    s += fold[LB_TI * LB_TK + idx];
    s += fold[2 * LB_TI * LB_TK + idx];
    s += fold[3 * LB_TI * LB_TK + idx];
    const int gi = i0 + i, gk = k0 + k;
    if (gk >= p.K) continue;
    if (roleW) {
      if (gi < p.N) { float* o = p.dw + (long)gi * p.K + gk; *o = p.accumulate ? *o + s : s; }
    } else if (gi < p.M) {
      p.dx[(long)gi * p.K + gk] = f2bf(s);
    }
  }
}
}  // namespace

extern "C" int llmseg_linear_bwd(const void* dy, const void* y, int act, const void* x, const void* w, void* dx, float* dw, float* db, int64_t M, int64_t N, int64_t K,
                                 int accumulate, void* stream) {
  LL_CHECK(dy && x && w && M > 0 && N > 0 && K > 0 && (dx || dw || db), "linear_bwd: bad arguments");
  LL_CHECK(act == LLMSEG_ACT_NONE || ((act == LLMSEG_ACT_RELU || act == LLMSEG_ACT_SIGMOID) && y), "linear_bwd: only relu/sigmoid are differentiated, from the output y");
  if (M > 2048 || N * K > (1L << 22)) return LLMSEG_NOT_TAKEN;               // one workgroup per output tile walks the whole contraction: small Linears only
  LinBwd p;
  p.dy = (const bf16_t*)dy; p.y = (const bf16_t*)y; p.x = (const bf16_t*)x; p.w = (const bf16_t*)w;
  p.dx = (bf16_t*)dx; p.dw = dw; p.db = db;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.act = act; p.accumulate = accumulate ? 1 : 0;
  p.w_it = (dw || db) ? (int)((N + LB_TI - 1) / LB_TI) : 0;
  p.w_kt = dw ? (int)((K + LB_TK - 1) / LB_TK) : 1;
  p.x_kt = (int)((K + LB_TK - 1) / LB_TK);
  p.vec_n = (N & 7) == 0 && AL16(dy) && (act == LLMSEG_ACT_NONE || AL16(y));
  p.vec_k = (K & 7) == 0 && AL16(x) && AL16(w);
  const long grid = (long)p.w_it * p.w_kt + (dx ? (long)((M + LB_TI - 1) / LB_TI) * p.x_kt : 0L);
  LL_LAUNCH_KERNEL(linear_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
  LL_LAUNCH_CHECK("linear_bwd");
  return LLMSEG_OK;
}
