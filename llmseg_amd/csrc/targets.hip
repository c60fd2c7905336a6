// Proposal decode + training-target computation on the device: what the reference does per sample on CPU
// workers -- pycocotools RLE decode (utils/sam_mask_reader.py:69-113), zero-pad to square + antialiased bilinear resize to 256 x 256
// (utils/reason_seg_dataset.py:166-173), IoU / IoP of every proposal against the ground truth (utils/utils.py:174-272) -- as three
// HBM-bound kernels on uint8 masks.  Integer results (pixels, intersections, areas) are exact; the IoU / IoP divisions are IEEE double
// divisions of those integers, i.e. bit-identical to numpy's.  All index tables (nearest-neighbour source rows / columns, resampling
// taps and weights) are computed on the host in float64 with the library formulas and passed in, so no device floating-point
// contraction can move a sample point.
#include <algorithm>
#include "common.h"
#include "llmseg_hip.h"

namespace {

// COCO RLE -> dense masks.  ends: inclusive prefix sums of the run lengths of all K masks, concatenated (uint32); offs[k] .. offs[k+1]
// is mask k's slice.  Runs alternate 0 / 1 starting with 0 and walk the image in COLUMN-major order (pixel index p = x H + y).
// out: [K][H][W] (hwk = 0) or [H][W][K] (hwk = 1, the reader's layout).
__global__ __launch_bounds__(256) void rle_decode_kernel(const uint32_t* __restrict__ ends, const int64_t* __restrict__ offs, uint8_t* __restrict__ out,
                                                        int K, int H, int W, int hwk) {
  const long n = (long)K * H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int k, y, x;
    if (hwk) { k = (int)(i % K); const long r = i / K; x = (int)(r % W); y = (int)(r / W); }
    else { x = (int)(i % W); const long r = i / W; y = (int)(r % H); k = (int)(r / H); }
    const uint32_t p = (uint32_t)x * (uint32_t)H + (uint32_t)y;
    long lo = offs[k], hi = offs[k + 1];                 // first run whose end exceeds p
    const long base = lo, last = hi;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (ends[mid] > p) hi = mid; else lo = mid + 1;
    }
    out[i] = lo == last ? (uint8_t)0 : (uint8_t)((lo - base) & 1);      // beyond the last run (malformed input): zero after any number of runs, as pycocotools leaves it
  }
}

// Per proposal k: S_k = |seg_k|, I_k = |seg_k & gt'|, where gt' is the ground truth resampled to the proposals' H x W grid by the
// nearest-neighbour maps gy[H], gx[W] (skimage.transform.resize(order=0) == scipy.ndimage.zoom(grid_mode=True), tables from the host).
// segs [K][H][W] uint8 (non-zero = inside).  cnt int64 [K][2] += {I_k, S_k}; gcnt int64[1] += |gt'| (added by the k = 0 blocks only).
__global__ __launch_bounds__(256) void mask_targets_kernel(const uint8_t* __restrict__ segs, const uint8_t* __restrict__ gt, const int32_t* __restrict__ gy,
                                                          const int32_t* __restrict__ gx, int H, int W, int Wg, unsigned long long* __restrict__ cnt,
                                                          unsigned long long* __restrict__ gcnt) {
  __shared__ unsigned long long sh[3];
  if (threadIdx.x < 3) sh[threadIdx.x] = 0;
  __syncthreads();
  const int k = blockIdx.y;
  const uint8_t* s = segs + (long)k * H * W;
  unsigned int ci = 0, cs = 0, cg = 0;
  const long n = (long)H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i % W);
    const unsigned int g = gt[(long)gy[y] * Wg + gx[x]] != 0, v = s[i] != 0;
    ci += v & g; cs += v; cg += g;
  }
  unsigned int v3[3] = {ci, cs, cg};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    unsigned int v = v3[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[j], (unsigned long long)v);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sh[0]) atomicAdd(&cnt[2 * k], sh[0]);
    if (sh[1]) atomicAdd(&cnt[2 * k + 1], sh[1]);
    if (k == 0 && sh[2]) atomicAdd(gcnt, sh[2]);
  }
}

// iou_k = I / (S + G - I), iop_k = I / S as IEEE doubles of the exact integer counts (numpy: np.sum(bool) / np.sum(bool); 0 / 0 = nan)
__global__ void targets_finalize_kernel(const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ gcnt, double* __restrict__ iou,
                                        double* __restrict__ iop, int K) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const double I = (double)cnt[2 * k], S = (double)cnt[2 * k + 1], G = (double)gcnt[0];
  iou[k] = I / (S + G - I);
  iop[k] = I / S;
}

// Antialiased separable resampling (torch F.interpolate(mode="bilinear", antialias=True, align_corners=False) of the zero-padded square
// mask): out[k][oy][ox] = sum_j wy[oy][j] sum_i wx[ox][i] in[k][y0[oy] + j][x0[ox] + i], samples beyond H / W are the zero padding.
// Tap tables (first index, count, weights in float64) come from the host.  Accumulation in double, one rounding to bf16.
__global__ __launch_bounds__(256) void resize_aa_kernel(const uint8_t* __restrict__ segs, bf16_t* __restrict__ out, int H, int W, int OS,
                                                       const int32_t* __restrict__ y0, const int32_t* __restrict__ ny, const double* __restrict__ wy,
                                                       const int32_t* __restrict__ x0, const int32_t* __restrict__ nx, const double* __restrict__ wx, int taps) {
  const int k = blockIdx.z, oy = blockIdx.y;
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  if (ox >= OS) return;
  const uint8_t* s = segs + (long)k * H * W;
  const int ys = y0[oy], yn = ny[oy], xs = x0[ox], xn = nx[ox];
  double acc = 0.0;
  for (int j = 0; j < yn; ++j) {
    const int y = ys + j;
    if (y >= H) break;                                   // zero padding below the image
    double row = 0.0;
    for (int i = 0; i < xn; ++i) {
      const int x = xs + i;
      if (x < W && s[(long)y * W + x]) row += wx[(long)ox * taps + i];
    }
    acc += wy[(long)oy * taps + j] * row;
  }
  out[((long)k * OS + oy) * OS + ox] = f2bf((float)acc);
}

// ---- one pass over the proposals (round 4) -----------------------------------------------------------------------------------------
// gtp[y][x] = (gt[gy[y]][gx[x]] != 0): the ground truth on the proposals' grid, built once per (image, ground truth) instead of being
// gathered again for every proposal
__global__ __launch_bounds__(256) void gt_resample_kernel(const uint8_t* __restrict__ gt, const int32_t* __restrict__ gy, const int32_t* __restrict__ gx,
                                                         uint8_t* __restrict__ out, int H, int W, int Wg) {
  const long n = (long)H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i % W);
    out[i] = gt[(long)gy[y] * Wg + gx[x]] != 0;
  }
}

// Every byte of a proposal is read ONCE (16-byte loads, through the `order` index -- no gathered copy of the selected proposals) and feeds
// (a) the integer counts |seg|, |seg & gt'_g| for up to 4 ground truths and (b) the antialiased resize, done separably with EXACTLY the
// arithmetic of resize_aa_kernel: rowsum[y][ox] = sum_i wx[ox][i] in[y][x0 + i] (double, i ascending), then out[oy][ox] = bf16(sum_j wy[oy][j]
// rowsum[y0 + j][ox]) (double, j ascending) -- the per-row sums are shared by the ~2 output rows that use them instead of being recomputed
// per output pixel (adding 0.0 where the old kernel skipped a tap is exact).  Grid = (proposal, slice of output rows): a workgroup walks its
// output rows in order, stages the input rows they need FOUR at a time in LDS, keeps their row sums in a ring of RING rows x OS doubles, and
// counts the input rows [first row of its slice, first row of the next slice) -- a disjoint cover of the image; counts are integer atomics.
// Limits: OS <= 256 (one thread per output column), taps + 4 <= RING, W <= 2048.
constexpr int TG_ROWS = 4, TG_MAXW = 2048, TG_MAXG = 4, TG_WREG = 12;
template <int RING>
__global__ __launch_bounds__(256) void proposal_targets_kernel(const uint8_t* __restrict__ masks, const int64_t* __restrict__ order, const uint8_t* __restrict__ gtp,
                                                              int n_gt, bf16_t* __restrict__ out, int H, int W, int OS, const int32_t* __restrict__ y0,
                                                              const int32_t* __restrict__ ny, const double* __restrict__ wy, const int32_t* __restrict__ x0,
                                                              const int32_t* __restrict__ nx, const double* __restrict__ wx, int taps,
                                                              unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ gcnt, int K) {
  __shared__ double ring[RING][256];
  __shared__ __attribute__((aligned(16))) uint8_t rows[TG_ROWS][TG_MAXW + 16];    // + 16: the word reads of the last column's window
  __shared__ unsigned int s_cnt[1 + 2 * TG_MAXG];
  const int k = blockIdx.x, t = threadIdx.x;
  const int oy_a = (int)((long)blockIdx.y * OS / gridDim.y), oy_b = (int)((long)(blockIdx.y + 1) * OS / gridDim.y);
  const int cnt_a = blockIdx.y == 0 ? 0 : y0[oy_a], cnt_b = blockIdx.y + 1 == gridDim.y ? H : min(H, y0[oy_b]);      // input rows this slice counts
  const uint8_t* m = masks + (order ? order[k] : (long)k) * H * W;
  if (t < 1 + 2 * TG_MAXG) s_cnt[t] = 0;
  const int ox = t;
  const bool col_on = ox < OS;
  const int xs = col_on ? x0[ox] : 0, xn = col_on ? nx[ox] : 0;
  unsigned int c_s = 0, c_i[TG_MAXG] = {0, 0, 0, 0}, c_g[TG_MAXG] = {0, 0, 0, 0};
  const int wch = (W + 15) >> 4;                                   // 16-byte chunks per row (the last may be partial)
  const bool vec_ok = (W & 15) == 0 && ((((uintptr_t)m) & 15) == 0) && (gtp == nullptr || (((uintptr_t)gtp) & 15) == 0);
  auto nzmask = [](uint32_t w) {            // per byte: 1 if any bit is set (each fold is masked so that no bit crosses a byte boundary)
    w = (w | (w >> 4)) & 0x0f0f0f0fu; w = (w | (w >> 2)) & 0x03030303u; return (w | (w >> 1)) & 0x01010101u;
  };
  auto stage = [&](int ya, int nrows) {                            // rows ya .. ya + nrows - 1 -> LDS, counting the ones this slice owns
    for (int idx = t; idx < nrows * wch; idx += 256) {
      const int r = idx / wch, c = idx - r * wch;
      const int y = ya + r;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (vec_ok) v = *reinterpret_cast<const uint4*>(m + (long)y * W + c * 16);
      else {
        uint8_t* vb = reinterpret_cast<uint8_t*>(&v);
        for (int e = 0; e < 16; ++e) { const int x = c * 16 + e; vb[e] = x < W ? m[(long)y * W + x] : 0; }
      }
      *reinterpret_cast<uint4*>(&rows[r][c * 16]) = v;
      if (y < cnt_a || y >= cnt_b) continue;
      const uint32_t n0 = nzmask(v.x), n1 = nzmask(v.y), n2 = nzmask(v.z), n3 = nzmask(v.w);      // non-zero bytes -> 0x01 each (masks hold 0 / 1 or 0 / 255)
      c_s += __popc(n0) + __popc(n1) + __popc(n2) + __popc(n3);
      for (int g = 0; g < n_gt; ++g) {
        uint4 q = make_uint4(0, 0, 0, 0);
        const uint8_t* gp = gtp + ((long)g * H + y) * W;
        if (vec_ok) q = *reinterpret_cast<const uint4*>(gp + c * 16);
        else {
          uint8_t* qb = reinterpret_cast<uint8_t*>(&q);
          for (int e = 0; e < 16; ++e) { const int x = c * 16 + e; qb[e] = x < W ? gp[x] : 0; }
        }
        const uint32_t g0 = nzmask(q.x), g1 = nzmask(q.y), g2 = nzmask(q.z), g3 = nzmask(q.w);
        c_i[g] += __popc(n0 & g0) + __popc(n1 & g1) + __popc(n2 & g2) + __popc(n3 & g3);
        if (k == 0) c_g[g] += __popc(g0) + __popc(g1) + __popc(g2) + __popc(g3);
      }
    }
  };
  double wreg[TG_WREG];                                            // this column's horizontal weights (register-resident when there are <= 12 taps)
  const bool in_regs = taps <= TG_WREG;
#pragma unroll
  for (int i = 0; i < TG_WREG; ++i) {
    const bool on = col_on && in_regs && i < xn && xs + i < W;      // a tap beyond the row (zero padding) or beyond the window weighs nothing
    wreg[i] = on ? wx[(long)ox * taps + i] : 0.0;
  }
  const int xw = min(xs, TG_MAXW - 1) & ~3;                         // the window's 12 bytes = 4 aligned LDS words + one byte-align per 4 taps
  const unsigned sh = (unsigned)(min(xs, TG_MAXW - 1) & 3);
  auto rowsums = [&](int ya, int nrows) {                          // rowsum rows ya .. into the ring: branch-free, the four rows' chains interleave
    if (!col_on) return;
    if (in_regs) {
      double acc[TG_ROWS];
#pragma unroll
      for (int r = 0; r < TG_ROWS; ++r) acc[r] = 0.0;
#pragma unroll
      for (int r = 0; r < TG_ROWS; ++r) {                            // rows beyond nrows hold stale bytes: computed, never stored
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(&rows[r][xw]);
        const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
        const uint32_t b[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh)};
#pragma unroll
        for (int i = 0; i < TG_WREG; ++i) acc[r] += ((b[i >> 2] >> (8 * (i & 3))) & 0xffu) ? wreg[i] : 0.0;
      }
#pragma unroll
      for (int r = 0; r < TG_ROWS; ++r)
        if (r < nrows) ring[(ya + r) & (RING - 1)][ox] = acc[r];
    } else {
      for (int r = 0; r < nrows; ++r) {
        double acc = 0.0;
        for (int i = 0; i < xn; ++i) {
          const int x = xs + i;
          if (x < W && rows[r][x]) acc += wx[(long)ox * taps + i];
        }
        ring[(ya + r) & (RING - 1)][ox] = acc;
      }
    }
  };
  int next_y = blockIdx.y == 0 ? 0 : y0[oy_a];
  for (int oy = oy_a; oy < oy_b; ++oy) {
    const int ya = y0[oy], need = min(H, ya + ny[oy]);
    while (next_y < need) {
      const int nrows = min(TG_ROWS, H - next_y);                  // staging ahead of `need` is fine: the ring holds taps + 4 rows
      __syncthreads();                                             // the previous batch's readers are done with `rows`
      stage(next_y, nrows);
      __syncthreads();
      rowsums(next_y, nrows);
      next_y += nrows;
    }
    __syncthreads();                                               // ring rows of this output row are complete
    if (col_on) {
      double acc = 0.0;
      const int yn = ny[oy];
      for (int j = 0; j < yn; ++j) {
        const int y = ya + j;
        if (y >= H) break;                                         // zero padding below the image
        acc += wy[(long)oy * taps + j] * ring[y & (RING - 1)][ox];
      }
      out[((long)k * OS + oy) * OS + ox] = f2bf((float)acc);
    }
  }
  // rows this slice owns but none of its windows reached: counts only
  while (next_y < cnt_b) {
    const int nrows = min(TG_ROWS, cnt_b - next_y);
    __syncthreads();
    stage(next_y, nrows);
    next_y += nrows;
  }
  auto fold = [&](unsigned int v, int slot) {                      // wave shuffles, then LDS
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0 && v) atomicAdd(&s_cnt[slot], v);
  };
  __syncthreads();
  fold(c_s, 0);
  for (int g = 0; g < n_gt; ++g) { fold(c_i[g], 1 + 2 * g); if (k == 0) fold(c_g[g], 2 + 2 * g); }
  __syncthreads();
  if (t < n_gt) {                                                  // integer atomics onto zero-filled counters: exact in any order
    if (s_cnt[1 + 2 * t]) atomicAdd(&cnt[((long)t * K + k) * 2], (unsigned long long)s_cnt[1 + 2 * t]);
    if (s_cnt[0]) atomicAdd(&cnt[((long)t * K + k) * 2 + 1], (unsigned long long)s_cnt[0]);
    if (k == 0 && s_cnt[2 + 2 * t]) atomicAdd(&gcnt[t], (unsigned long long)s_cnt[2 + 2 * t]);
  }
}

// ---- COCO RLE codec (the proposals' FILE format: pycocotools rleEncode + rleToString / rleFrString) ---------------------------------------
// Encode.  The mask is row-major but the runs walk it column-major (p = x H + y).  A UNIT is RE_SEG rows of one column; units are ordered as
// the walk meets them (u = x S + s, S = ceil(H / RE_SEG)).  A lane owns four adjacent columns of one row segment and loops over y: the wave
// reads 256 contiguous bytes per row, no transpose, and a tall image spreads over S lanes per column.  A TRANSITION is a pixel that differs
// from its predecessor in the walk (pixel 0 against a virtual 0); t_0 < t_1 < ... are their positions.  counts[i] = t_i - t_(i-1) (t_-1 = 0),
// the last count is H W - t_(n-1).  Three steps, every output position from a prefix sum:
//   walk<false>: per unit {number of transitions, positions of its last three}                                   -> rec[k][u]
//   scan       : per mask, exclusive scan over the units of {sum, last three transitions of the concatenation}     -> rec[k][u], n_counts
//   walk<true> : the same walk with the unit's carry {index of its first transition, t_(i-1), t_(i-2), t_(i-3)}: writes counts[i] (i < cap)
//                and the unit's character total (the delta needs three transitions back)                          -> rec[k][u].x
//   chars      : per mask, deltas of the stored counts -> character lengths -> scan -> characters; n_chars = sum of the units' totals
constexpr int RE_SEG = 64;
constexpr uint32_t RE_NONE = 0xffffffffu;                 // no transition (positions are < 2^31)
struct RleAgg { uint32_t n, a1, a2, a3; };                // a1 = the most recent transition
__device__ __forceinline__ RleAgg rle_join(const RleAgg& l, const RleAgg& r) {      // l earlier in the walk; associative
  RleAgg o;
  o.n = l.n + r.n;
  if (r.a1 == RE_NONE) { o.a1 = l.a1; o.a2 = l.a2; o.a3 = l.a3; }
  else if (r.a2 == RE_NONE) { o.a1 = r.a1; o.a2 = l.a1; o.a3 = l.a2; }
  else if (r.a3 == RE_NONE) { o.a1 = r.a1; o.a2 = r.a2; o.a3 = l.a1; }
  else { o.a1 = r.a1; o.a2 = r.a2; o.a3 = r.a3; }
  return o;
}
__device__ __forceinline__ RleAgg rle_shfl_up(const RleAgg& v, int o) {
  RleAgg r;
  r.n = __shfl_up(v.n, o, 64); r.a1 = __shfl_up(v.a1, o, 64); r.a2 = __shfl_up(v.a2, o, 64); r.a3 = __shfl_up(v.a3, o, 64);
  return r;
}
// characters of one (delta-coded) count: 5-bit groups until the rest is pure sign extension
__device__ __forceinline__ int rle_nchars(long x) {
  int n = 0;
  bool more;
  do { const int c = (int)(x & 0x1f); x >>= 5; more = (c & 0x10) ? x != -1 : x != 0; ++n; } while (more);
  return n;
}
// inclusive scan over the 256 threads of a workgroup (wave64 shuffles, then the four wave totals through LDS); total = the workgroup's sum
template <typename T>
__device__ __forceinline__ T block_scan256(T v, T* wt, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
  __syncthreads();                                         // the previous scan's readers are done with wt
  if (lane == 63) wt[wave] = inc;
  __syncthreads();
  T pre = 0;
  for (int w = 0; w < wave; ++w) pre += wt[w];
  total = wt[0] + wt[1] + wt[2] + wt[3];
  return inc + pre;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void rle_walk_kernel(const uint8_t* __restrict__ masks, int H, int W, int S, int WQ, int bpm, uint4* __restrict__ rec,
                                                      uint32_t* __restrict__ counts, int cap_counts) {
  const int k = blockIdx.x / bpm;
  const long g = (long)(blockIdx.x - k * bpm) * 256 + threadIdx.x;
  if (g >= (long)S * WQ) return;
  const int s = (int)(g / WQ), x4 = (int)(g % WQ) * 4;
  const uint8_t* m = masks + (long)k * H * W;
  const int y0 = s * RE_SEG, y1 = min(H, y0 + RE_SEG), nc = min(4, W - x4);
  const bool vec = (W & 3) == 0 && (((uintptr_t)masks) & 3) == 0;
  const uint32_t valid = nc == 4 ? 0x01010101u : (0x01010101u & ((1u << (8 * nc)) - 1u));
  auto load4 = [&](int y) -> uint32_t {                    // byte c = 1 where pixel (y, x4 + c) is set
    uint32_t w = 0;
    if (vec) w = *reinterpret_cast<const uint32_t*>(m + (long)y * W + x4);
    else
      for (int c = 0; c < nc; ++c) w |= (uint32_t)m[(long)y * W + x4 + c] << (8 * c);
    w = (w | (w >> 4)) & 0x0f0f0f0fu; w = (w | (w >> 2)) & 0x03030303u;
    return (w | (w >> 1)) & 0x01010101u;
  };
  uint32_t prev;                                           // the walk's predecessors of row y0: the row above, or the foot of the column to the left
  if (y0 > 0) prev = load4(y0 - 1);
  else prev = ((load4(H - 1) << 8) | (x4 > 0 ? (uint32_t)(m[(long)(H - 1) * W + x4 - 1] != 0) : 0u)) & valid;
  uint32_t n[4], a1[4], a2[4], a3[4], len[4];
  uint4* R = rec + (long)k * W * S;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    n[c] = 0; a1[c] = a2[c] = a3[c] = RE_NONE; len[c] = 0;
    if (WRITE && c < nc) { const uint4 r = R[(long)(x4 + c) * S + s]; n[c] = r.x; a1[c] = r.y; a2[c] = r.z; a3[c] = r.w; }      // n = index of the next transition
  }
  uint32_t* crow = WRITE ? counts + (long)k * cap_counts : nullptr;
  auto emit = [&](uint32_t i, uint32_t p, uint32_t b1, uint32_t b2, uint32_t b3) -> uint32_t {      // count i ends at p; -> its characters
    const uint32_t cnt = p - (i >= 1 ? b1 : 0u);
    const long d = i >= 3 ? (long)cnt - (long)(b2 - b3) : (long)cnt;
    if (i < (uint32_t)cap_counts) crow[i] = cnt;
    return (uint32_t)rle_nchars(d);
  };
  for (int yb = y0; yb < y1; yb += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = yb + j < y1 ? load4(yb + j) : 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (yb + j >= y1) break;
      const uint32_t d = v[j] ^ prev;
      prev = v[j];
      if (!d) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (!((d >> (8 * c)) & 1u)) continue;
        const uint32_t p = (uint32_t)(x4 + c) * (uint32_t)H + (uint32_t)(yb + j);
        if (WRITE) len[c] += emit(n[c], p, a1[c], a2[c], a3[c]);
        ++n[c]; a3[c] = a2[c]; a2[c] = a1[c]; a1[c] = p;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c >= nc) continue;
    if (WRITE) {
      if (x4 + c == W - 1 && s == S - 1) len[c] += emit(n[c], (uint32_t)H * (uint32_t)W, a1[c], a2[c], a3[c]);      // the run that reaches the end of the walk
      R[(long)(x4 + c) * S + s].x = len[c];
    } else R[(long)(x4 + c) * S + s] = make_uint4(n[c], a1[c], a2[c], a3[c]);
  }
}

// rec[k][u] <- exclusive scan over u of rle_join; n_counts[k] = transitions + 1.  One workgroup per mask, four units per thread, carry across chunks.
__global__ __launch_bounds__(256) void rle_scan_kernel(uint4* __restrict__ rec, int U, int32_t* __restrict__ n_counts) {
  __shared__ RleAgg wt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint4* R = rec + (long)blockIdx.x * U;
  const RleAgg none = {0u, RE_NONE, RE_NONE, RE_NONE};
  RleAgg carry = none;
  for (int base = 0; base < U; base += 1024) {
    const int u0 = base + (int)threadIdx.x * 4;
    RleAgg e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j] = none;
      if (u0 + j < U) { const uint4 r = R[u0 + j]; e[j] = RleAgg{r.x, r.y, r.z, r.w}; }
    }
    RleAgg inc = rle_join(rle_join(e[0], e[1]), rle_join(e[2], e[3]));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const RleAgg t = rle_shfl_up(inc, o); if (lane >= o) inc = rle_join(t, inc); }
    RleAgg pre = rle_shfl_up(inc, 1);                      // exclusive inside the wave
    if (lane == 0) pre = none;
    if (lane == 63) wt[wave] = inc;
    __syncthreads();
    RleAgg before = carry, total = carry;
    for (int w = 0; w < 4; ++w) { if (w < wave) before = rle_join(before, wt[w]); total = rle_join(total, wt[w]); }
    pre = rle_join(before, pre);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (u0 + j < U) { R[u0 + j] = make_uint4(pre.n, pre.a1, pre.a2, pre.a3); pre = rle_join(pre, e[j]); }
    carry = total;
    __syncthreads();                                       // wt is rewritten by the next chunk
  }
  if (threadIdx.x == 0) n_counts[blockIdx.x] = (int32_t)(carry.n + 1u);
}

// stored counts -> deltas -> characters at scanned offsets; n_chars[k] = the units' character totals (true also when a cap cut the rows)
__global__ __launch_bounds__(256) void rle_chars_kernel(const uint4* __restrict__ rec, int U, const uint32_t* __restrict__ counts, const int32_t* __restrict__ n_counts,
                                                       int cap_counts, uint8_t* __restrict__ chars, int32_t* __restrict__ n_chars, int cap_chars) {
  __shared__ uint32_t wt[4];
  const int k = blockIdx.x;
  const uint32_t* c = counts + (long)k * cap_counts;
  uint8_t* out = chars + (long)k * cap_chars;
  const int n = min(n_counts[k], cap_counts);
  uint32_t carry = 0, total;
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    long d = 0;
    uint32_t len = 0;
    if (i < n) { d = (long)c[i]; if (i >= 3) d -= (long)c[i - 2]; len = (uint32_t)rle_nchars(d); }
    uint32_t pos = carry + block_scan256(len, wt, total) - len;
    for (uint32_t j = 0; j < len; ++j, ++pos) {
      int ch = (int)(d & 0x1f);
      d >>= 5;
      if (j + 1 < len) ch |= 0x20;
      if (pos < (uint32_t)cap_chars) out[pos] = (uint8_t)(ch + 48);
    }
    carry += total;
  }
  uint32_t sum = 0;
  for (int u = threadIdx.x; u < U; u += 256) sum += rec[(long)k * U + u].x;
  block_scan256(sum, wt, total);
  if (threadIdx.x == 0) n_chars[k] = (int32_t)total;
}

// Parse.  Every count ends at a character without the continuation bit (bit 5), so the number of such characters before character j is the
// index of j's count, inside the mask and -- strings end on one -- in the concatenated output.  One workgroup per mask walks its string in
// chunks of 256 characters; the thread at a count's LAST character gathers the count's (at most 7) groups, and the delta coding
// cnt[i] = v[i] + cnt[i - 2] (i >= 3) is two interleaved prefix sums (odd indices from 1, even indices from 2; index 0 stands alone), followed
// by the inclusive sum to run ends: block scans with a carry across the chunks, all mod 2^32.
__global__ __launch_bounds__(256) void rle_parse_count_kernel(const uint8_t* __restrict__ chars, const int64_t* __restrict__ co, int32_t* __restrict__ n) {
  __shared__ uint32_t wt[4];
  const long a = co[blockIdx.x], b = co[blockIdx.x + 1];
  uint32_t c = 0, total;
  for (long j = a + threadIdx.x; j < b; j += 256) c += (((int)chars[j] - 48) & 0x20) == 0;
  block_scan256(c, wt, total);
  if (threadIdx.x == 0) n[blockIdx.x] = (int32_t)total;
}
__global__ __launch_bounds__(256) void rle_parse_offsets_kernel(const int32_t* __restrict__ n, int K, int64_t* __restrict__ ro) {
  __shared__ long wt[4];
  long carry = 0, total;
  if (threadIdx.x == 0) ro[0] = 0;
  for (int base = 0; base < K; base += 256) {
    const int k = base + (int)threadIdx.x;
    const long inc = block_scan256<long>(k < K ? (long)n[k] : 0L, wt, total);
    if (k < K) ro[k + 1] = carry + inc;
    carry += total;
  }
}
__global__ __launch_bounds__(256) void rle_parse_kernel(const uint8_t* __restrict__ chars, const int64_t* __restrict__ co, const int64_t* __restrict__ ro,
                                                       uint32_t* __restrict__ run_ends) {
  __shared__ uint32_t wt[4];
  const long a = co[blockIdx.x], b = co[blockIdx.x + 1];
  uint32_t* out = run_ends + ro[blockIdx.x];
  uint32_t c_idx = 0, c_odd = 0, c_even = 0, c_end = 0, total;
  for (long base = a; base < b; base += 256) {
    const long j = base + threadIdx.x;
    const int bj = j < b ? (int)chars[j] - 48 : 0x20;
    const bool last = j < b && (bj & 0x20) == 0;
    const uint32_t i = c_idx + block_scan256<uint32_t>(last ? 1u : 0u, wt, total) - (last ? 1u : 0u);      // this count's index in its mask
    c_idx += total;
    uint32_t val = 0;
    if (last) {
      long st = j;                                         // first character of the count: at most 6 continuation characters back, inside the mask
      while (st > a && j - st < 6 && ((((int)chars[st - 1] - 48) & 0x20) != 0)) --st;
      unsigned long x = 0;
      for (long q = st; q <= j; ++q) x |= (unsigned long)(((int)chars[q] - 48) & 0x1f) << (5 * (int)(q - st));
      if (bj & 0x10) x |= ~0ul << (5 * (int)(j - st + 1));
      val = (uint32_t)x;
    }
    const bool odd = (i & 1u) != 0;
    const uint32_t s_odd = c_odd + block_scan256<uint32_t>(last && odd ? val : 0u, wt, total);
    c_odd += total;
    const uint32_t s_even = c_even + block_scan256<uint32_t>(last && !odd && i >= 2 ? val : 0u, wt, total);
    c_even += total;
    const uint32_t cnt = !last ? 0u : i == 0 ? val : odd ? s_odd : s_even;
    const uint32_t end = c_end + block_scan256<uint32_t>(cnt, wt, total);
    c_end += total;
    if (last) out[i] = end;
  }
}

}  // namespace

extern "C" int llmseg_gt_resample(const uint8_t* gt, const int32_t* gy, const int32_t* gx, uint8_t* out, int32_t H, int32_t W, int32_t Hg, int32_t Wg, void* stream) {
  LL_CHECK(gt && gy && gx && out && H > 0 && W > 0 && Hg > 0 && Wg > 0, "gt_resample: bad arguments");
  const long n = (long)H * W;
  LL_LAUNCH_KERNEL(gt_resample_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, gt, gy, gx, out, H, W, Wg);
  LL_LAUNCH_CHECK("gt_resample");
  return LLMSEG_OK;
}

extern "C" int llmseg_proposal_targets(const uint8_t* masks, const int64_t* order, const uint8_t* gtp, int32_t n_gt, void* out, int32_t K, int32_t H, int32_t W,
                                       int32_t out_size, const int32_t* y0, const int32_t* ny, const double* wy, const int32_t* x0, const int32_t* nx,
                                       const double* wx, int32_t taps, int64_t* counts, int64_t* gt_area, double* iou, double* iop, void* stream) {
  LL_CHECK(masks && out && y0 && ny && wy && x0 && nx && wx && K > 0 && H > 0 && W > 0, "proposal_targets: bad arguments");
  LL_CHECK(out_size > 0 && out_size <= 256 && taps > 0 && taps + TG_ROWS <= 32 && W <= TG_MAXW,
           "proposal_targets: out_size <= 256, taps <= 28, W <= 2048 (use llmseg_mask_targets + llmseg_resize_aa beyond)");
  LL_CHECK(n_gt >= 0 && n_gt <= TG_MAXG && (n_gt == 0 || (gtp && counts && gt_area && iou && iop)), "proposal_targets: 0..4 ground truths with their outputs");
  if (n_gt) {
    LL_CHECK(hipMemsetAsync(counts, 0, (size_t)n_gt * K * 2 * sizeof(int64_t), (hipStream_t)stream) == hipSuccess, "proposal_targets: memset failed");
    LL_CHECK(hipMemsetAsync(gt_area, 0, (size_t)n_gt * sizeof(int64_t), (hipStream_t)stream) == hipSuccess, "proposal_targets: memset failed");
  }
  // slices of output rows per proposal: enough workgroups for ~4 per CU (the kernel is latency-bound per workgroup), each >= 16 output rows
  int ns = (int)std::min<long>(std::max<long>(1, 1024 / K), std::max(1, out_size / 16));
  const dim3 grid((unsigned)K, (unsigned)ns);
#define LL_PT(R)                                                                                                                                              \
  LL_LAUNCH_KERNEL(proposal_targets_kernel<R>, grid, dim3(256), 0, (hipStream_t)stream, masks, order, gtp, n_gt, (bf16_t*)out, H, W, out_size, y0, ny, wy, x0, nx, \
                   wx, taps, (unsigned long long*)counts, (unsigned long long*)gt_area, K)
  if (taps + TG_ROWS <= 16) LL_PT(16); else LL_PT(32);
#undef LL_PT
  for (int g = 0; g < n_gt; ++g)
    LL_LAUNCH_KERNEL(targets_finalize_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)counts + (long)g * K * 2,
                     (const unsigned long long*)gt_area + g, iou + (long)g * K, iop + (long)g * K, K);
  LL_LAUNCH_CHECK("proposal_targets");
  return LLMSEG_OK;
}

extern "C" int llmseg_rle_decode(const uint32_t* run_ends, const int64_t* offsets, uint8_t* out, int32_t K, int32_t H, int32_t W, int32_t hwk, void* stream) {
  LL_CHECK(run_ends && offsets && out && K > 0 && H > 0 && W > 0 && (long)H * W < (1L << 32), "rle_decode: bad arguments");
  const long n = (long)K * H * W;
  LL_LAUNCH_KERNEL(rle_decode_kernel, dim3((unsigned)((n + 255) / 256 > 65535 * 16 ? 65535 * 16 : (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, run_ends,
                     offsets, out, K, H, W, hwk);
  LL_LAUNCH_CHECK("rle_decode");
  return LLMSEG_OK;
}

extern "C" int64_t llmseg_rle_encode_ws_bytes(int32_t K, int32_t H, int32_t W) {
  if (K <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)K * W * ((H + RE_SEG - 1) / RE_SEG) * (int64_t)sizeof(uint4);      // one record per unit
}

extern "C" int llmseg_rle_encode(const uint8_t* masks, int32_t K, int32_t H, int32_t W, uint32_t* counts, int32_t* n_counts, int32_t cap_counts, uint8_t* chars,
                                 int32_t* n_chars, int32_t cap_chars, void* workspace, int64_t workspace_bytes, void* stream) {
  LL_CHECK(masks && counts && n_counts && chars && n_chars && K > 0 && H > 0 && W > 0 && cap_counts > 0 && cap_chars > 0, "rle_encode: bad arguments");
  LL_CHECK((long)H * W < (1L << 31), "rle_encode: H * W must be below 2^31");
  LL_CHECK(workspace && (((uintptr_t)workspace) & 15) == 0 && workspace_bytes >= llmseg_rle_encode_ws_bytes(K, H, W),
           "rle_encode: workspace of llmseg_rle_encode_ws_bytes(K, H, W) bytes, 16-byte aligned");
  const int S = (H + RE_SEG - 1) / RE_SEG, WQ = (W + 3) / 4;
  const long bpm = ((long)S * WQ + 255) / 256, U = (long)W * S;
  LL_CHECK(bpm * K < (1L << 24) && U < (1L << 31), "rle_encode: too many masks for one launch at this size");
  uint4* rec = (uint4*)workspace;
  LL_LAUNCH_KERNEL(rle_walk_kernel<false>, dim3((unsigned)(bpm * K)), dim3(256), 0, (hipStream_t)stream, masks, H, W, S, WQ, (int)bpm, rec, (uint32_t*)nullptr, 0);
  LL_LAUNCH_KERNEL(rle_scan_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, rec, (int)U, n_counts);
  LL_LAUNCH_KERNEL(rle_walk_kernel<true>, dim3((unsigned)(bpm * K)), dim3(256), 0, (hipStream_t)stream, masks, H, W, S, WQ, (int)bpm, rec, counts, cap_counts);
  LL_LAUNCH_KERNEL(rle_chars_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, (const uint4*)rec, (int)U, (const uint32_t*)counts, (const int32_t*)n_counts,
                   cap_counts, chars, n_chars, cap_chars);
  LL_LAUNCH_CHECK("rle_encode");
  return LLMSEG_OK;
}

extern "C" int64_t llmseg_rle_parse_ws_bytes(int32_t K, int64_t total_chars) {
  if (K <= 0 || total_chars < 0) return 0;
  return ((int64_t)K * (int64_t)sizeof(int32_t) + 255) / 256 * 256;      // counts per mask
}

extern "C" int llmseg_rle_parse(const uint8_t* chars, const int64_t* char_offsets, int32_t K, uint32_t* run_ends, int64_t* run_offsets, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  LL_CHECK(chars && char_offsets && run_ends && run_offsets && K > 0, "rle_parse: bad arguments");
  LL_CHECK(workspace && (((uintptr_t)workspace) & 3) == 0 && workspace_bytes >= llmseg_rle_parse_ws_bytes(K, 0), "rle_parse: workspace of llmseg_rle_parse_ws_bytes(K, total) bytes");
  int32_t* n = (int32_t*)workspace;
  LL_LAUNCH_KERNEL(rle_parse_count_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, chars, char_offsets, n);
  LL_LAUNCH_KERNEL(rle_parse_offsets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int32_t*)n, K, run_offsets);
  LL_LAUNCH_KERNEL(rle_parse_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, chars, char_offsets, (const int64_t*)run_offsets, run_ends);
  LL_LAUNCH_CHECK("rle_parse");
  return LLMSEG_OK;
}

extern "C" int llmseg_mask_targets(const uint8_t* segs, const uint8_t* gt, const int32_t* gy, const int32_t* gx, int32_t K, int32_t H, int32_t W, int32_t Hg,
                                   int32_t Wg, int64_t* counts, int64_t* gt_area, double* iou, double* iop, void* stream) {
  LL_CHECK(segs && gt && gy && gx && counts && gt_area && iou && iop && K > 0 && H > 0 && W > 0 && Hg > 0 && Wg > 0, "mask_targets: bad arguments");
  const long n = (long)H * W;
  const unsigned bx = (unsigned)((n + 256 * 16 - 1) / (256 * 16));
  LL_LAUNCH_KERNEL(mask_targets_kernel, dim3(bx < 1 ? 1 : (bx > 256 ? 256 : bx), (unsigned)K), dim3(256), 0, (hipStream_t)stream, segs, gt, gy, gx, H, W, Wg,
                     (unsigned long long*)counts, (unsigned long long*)gt_area);
  LL_LAUNCH_KERNEL(targets_finalize_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)counts,
                     (const unsigned long long*)gt_area, iou, iop, K);
  LL_LAUNCH_CHECK("mask_targets");
  return LLMSEG_OK;
}

extern "C" int llmseg_resize_aa(const uint8_t* segs, void* out, int32_t K, int32_t H, int32_t W, int32_t out_size, const int32_t* y0, const int32_t* ny,
                                const double* wy, const int32_t* x0, const int32_t* nx, const double* wx, int32_t taps, void* stream) {
  LL_CHECK(segs && out && y0 && ny && wy && x0 && nx && wx && K > 0 && H > 0 && W > 0 && out_size > 0 && taps > 0, "resize_aa: bad arguments");
  LL_LAUNCH_KERNEL(resize_aa_kernel, dim3((unsigned)((out_size + 255) / 256), (unsigned)out_size, (unsigned)K), dim3(256), 0, (hipStream_t)stream, segs,
                     (bf16_t*)out, H, W, out_size, y0, ny, wy, x0, nx, wx, taps);
  LL_LAUNCH_CHECK("resize_aa");
  return LLMSEG_OK;
}
