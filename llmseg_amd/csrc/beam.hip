// Beam search for generation (generate(num_beams >= 2)): the decode-step attention over a KV cache that is never moved, and the pick.
//   * llmseg_decode_attn_beams is attention.hip's decode_attn_kernel with ONE change: key t < pos of row r is read from the physical cache row
//     src[r][t] (an int32 table, a few KB) instead of row r.  A beam's history then lives wherever its ancestors wrote it, and re-ordering the beams
//     re-orders the table, not 32 layers of K and V.  Everything else -- RoPE, the append to [r][pos], the split count, the 16-lane key groups, the
//     trip of 64 keys, the online softmax, the merge -- is copied, so a table that names every row's own row gives the bits of llmseg_decode_attn_rows.
//     The table entry of a key is uniform over the 16 lanes that own the key: one 4-byte load per lane (the lanes of a group hit one address), issued with the
//     trip's K and V requests; no LDS stage.
//   * llmseg_beam_step is the pick, in two launches.  (1) one workgroup per logits row: the row maximum, the softmax denominator as an INTEGER sum
//     (the device of sample.hip), the score of every candidate and the row's best 2B by (score descending, flat index ascending) as 64-bit keys.
//     (2) one workgroup per prompt: the best 2B of the rows' B * 2B keys, the walk of include/llmseg_hip.h's rule, and the table's re-ordering.
//     No floating-point atomics, no floating-point sum at all: a pure function of its inputs.
#include "common.h"
#include <math.h>
#include <algorithm>

namespace {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------------- attention
struct DecBP {
  const bf16_t* qkv; long ld;
  const float *cs, *sn;
  bf16_t *kc, *vc; long cstride;
  const int32_t* pos_dev;
  const int32_t* src; long ld_src;
  int heads, splits;
  float scale;
  bf16_t* out; long ldo;
  float* part;                                         // [R][heads][splits][130]: 128 unnormalised outputs, running max, running sum
};

__global__ __launch_bounds__(256) void decode_attn_beams_kernel(DecBP p) {
  constexpr int HD = 128, UN = 4;
  __shared__ float qs[HD];
  __shared__ __align__(16) bf16_t knew[HD], vnew[HD];
  __shared__ float red[4][HD], rm[4], rl[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, c = tid & 15;
  const int h = blockIdx.x / p.splits, sp = blockIdx.x - h * p.splits, n = blockIdx.y;
  const long D = (long)p.heads * HD;
  const int pos = p.pos_dev[n], nk = pos + 1;           // workgroup-uniform: a scalar load
  const int per = ((nk + p.splits - 1) / p.splits + 15) & ~15;
  const int j0 = sp * per, j1 = min(nk, j0 + per);
  const bool owner = pos >= j0 && pos < j1;              // the workgroup whose key range holds the new token appends it
  const bf16_t* row = p.qkv + (long)n * p.ld + (long)h * HD;
  bf16_t* kb = p.kc + (long)n * p.cstride + (long)h * HD;      // the row's OWN physical row: the append
  bf16_t* vb = p.vc + (long)n * p.cstride + (long)h * HD;
  const bf16_t* kh = p.kc + (long)h * HD;                       // physical row 0: the reads add src[n][t] * cstride
  const bf16_t* vh = p.vc + (long)h * HD;
  const int32_t* srow = p.src + (long)n * p.ld_src;
  if (tid < 128) {
    const int i = tid & 63;
    if (tid < 64 || owner) {
      const bf16_t* src = row + (tid < 64 ? 0 : D);
      const float a = bf2f(src[i]), b = bf2f(src[i + 64]);
      const float cv = p.cs[(long)pos * 64 + i], sv = p.sn[(long)pos * 64 + i];
      const bf16_t o1 = f2bf(rope_lo(a, b, cv, sv)), o2 = f2bf(rope_hi(a, b, cv, sv));
      if (tid < 64) { qs[i] = bf2f(o1); qs[i + 64] = bf2f(o2); }
      else {
        knew[i] = o1; knew[i + 64] = o2;
        kb[(long)pos * D + i] = o1; kb[(long)pos * D + i + 64] = o2;
      }
    }
  } else if (tid < 192 && owner) {
    const int i = tid - 128;
    const bf16_t v1 = row[2 * D + i], v2 = row[2 * D + i + 64];
    vnew[i] = v1; vnew[i + 64] = v2;
    vb[(long)pos * D + i] = v1; vb[(long)pos * D + i + 64] = v2;
  }
  __syncthreads();
  float q[8], acc[8], m = -1e30f, l = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) { q[e] = qs[c * 8 + e]; acc[e] = 0.f; }
  for (int jb = j0; jb < j1; jb += 16 * UN) {
    uint4 kk[UN], vv[UN];
    long phys[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {                      // the trip's table entries first: the K and V addresses wait for them
      const int j = jb + u * 16 + g;
      phys[u] = (j < j1 && j != pos) ? (long)srow[j] : 0L;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = jb + u * 16 + g;
      kk[u] = make_uint4(0, 0, 0, 0); vv[u] = kk[u];
      if (j < j1) {
        if (j == pos) { kk[u] = *reinterpret_cast<const uint4*>(knew + c * 8); vv[u] = *reinterpret_cast<const uint4*>(vnew + c * 8); }
        else {
          const long off = phys[u] * p.cstride + (long)j * D + c * 8;
          kk[u] = *reinterpret_cast<const uint4*>(kh + off); vv[u] = *reinterpret_cast<const uint4*>(vh + off);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = jb + u * 16 + g;
      float kf[8], vf[8], s = 0.f;
      unpack8(kk[u], kf);
      unpack8(vv[u], vf);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(q[e], kf[e], s);
      s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
      const bool valid = j < j1;
      s = valid ? s * p.scale : -1e30f;
      const float mn = fmaxf(m, s), corr = __expf(m - mn), pj = valid ? __expf(s - mn) : 0.f;
      l = l * corr + pj;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = acc[e] * corr + pj * vf[e];
      m = mn;
    }
  }
  // the four key groups of a wave, then the four waves
  float mw = fmaxf(m, __shfl_xor(m, 16));
  mw = fmaxf(mw, __shfl_xor(mw, 32));
  const float f = __expf(m - mw);
  l *= f; l += __shfl_xor(l, 16); l += __shfl_xor(l, 32);
#pragma unroll
  for (int e = 0; e < 8; ++e) { float a = acc[e] * f; a += __shfl_xor(a, 16); a += __shfl_xor(a, 32); acc[e] = a; }
  if (lane < 16) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][c * 8 + e] = acc[e];
    if (lane == 0) { rm[wave] = mw; rl[wave] = l; }
  }
  __syncthreads();
  if (tid < HD) {
    const float M = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
    float L = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const float e = __expf(rm[w] - M); L += e * rl[w]; o += e * red[w][tid]; }
    if (p.splits == 1) p.out[(long)n * p.ldo + (long)h * HD + tid] = f2bf(o / L);
    else {
      float* pp = p.part + (((long)n * p.heads + h) * p.splits + sp) * 130;
      pp[tid] = o;
      if (tid == 0) { pp[128] = M; pp[129] = L; }
    }
  }
}

// attention.hip's decode_attn_merge_kernel, copied (a kernel cannot be launched across translation units without relocatable device code)
__global__ __launch_bounds__(128) void decode_attn_beams_merge_kernel(const float* __restrict__ part, int heads, int splits, bf16_t* __restrict__ out, long ldo) {
  const int h = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const float* pp = part + ((long)n * heads + h) * splits * 130;
  float mv[16], lv[16], ov[16], M = -1e30f;            // every partial requested before the first use: one memory round trip
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int sc = min(s, splits - 1);
    mv[s] = pp[sc * 130 + 128]; lv[s] = pp[sc * 130 + 129]; ov[s] = pp[sc * 130 + tid];
  }
#pragma unroll
  for (int s = 0; s < 16; ++s) M = fmaxf(M, mv[s]);
  float L = 0.f, o = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float e = s < splits ? __expf(mv[s] - M) : 0.f;
    L += e * lv[s]; o += e * ov[s];
  }
  out[(long)n * ldo + (long)h * 128 + tid] = f2bf(o / L);
}

// --------------------------------------------------------------------------------------------------------------------------- pick
constexpr int BT = 1024;                  // threads per workgroup of the row kernel
constexpr int MAXB = 16;                  // beams
constexpr int FB = 40;                    // a weight e <= 1 is held as floor(e * 2^FB); V <= 2^22 keeps every sum below 2^63

__device__ __forceinline__ float logit_of(bf16_t b) { return bf2f(b); }
// order-preserving 32-bit key of an fp32 score (a larger score has a larger key; -0 is +0)
__device__ __forceinline__ uint32_t skey_of(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_of_skey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// candidate key: score first, then the SMALLER flat index b * V + v (flat < 2^31)
__device__ __forceinline__ u64 ckey(float score, uint32_t flat) { return ((u64)skey_of(score) << 32) | (u64)(0xffffffffu - flat); }

__device__ __forceinline__ u64 shfl_xor64(u64 v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
// block-wide reductions over BT threads, the result visible to every thread; `ws` is BT / 64 u64 of LDS
__device__ __forceinline__ u64 block_max64(u64 v, u64* ws) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const u64 t = shfl_xor64(v, o); v = t > v ? t : v; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 t = 0;
#pragma unroll
  for (int i = 0; i < BT / 64; ++i) t = ws[i] > t ? ws[i] : t;
  return t;
}
__device__ __forceinline__ u64 block_sum64(u64 v, u64* ws) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor64(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 t = 0;
#pragma unroll
  for (int i = 0; i < BT / 64; ++i) t += ws[i];
  return t;
}

// the score of candidate v of a row, as include/llmseg_hip.h states it: three fp32 operations, each rounded once
__device__ __forceinline__ float cand_score(float l, float lmax, float lse, float s) { return __fadd_rn(s, __fsub_rn(__fsub_rn(l, lmax), lse)); }

// (1) one workgroup per logits row (n, b): -> keys[row][0 .. 2B): the row's best 2B candidates, best first
__global__ __launch_bounds__(BT) void beam_rows_kernel(const bf16_t* __restrict__ logits, long ldl, int V, const float* __restrict__ beam_scores, const int32_t* __restrict__ done,
                                                       int beams_in, int K2, u64* __restrict__ keys) {
  __shared__ u64 ws[BT / 64];
  const int tid = threadIdx.x;
  const long r = blockIdx.x;
  const int n = (int)(r / beams_in), b = (int)(r - (long)n * beams_in);
  if (done[n]) return;                                              // workgroup-uniform: a done prompt's rows contribute nothing
  const bf16_t* __restrict__ row = logits + r * ldl;
  const float s = beam_scores[r];
  // the row maximum (NaN logits are skipped by fmaxf: such a row's result is unspecified but in range)
  float mx = -INFINITY;
  for (int v = tid; v < V; v += BT) mx = fmaxf(mx, logit_of(row[v]));
  const float lmax = score_of_skey((uint32_t)block_max64((u64)skey_of(mx), ws));
  // the denominator: an integer sum, so the order of the terms does not matter
  u64 mine = 0;
  for (int v = tid; v < V; v += BT) {
    const float e = expf(__fsub_rn(logit_of(row[v]), lmax));
    mine += e > 0.f ? (u64)(e * 1099511627776.f) : 0ull;           // e <= 1: e * 2^40 is exact; NaN -> 0
  }
  const u64 S = block_sum64(mine, ws);
  const float lse = (float)(log((double)S) - (double)FB * 0.69314718055994530942);
  // this thread's best candidate below `prev` (keys are distinct: the flat index is part of them); rescanned only when it was taken
  const uint32_t flat0 = (uint32_t)b * (uint32_t)V;
  auto best_below = [&](u64 prev) {
    u64 best = 0;
    for (int v = tid; v < V; v += BT) {
      const u64 k = ckey(cand_score(logit_of(row[v]), lmax, lse, s), flat0 + (uint32_t)v);
      if (k < prev && k > best) best = k;
    }
    return best;
  };
  u64 prev = ~0ull, local = best_below(prev);
  for (int i = 0; i < K2; ++i) {
    const u64 top = block_max64(local, ws);
    if (tid == 0) keys[r * K2 + i] = top;
    if (local == top && top != 0) local = best_below(top);
    prev = top;
  }
}

struct StepP {
  const u64* keys;
  const float* beam_scores; const int32_t* done;
  long eos, pad;
  const int32_t* src_in; int32_t* src_out; long ld_src;
  const int32_t* pos_rows;
  int B, beams_in, V;
  int64_t* next_token; int32_t* parent; float* next_scores; float* step_best; int32_t* fin_count; int32_t* fin_parent; float* fin_score;
};

// (2) one workgroup per prompt: rank the beams_in * 2B keys, walk the best 2B, re-order the table
__global__ __launch_bounds__(512) void beam_pick_kernel(StepP a) {
  __shared__ u64 all[2 * MAXB * MAXB];
  __shared__ u64 top[2 * MAXB];
  __shared__ int s_parent[MAXB];
  const int tid = threadIdx.x, n = blockIdx.x, B = a.B, K2 = 2 * B, nc = a.beams_in * K2;
  const long r0 = (long)n * B;
  const bool fin = a.done[n] != 0;                                  // workgroup-uniform
  if (!fin) {
    const u64 mykey = tid < nc ? a.keys[(long)n * nc + tid] : 0ull;
    all[tid] = mykey;
    __syncthreads();
    if (tid < nc) {                                                 // keys are distinct: the rank is the count of larger keys
      int rank = 0;
      for (int j = 0; j < nc; ++j) rank += all[j] > mykey;
      if (rank < K2) top[rank] = mykey;
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (fin) {                                                      // a done prompt: pad, parent = own slot, scores unchanged
      for (int i = 0; i < B; ++i) {
        const int j = min(i, a.beams_in - 1);
        a.next_token[r0 + i] = a.pad; a.parent[r0 + i] = j; a.next_scores[r0 + i] = a.beam_scores[(long)n * a.beams_in + j];
        s_parent[i] = j;
      }
      a.step_best[n] = 0.f; a.fin_count[n] = 0;
    } else {
      int live = 0, nf = 0;
      for (int k = 0; k < K2; ++k) {
        const u64 key = top[k];
        const float sc = score_of_skey((uint32_t)(key >> 32));
        const uint32_t flat = 0xffffffffu - (uint32_t)key;
        int b = (int)(flat / (uint32_t)a.V);
        b = min(b, a.beams_in - 1);                                 // (in range whatever a NaN row left in the key)
        const long v = (long)(flat - (uint32_t)b * (uint32_t)a.V);
        if (k == 0) a.step_best[n] = sc;
        if (a.eos >= 0 && v == a.eos) {
          if (k < B) { a.fin_parent[r0 + nf] = b; a.fin_score[r0 + nf] = sc; ++nf; }      // an eos of rank >= B is dropped
        } else if (live < B) {
          a.next_token[r0 + live] = min(v, (long)a.V - 1); a.parent[r0 + live] = b; a.next_scores[r0 + live] = sc;
          s_parent[live] = b;
          ++live;
        }
      }
      a.fin_count[n] = nf;
    }
  }
  __syncthreads();
  // the table: row i inherits its parent's history and learns where the parent wrote the key of the token it was just fed
  for (int i = 0; i < B; ++i) {
    const long r = r0 + i;
    const int p = min(a.pos_rows[r], (int)a.ld_src);
    int32_t* o = a.src_out + r * a.ld_src;
    if (a.beams_in == 1) {                                          // first pick: every prompt key lives in physical row n * B
      for (int t = tid; t < p; t += 512) o[t] = (int32_t)r0;
    } else {
      const long pr = r0 + s_parent[i];
      const int32_t* in = a.src_in + pr * a.ld_src;
      for (int t = tid; t < p - 1; t += 512) o[t] = in[t];
      if (tid == 0 && p >= 1) o[p - 1] = (int32_t)pr;
    }
  }
}

}  // namespace

extern "C" int llmseg_decode_attn_beams(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                        const int32_t* pos_rows_dev, const int32_t* src, int64_t ld_src, int64_t capacity, int64_t N, int32_t heads,
                                        int32_t head_dim, float scale, void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream) {
  LL_CHECK(qkv && cos && sin && kcache && vcache && pos_rows_dev && out && N > 0 && N < 65536 && heads > 0, "decode_attn_beams: bad arguments");
  LL_CHECK(head_dim == 128, "decode_attn_beams: head_dim 128 only");
  LL_CHECK((ld & 7) == 0 && (cache_stride_n & 7) == 0 && AL16(qkv) && AL16(kcache) && AL16(vcache), "decode_attn_beams: 16-byte alignment required");
  LL_CHECK(src && ((uintptr_t)src & 3) == 0, "decode_attn_beams: src must be a 4-byte aligned int32 table");
  LL_CHECK(capacity > 0 && ld_src >= capacity, "decode_attn_beams: ld_src %ld < capacity %ld", (long)ld_src, (long)capacity);
  int splits = 1;
  if (scratch) {
    splits = (int)std::min<int64_t>(16, std::max<int64_t>(1, 256 / (N * heads)));
    while (splits > 1 && (int64_t)N * heads * splits * 130 * 4 > scratch_bytes) --splits;
  }
  DecBP p{(const bf16_t*)qkv, (long)ld, cos, sin, (bf16_t*)kcache, (bf16_t*)vcache, (long)cache_stride_n, pos_rows_dev, src, (long)ld_src, heads, splits, scale,
          (bf16_t*)out, (long)ldo, (float*)scratch};
  LL_LAUNCH_KERNEL(decode_attn_beams_kernel, dim3(heads * splits, (unsigned)N), dim3(256), 0, (hipStream_t)stream, p);
  LL_LAUNCH_CHECK("decode_attn_beams");
  if (splits > 1) {
    LL_LAUNCH_KERNEL(decode_attn_beams_merge_kernel, dim3(heads, (unsigned)N), dim3(128), 0, (hipStream_t)stream, (const float*)scratch, heads, splits,
                     (bf16_t*)out, (long)ldo);
    LL_LAUNCH_CHECK("decode_attn_beams_merge");
  }
  return LLMSEG_OK;
}

extern "C" int llmseg_beam_step(const void* logits, int64_t ldl, const float* beam_scores, const int32_t* done, int64_t eos, int64_t pad, const int32_t* src_in,
                                int32_t* src_out, int64_t ld_src, const int32_t* pos_rows, int64_t N, int32_t B, int32_t beams_in, int64_t V, int64_t* next_token,
                                int32_t* parent, float* next_scores, float* step_best, int32_t* fin_count, int32_t* fin_parent, float* fin_score, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  LL_CHECK(logits && beam_scores && done && src_in && src_out && pos_rows && next_token && parent && next_scores && step_best && fin_count && fin_parent && fin_score &&
               workspace, "beam_step: null pointer");
  LL_CHECK(src_in != src_out, "beam_step: src_in == src_out (one row's copy would read another row's output)");
  LL_CHECK(B >= 2 && B <= MAXB, "beam_step: need 2 <= B <= 16, got %d", (int)B);
  LL_CHECK(beams_in == 1 || beams_in == B, "beam_step: beams_in must be 1 or B = %d, got %d", (int)B, (int)beams_in);
  LL_CHECK(N >= 1 && N * (int64_t)B <= 0x7fffffffL, "beam_step: need 1 <= N and N * B < 2^31 (N = %ld)", (long)N);
  LL_CHECK(V >= 2 * (int64_t)B && V <= (1L << 22), "beam_step: need 2 B <= V <= 2^22 (V = %ld, B = %d)", (long)V, (int)B);
  LL_CHECK(ldl >= V, "beam_step: ldl %ld < V %ld", (long)ldl, (long)V);
  LL_CHECK(ld_src >= 1, "beam_step: ld_src %ld < 1", (long)ld_src);
  LL_CHECK(eos < V && pad >= 0, "beam_step: eos %ld must be < V (negative = none) and pad %ld >= 0", (long)eos, (long)pad);
  LL_CHECK(workspace_bytes >= N * (int64_t)beams_in * 2 * B * 8, "beam_step: workspace %ld < N * beams_in * 2 B * 8 = %ld bytes", (long)workspace_bytes,
           (long)(N * (int64_t)beams_in * 2 * B * 8));
  LL_CHECK(((uintptr_t)logits & 1) == 0 && (((uintptr_t)beam_scores | (uintptr_t)done | (uintptr_t)src_in | (uintptr_t)src_out | (uintptr_t)pos_rows | (uintptr_t)parent |
                                              (uintptr_t)next_scores | (uintptr_t)step_best | (uintptr_t)fin_count | (uintptr_t)fin_parent | (uintptr_t)fin_score) & 3) == 0 &&
               (((uintptr_t)next_token | (uintptr_t)workspace) & 7) == 0,
           "beam_step: a pointer is not aligned to its element type");
  LL_LAUNCH_KERNEL(beam_rows_kernel, dim3((unsigned)(N * beams_in)), dim3(BT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ldl, (int)V, beam_scores, done,
                   (int)beams_in, 2 * (int)B, (u64*)workspace);
  LL_LAUNCH_CHECK("beam_rows");
  StepP a{(const u64*)workspace, beam_scores, done, (long)eos, (long)pad, src_in, src_out, (long)ld_src, pos_rows, (int)B, (int)beams_in, (int)V,
          next_token, parent, next_scores, step_best, fin_count, fin_parent, fin_score};
  LL_LAUNCH_KERNEL(beam_pick_kernel, dim3((unsigned)N), dim3(512), 0, (hipStream_t)stream, a);
  LL_LAUNCH_CHECK("beam_pick");
  return LLMSEG_OK;
}
