// Beam search for generation (generate(num_beams >= 2)): the pick.  (The decode-step attention over the KV cache that is never moved,
// llmseg_decode_attn_beams, is decode_attn.hip's one kernel with its table instance; the table it reads is re-ordered here.)
//   * llmseg_beam_step is the pick, in two launches.  (1) one workgroup per logits row: the row maximum, the softmax denominator as an INTEGER sum
//     (the device of sample.hip), the score of every candidate and the row's best 2B by (score descending, flat index ascending) as 64-bit keys.
//     (2) one workgroup per prompt: the best 2B of the rows' B * 2B keys, the walk of include/llmseg_hip.h's rule, and the table's re-ordering.
//     No floating-point atomics, no floating-point sum at all: a pure function of its inputs.
#include "common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;

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
