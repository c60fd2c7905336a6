// Sampling for generation (generate(do_sample=True)): temperature, top-k, top-p, the draw, the eos / pad rule and every optional output in
// ONE launch, one workgroup per logits row, no cross-workgroup communication.  The rule is stated in exact arithmetic in
// include/llmseg_hip.h; this file is its fixed-point realisation:
//   * a bf16 logit maps to an order-preserving 16-bit KEY (-0 is +0); T is one positive scalar, so z = l / T is monotone in the key, tie
//     groups are exactly equal keys, and both filters are two-level (high byte, low byte) histogram selects on the key: top-k on COUNTS,
//     top-p on MASS;
//   * the mass of a token is e = expf((l - l_max) / T) (the difference first: it is exact or rounded once, so a huge |l| / T costs nothing)
//     as the INTEGER floor(e * 2^fb) (fb = 40 for V <= 2^22).  Every sum -- per-bin mass, the softmax denominator, the CDF in token-id order --
//     is an integer sum: associative, so LDS integer atomics and any scan order give the same bits.  No floating-point atomics, no
//     floating-point sums at all; thresholds are compared as integers: (1 - p) * S and u * S2 are formed once in fp64 and floored;
//   * a thread owns a CONTIGUOUS range of token ids, so the CDF in id order is a block-wide exclusive scan of per-thread sums and a walk
//     of one thread's range.
// Two paths, one body: V <= 32768 keeps the row's keys (16 packed registers) and masses (32 fp32 registers) of every thread in registers
// and reads the row once; larger V re-reads the row from global memory (L2) on every pass.
#include "common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int ST = 1024;                  // threads per workgroup
constexpr int RC = 32;                    // register path: ids per thread (ST * RC = 32768)
constexpr uint32_t KEY_NEG_INF = 0x007fu; // key of -inf; smaller keys are negative NaNs
constexpr uint32_t NOT_FOUND = 256u;

__device__ __forceinline__ uint32_t key_of(bf16_t b) {
  uint32_t v = b;
  if (v == 0x8000u) v = 0u;                                        // -0 == +0: one tie group
  return (v & 0x8000u) ? (~v & 0xffffu) : (v | 0x8000u);
}
__device__ __forceinline__ float val_of_key(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __uint_as_float(b << 16);
}
__device__ __forceinline__ float weight_of(uint32_t k, float vmax, float T) { return expf(__fdiv_rn(val_of_key(k) - vmax, T)); }
__device__ __forceinline__ u64 mass_of(float e, float mscale) { return e > 0.f ? (u64)(e * mscale) : 0ull; }      // e <= 1: e * 2^fb is exact; NaN -> 0

__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_incl_scan(u64 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = shfl_up64(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
// exclusive scan of one u64 per thread over the workgroup, in thread order; total = the sum of all.  `ws` is 16 u64 of LDS.
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* ws, u64& total) {
  const u64 inc = wave_incl_scan(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 63) ws[w] = inc;
  __syncthreads();
  u64 off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < ST / 64; ++i) {
    const u64 s = ws[i];
    if (i < w) off += s;
    tot += s;
  }
  total = tot;
  return off + inc - v;
}
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, u64* ws) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < ST / 64; ++i) t = max(t, (uint32_t)ws[i]);
  return t;
}
// First bin, in scan order (descending bins when `desc`), whose inclusive running sum of hist[] exceeds `target`: -> sel[0] = the bin
// (NOT_FOUND when the total does not exceed target), sel[1] = the sum of the bins before it.  Wave 0 scans (4 bins a lane); hist[] must be
// complete (a barrier before the call); the result is visible to every thread on return.
__device__ __forceinline__ void select_bin(const u64* hist, u64 target, bool desc, u64* sel) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    u64 h[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pos = 4 * lane + i;
      h[i] = hist[desc ? 255 - pos : pos];
      s += h[i];
    }
    const u64 inc = wave_incl_scan(s);
    u64 c = inc - s;
    if (inc > target && c <= target) {                              // the crossing is in this lane's four bins: one lane at most
      bool done = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!done && c + h[i] > target) {
          const int pos = 4 * lane + i;
          sel[0] = (u64)(desc ? 255 - pos : pos);
          sel[1] = c;
          done = true;
        }
        if (!done) c += h[i];
      }
    }
    if (lane == 63 && inc <= target) {
      sel[0] = NOT_FOUND;
      sel[1] = inc;
    }
  }
  __syncthreads();
}

struct SampleP {
  const bf16_t* logits; long ldl; int V;
  float T; int k; float p; float mscale;
  const float* u; long eos, pad;
  int64_t* unfinished; int64_t* next; float* logprob; int32_t* kept; float* probs; long ldp;
};

template <bool REG>
__global__ __launch_bounds__(ST) void sample_tokens_kernel(SampleP a) {
  __shared__ u64 hist[256];
  __shared__ u64 ws[ST / 64];
  __shared__ u64 sel[2];
  __shared__ int s_tok, s_last, s_cnt;
  __shared__ float s_lp;
  const int tid = threadIdx.x, V = a.V;
  const long n = blockIdx.x;
  const bf16_t* __restrict__ row = a.logits + n * a.ldl;
  // thread t owns the ids [base, base + nvalid): a contiguous range, so thread order is token-id order
  const int C = REG ? min(RC, max(8, (((V + ST - 1) / ST) + 7) & ~7)) : (V + ST - 1) / ST;
  const long base = (long)tid * C;
  const int nvalid = (int)max(0L, min((long)C, (long)V - base));
  uint32_t kreg[RC / 2];
  float ef[RC];
  if constexpr (REG) {
    const bool vec = (((uintptr_t)row) & 15) == 0;
#pragma unroll
    for (int q = 0; q < RC / 8; ++q) {
      if (vec && 8 * q + 8 <= nvalid) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + base + 8 * q);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) kreg[4 * q + i] = key_of((bf16_t)(w[i] & 0xffffu)) | (key_of((bf16_t)(w[i] >> 16)) << 16);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 8 * q + 2 * i;
          const uint32_t lo = j < nvalid ? key_of(row[base + j]) : 0u, hi = j + 1 < nvalid ? key_of(row[base + j + 1]) : 0u;
          kreg[4 * q + i] = lo | (hi << 16);
        }
      }
    }
  }
  // f(j, key, e): every owned id in ascending order; e = its softmax weight relative to the row maximum (valid once `vmax` is set)
  float vmax = 0.f;
  auto each = [&](auto&& f) {
    if constexpr (REG) {
#pragma unroll
      for (int j = 0; j < RC; ++j)
        if (j < nvalid) f(j, (kreg[j >> 1] >> (16 * (j & 1))) & 0xffffu, ef[j]);
    } else {
      for (int j = 0; j < nvalid; ++j) {
        const uint32_t k = key_of(row[base + j]);
        f(j, k, weight_of(k, vmax, a.T));
      }
    }
  };
  auto zero_hist = [&]() {
    __syncthreads();                                                // every reader of hist[] / sel[] is done
    if (tid < 256) hist[tid] = 0ull;
    __syncthreads();
  };

  uint32_t kmax = 0u;
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < RC; ++j)
      if (j < nvalid) kmax = max(kmax, (kreg[j >> 1] >> (16 * (j & 1))) & 0xffffu);
  } else {
    for (int j = 0; j < nvalid; ++j) kmax = max(kmax, key_of(row[base + j]));
  }
  kmax = block_max_u32(kmax, ws);
  vmax = val_of_key(kmax);
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < RC; ++j) ef[j] = j < nvalid ? weight_of((kreg[j >> 1] >> (16 * (j & 1))) & 0xffffu, vmax, a.T) : 0.f;
  }
  if (tid == 0) { s_tok = -1; s_last = -1; s_cnt = 0; s_lp = 0.f; }

  // ---- top-k: the k-th largest key, by count ----
  uint32_t tk = 0u;
  if (a.k >= 1 && a.k < V) {
    zero_hist();
    each([&](int, uint32_t k, float) { atomicAdd(&hist[k >> 8], 1ull); });
    __syncthreads();
    select_bin(hist, (u64)(a.k - 1), true, sel);
    const uint32_t bh = (uint32_t)sel[0];
    const u64 before = sel[1];
    zero_hist();
    each([&](int, uint32_t k, float) { if ((k >> 8) == bh) atomicAdd(&hist[k & 255u], 1ull); });
    __syncthreads();
    select_bin(hist, (u64)(a.k - 1) - before, true, sel);
    tk = (bh << 8) | ((uint32_t)sel[0] & 255u);
  }
  if (kmax > KEY_NEG_INF && tk <= KEY_NEG_INF) tk = KEY_NEG_INF + 1u;      // -inf is never kept while anything larger exists

  // ---- top-p: the smallest key whose cumulative mass from below exceeds (1 - p) * S ----
  uint32_t t2 = tk;
  if (a.p < 1.f) {
    zero_hist();
    u64 mine = 0;
    each([&](int, uint32_t k, float e) {
      if (k >= tk) {
        const u64 m = mass_of(e, a.mscale);
        mine += m;
        if (m) atomicAdd(&hist[k >> 8], m);
      }
    });
    u64 S;
    block_excl_scan(mine, ws, S);                                   // (its barriers also complete hist[])
    const u64 target = (u64)((1.0 - (double)a.p) * (double)S);
    select_bin(hist, target, false, sel);
    const uint32_t bh = (uint32_t)sel[0];
    const u64 before = sel[1];
    if (bh != NOT_FOUND) {                                          // (S == 0 only on a row without a finite maximum: keep K1)
      zero_hist();
      each([&](int, uint32_t k, float e) {
        if (k >= tk && (k >> 8) == bh) {
          const u64 m = mass_of(e, a.mscale);
          if (m) atomicAdd(&hist[k & 255u], m);
        }
      });
      __syncthreads();
      select_bin(hist, target - before, false, sel);
      if ((uint32_t)sel[0] != NOT_FOUND) t2 = max(tk, (bh << 8) | ((uint32_t)sel[0] & 255u));
    }
  }

  // ---- the draw: CDF over K2 = {key >= t2} in token-id order ----
  u64 mine = 0;
  int cnt = 0, last = -1;
  each([&](int j, uint32_t k, float e) {
    if (k >= t2) {
      mine += mass_of(e, a.mscale);
      ++cnt;
      last = (int)(base + j);
    }
  });
  u64 S2;
  const u64 exc = block_excl_scan(mine, ws, S2);
  if (cnt) atomicAdd(&s_cnt, cnt);
  if (last >= 0) atomicMax(&s_last, last);
  float u = a.u[n];
  u = u >= 0.f ? fminf(u, 0.99999994f) : 0.f;                       // the interface asks for [0, 1); anything else (NaN too) is clamped into it
  const u64 tt = (u64)((double)u * (double)S2);
  const double rinv = S2 ? 1.0 / (double)S2 : 0.0;
  if (exc <= tt && tt < exc + mine) {                               // one thread at most
    u64 c = exc;
    bool done = false;
    each([&](int j, uint32_t k, float e) {
      if (!done && k >= t2) {
        const u64 m = mass_of(e, a.mscale);
        c += m;
        if (c > tt) {
          s_tok = (int)(base + j);
          s_lp = (float)log((double)m * rinv);
          done = true;
        }
      }
    });
  }
  if (a.probs) {
    float* pr = a.probs + n * a.ldp + base;
    each([&](int j, uint32_t k, float e) { pr[j] = k >= t2 ? (float)((double)mass_of(e, a.mscale) * rinv) : 0.f; });
  }
  __syncthreads();
  if (tid == 0) {
    long tok = s_tok;
    float lp = s_lp;
    if (tok < 0) {                                                  // rounding left no crossing: the largest index of K2
      tok = s_last >= 0 ? s_last : V - 1;
      lp = (float)log((double)mass_of(weight_of(key_of(row[tok]), vmax, a.T), a.mscale) * rinv);
    }
    if (a.eos >= 0) {                                               // the greedy loop's rule: a finished row emits pad; a row finishes on eos
      const long uf = a.unfinished ? (long)a.unfinished[n] : 1L;
      if (!uf) { tok = a.pad; lp = 0.f; }
      if (a.unfinished) a.unfinished[n] = (uf && tok != a.eos) ? 1 : 0;
    }
    a.next[n] = tok;
    if (a.logprob) a.logprob[n] = lp;
    if (a.kept) a.kept[n] = s_cnt;
  }
}

}  // namespace

extern "C" int llmseg_sample_tokens(const void* logits, int64_t ldl, int64_t N, int64_t V, float temperature, int32_t top_k, float top_p, const float* u,
                                    int64_t eos, int64_t pad, int64_t* unfinished, int64_t* next, float* logprob, int32_t* kept, float* probs, int64_t ldp,
                                    void* stream) {
  LL_CHECK(logits && u && next, "sample_tokens: null pointer (logits, u and next are required)");
  LL_CHECK(N >= 1 && N <= 0x7fffffffL && V >= 1 && V <= 0x7fffffffL, "sample_tokens: need 1 <= N, V < 2^31 (N = %ld, V = %ld)", (long)N, (long)V);
  LL_CHECK(ldl >= V, "sample_tokens: ldl %ld < V %ld", (long)ldl, (long)V);
  LL_CHECK(isfinite(temperature) && temperature > 0.f, "sample_tokens: temperature must be finite and > 0, got %g", (double)temperature);
  LL_CHECK(top_k >= 0, "sample_tokens: top_k must be >= 0 (0 = off), got %d", (int)top_k);
  LL_CHECK(top_p > 0.f && top_p <= 1.f, "sample_tokens: top_p must be in (0, 1] (1 = off), got %g", (double)top_p);
  LL_CHECK(!probs || ldp >= V, "sample_tokens: ldp %ld < V %ld", (long)ldp, (long)V);
  LL_CHECK(((uintptr_t)logits & 1) == 0 && ((uintptr_t)u & 3) == 0 && ((uintptr_t)logprob & 3) == 0 && ((uintptr_t)kept & 3) == 0 && ((uintptr_t)probs & 3) == 0 &&
               ((uintptr_t)next & 7) == 0 && ((uintptr_t)unfinished & 7) == 0,
           "sample_tokens: a pointer is not aligned to its element type");
  int bits = 0;
  while ((V >> bits) != 0) ++bits;                                  // V < 2^bits
  const int fb = bits <= 22 ? 40 : 62 - bits;                       // V * 2^fb < 2^62: the integer sums cannot overflow
  SampleP a;
  a.logits = (const bf16_t*)logits; a.ldl = ldl; a.V = (int)V;
  a.T = temperature; a.k = top_k; a.p = top_p; a.mscale = ldexpf(1.f, fb);
  a.u = u; a.eos = eos; a.pad = pad;
  a.unfinished = unfinished; a.next = next; a.logprob = logprob; a.kept = kept; a.probs = probs; a.ldp = ldp;
  if (V <= (int64_t)ST * RC) LL_LAUNCH_KERNEL(sample_tokens_kernel<true>, dim3((unsigned)N), dim3(ST), 0, (hipStream_t)stream, a);
  else LL_LAUNCH_KERNEL(sample_tokens_kernel<false>, dim3((unsigned)N), dim3(ST), 0, (hipStream_t)stream, a);
  LL_LAUNCH_CHECK("sample_tokens");
  return LLMSEG_OK;
}
