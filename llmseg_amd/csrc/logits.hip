// Logits processors for generation (generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=)): the append of the token a
// row was just given to its device-side history, the repetition penalty, the n-gram ban, the eos ban and the suppress list in ONE launch, one workgroup
// per logits row, in place.  The rule is stated in include/llmseg_hip.h.  The launch touches the O(len) affected logits only, never the whole row.
//   * the history (at most LLMSEG_LOGITS_HIST_CAP ids) goes to LDS once; thread t owns positions t, t + 1024, ...;
//   * the penalty must hit a token ONCE however often it occurs: every thread loads the ORIGINAL logit of each of its positions and forms f(original)
//     in registers, a barrier follows, then every thread stores: duplicates store the same bits.  The whole history is loaded before the first store
//     (the cap sizes the register array): a loop that stored between chunks would penalise a token of two chunks twice;
//   * the -inf writes (n-gram ban, ban_token, suppress list) come after a second barrier, so they win over a penalised value at the same id.
// No floating-point atomics, no sums: the result is a pure function of the inputs.
#include "common.h"
#include <math.h>

namespace {

constexpr int LT = 1024;                              // threads per workgroup
constexpr int CAP = LLMSEG_LOGITS_HIST_CAP;
constexpr int HP = CAP / LT;                          // history positions per thread
constexpr bf16_t BF_NEG_INF = 0xff80u;
static_assert(CAP % LT == 0, "the history cap is a whole number of positions per thread");

struct LogitsP {
  bf16_t* logits; long ldl; int V;
  int64_t* hist; long ld_hist; int32_t* hist_len; const int64_t* append;
  float theta; int g; long ban; const int32_t* suppress; long n_suppress;
};

// bf16(fl32(l) * theta) for l < 0, bf16(fl32(l) / theta) otherwise (-0, NaN: the division), rounded to nearest even; a NaN is the canonical quiet NaN
__device__ __forceinline__ bf16_t penalised(bf16_t l, float theta) {
  const float x = bf2f(l);
  const float y = x < 0.f ? x * theta : __fdiv_rn(x, theta);
  return y != y ? (bf16_t)0x7fc0u : f2bf(y);
}

__global__ __launch_bounds__(LT) void logits_process_kernel(LogitsP a) {
  __shared__ int64_t h[CAP];
  const int tid = threadIdx.x, V = a.V;
  const long n = blockIdx.x;
  bf16_t* row = a.logits + n * a.ldl;
  int64_t* hrow = a.hist + n * a.ld_hist;
  const int cap = (int)a.ld_hist;                     // <= CAP (checked on the host)
  const int old = min(max(a.hist_len[n], 0), cap);
  const bool app = a.append != nullptr && old < cap;  // a full row drops the append and does not count it
  const int64_t tok = app ? a.append[n] : 0;
  const int len = old + (app ? 1 : 0);
  const bool pen = a.theta != 1.f;

  int at[HP];                                         // the id whose logit this thread rewrites, -1 = none
  bf16_t val[HP];
#pragma unroll
  for (int k = 0; k < HP; ++k) {
    const int i = tid + k * LT;
    at[k] = -1;
    val[k] = 0;
    if (i < len) {
      const int64_t t = (app && i == old) ? tok : hrow[i];
      h[i] = t;
      if (pen && t >= 0 && t < (int64_t)V) {
        at[k] = (int)t;
        val[k] = penalised(row[t], a.theta);            // the ORIGINAL logit: no thread has stored yet
      }
    }
  }
  __syncthreads();                                    // every original is in a register, the history is in LDS
#pragma unroll
  for (int k = 0; k < HP; ++k)
    if (at[k] >= 0) row[at[k]] = val[k];
  if (tid == 0 && app) {
    hrow[old] = tok;
    a.hist_len[n] = len;
  }
  __syncthreads();                                    // the -inf writes below come after every penalty store

  const int g = a.g;
  if (g >= 1 && len >= g) {
    const int s0 = len - g + 1;                       // the last g - 1 ids: h[s0 .. len)
    for (int j = tid; j <= len - g; j += LT) {
      bool m = true;
      for (int q = 0; q < g - 1 && m; ++q) m = h[j + q] == h[s0 + q];
      if (m) {
        const int64_t t = h[j + g - 1];
        if (t >= 0 && t < (int64_t)V) row[t] = BF_NEG_INF;
      }
    }
  }
  if (tid == 0 && a.ban >= 0 && a.ban < (long)V) row[a.ban] = BF_NEG_INF;
  for (long i = tid; i < a.n_suppress; i += LT) {
    const int t = a.suppress[i];
    if (t >= 0 && t < V) row[t] = BF_NEG_INF;
  }
}

}  // namespace

extern "C" int llmseg_logits_process(void* logits, int64_t ldl, int64_t N, int64_t V, int64_t* hist, int64_t ld_hist, int32_t* hist_len, const int64_t* append,
                                     float repetition_penalty, int32_t no_repeat_ngram, int64_t ban_token, const int32_t* suppress, int64_t n_suppress,
                                     void* stream) {
  LL_CHECK(logits && hist && hist_len, "logits_process: null pointer (logits, hist and hist_len are required)");
  LL_CHECK(((uintptr_t)logits & 1) == 0 && ((uintptr_t)hist & 7) == 0 && ((uintptr_t)append & 7) == 0 && ((uintptr_t)hist_len & 3) == 0 && ((uintptr_t)suppress & 3) == 0,
           "logits_process: a pointer is not aligned to its element type");
  LL_CHECK(N >= 1 && N <= 0x7fffffffL && V >= 1 && V <= 0x7fffffffL, "logits_process: need 1 <= N, V < 2^31 (N = %ld, V = %ld)", (long)N, (long)V);
  LL_CHECK(ldl >= V, "logits_process: ldl %ld < V %ld", (long)ldl, (long)V);
  LL_CHECK(ld_hist >= 1 && ld_hist <= CAP, "logits_process: ld_hist must be in [1, %d], got %ld", CAP, (long)ld_hist);
  LL_CHECK(isfinite(repetition_penalty) && repetition_penalty > 0.f, "logits_process: repetition_penalty must be finite and > 0 (1 = off), got %g", (double)repetition_penalty);
  LL_CHECK(no_repeat_ngram >= 0, "logits_process: no_repeat_ngram must be >= 0 (0 = off), got %d", (int)no_repeat_ngram);
  LL_CHECK(ban_token >= -1 && ban_token < V, "logits_process: ban_token must be in [-1, V = %ld) (-1 = none), got %ld", (long)V, (long)ban_token);
  LL_CHECK(n_suppress >= 0 && (n_suppress == 0) == (suppress == nullptr), "logits_process: n_suppress must be >= 0, and 0 exactly when suppress is NULL (got %ld)", (long)n_suppress);
  LogitsP a;
  a.logits = (bf16_t*)logits; a.ldl = ldl; a.V = (int)V;
  a.hist = hist; a.ld_hist = ld_hist; a.hist_len = hist_len; a.append = append;
  a.theta = repetition_penalty; a.g = no_repeat_ngram; a.ban = ban_token; a.suppress = suppress; a.n_suppress = n_suppress;
  LL_LAUNCH_KERNEL(logits_process_kernel, dim3((unsigned)N), dim3(LT), 0, (hipStream_t)stream, a);
  LL_LAUNCH_CHECK("logits_process");
  return LLMSEG_OK;
}
