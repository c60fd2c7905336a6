// Prompt-lookup decoding (generate(prompt_lookup_num_tokens=k)): the two launches around the decode step of Q = k + 1 tokens per sequence.  The rules are
// stated in include/llmseg_hip.h.
//   * llmseg_lookup_draft, one workgroup per row: the row's history (at most LLMSEG_LOGITS_HIST_CAP ids) goes to LDS once.  A window of g ids that ENDS in
//     front of position e equals the last g ids exactly when the r(e) ids in front of e equal the last r(e) ids for some r(e) >= g, so one backwards compare per
//     e (capped at max_g) answers every g at once: the rule's choice -- the longest g that has a match, the earliest match of that g -- is the e with the
//     largest r(e), the smallest e among equals.  That is ONE integer max over the key r(e) * 8192 + (8191 - e) in LDS (an integer atomic: order-free).
//   * llmseg_lookup_accept, two launches: the arg-max of every step row (one workgroup per row, the lowest index among equal values, a NaN counts as the
//     largest value: torch.argmax), then one thread per sequence that compares drafts and arg-maxes and keeps the books.
// No floating-point arithmetic beyond comparisons: both are pure functions of their inputs.
#include "common.h"

namespace {

constexpr int LT = 1024;                              // threads of a draft workgroup
constexpr int CAP = LLMSEG_LOGITS_HIST_CAP;
constexpr int QMAX = LLMSEG_DECODE_CHUNK_MAX;
static_assert(CAP <= 8192, "the match key packs e into 13 bits");

struct DraftP {
  const int64_t* hist; long ld_hist; const int32_t *hist_len, *count, *unfinished;
  int k, max_g, max_new; long V, pad;
  const int64_t* forced; long ld_forced;
  int64_t* tok; int32_t* draft_len;
};

__global__ __launch_bounds__(LT) void lookup_draft_kernel(DraftP a) {
  __shared__ int64_t h[CAP];
  __shared__ int best;
  const int tid = threadIdx.x;
  const long n = blockIdx.x;
  const int64_t* hrow = a.hist + n * a.ld_hist;
  const int len = min(max(a.hist_len[n], 0), (int)a.ld_hist);      // <= CAP (checked on the host)
  const int cnt = a.count[n];
  const bool live = a.unfinished[n] != 0 && cnt < a.max_new && len >= 1;
  const int limit = live ? min(a.k, a.max_new - cnt - 1) : 0;      // the step emits the accepted drafts and one more token: at most max_new - cnt in all
  for (int i = tid; i < len; i += LT) h[i] = hrow[i];
  if (tid == 0) best = -1;
  __syncthreads();
  if (limit > 0 && a.forced == nullptr) {
    const int gmax = min(a.max_g, len - 1);
    for (int e = 1 + tid; e < len; e += LT) {                  // e = where the continuation would start: the window in front of it is not the tail itself
      int r = 0;
      const int cap = min(gmax, e);
      while (r < cap && h[e - 1 - r] == h[len - 1 - r]) ++r;
      if (r > 0) atomicMax(&best, r * 8192 + (8191 - e));
    }
  }
  __syncthreads();
  if (tid == 0) {
    int64_t* t = a.tok + n * (a.k + 1);
    t[0] = len >= 1 ? h[len - 1] : a.pad;
    int d = 0;
    if (limit > 0) {
      const int64_t* src = nullptr;
      int avail = 0;
      if (a.forced != nullptr) { src = a.forced + n * a.ld_forced + cnt; avail = (int)min((long)limit, a.ld_forced - cnt); }
      else if (best >= 0) { const int e = 8191 - (best & 8191); src = h + e; avail = min(limit, len - e); }
      while (d < avail && src[d] >= 0 && src[d] < (int64_t)a.V) { t[1 + d] = src[d]; ++d; }      // cut before an id that is no vocabulary index (<image>)
    }
    for (int j = d; j < a.k; ++j) t[1 + j] = a.pad;
    a.draft_len[n] = d;
  }
}

// arg-max of a bf16 row: the lowest index among equal values; a NaN is the largest value (the first NaN wins)
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn) return i < bi;
  return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(256) void lookup_argmax_kernel(const bf16_t* __restrict__ logits, long ldl, int V, int32_t* __restrict__ am) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int tid = threadIdx.x;
  const bf16_t* row = logits + (long)blockIdx.x * ldl;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < V; i += 256) {
    const float v = bf2f(row[i]);
    if (bi == 0x7fffffff || better(v, i, bv, bi)) { bv = v; bi = i; }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || better(ov, oi, bv, bi))) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (si[w] != 0x7fffffff && (bi == 0x7fffffff || better(sv[w], si[w], bv, bi))) { bv = sv[w]; bi = si[w]; }
    am[blockIdx.x] = bi;
  }
}

struct AcceptP {
  const int32_t* am; const int64_t* tok; const int32_t* draft_len;
  int N, Q, max_new, first; long eos;
  int64_t* hist; long ld_hist; int32_t *hist_len, *pos_rows, *unfinished, *count;
  const int64_t* base; long dump; int64_t* map;
  int32_t* rec;                                       // [4][N]: unfinished | count | accepted | draft length
};

__global__ void lookup_accept_kernel(AcceptP a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  const int Q = a.Q, cnt = a.count[n];
  const int32_t* am = a.am + (long)n * Q;
  const bool live = a.unfinished[n] != 0 && cnt < a.max_new;
  const int d = (a.draft_len != nullptr && live) ? min(max(a.draft_len[n], 0), Q - 1) : 0;
  int acc = 0, emitted = 0;
  if (live) {
    const int64_t* t = a.tok + (long)n * Q;
    while (acc < d && t[1 + acc] == (int64_t)am[acc]) ++acc;
    const int room = min(acc + 1, a.max_new - cnt);             // the accepted drafts and one more token, cut at max_new_tokens ...
    int64_t* hrow = a.hist + (long)n * a.ld_hist;
    int len = a.hist_len[n];
    bool fin = false;
    while (emitted < room && !fin) {                           // ... and after the first eos
      const int64_t x = am[emitted];
      if (len < a.ld_hist) hrow[len] = x;
      ++len; ++emitted;
      fin = x == a.eos;
    }
    a.hist_len[n] = min(len, (int)a.ld_hist);
    a.count[n] = cnt + emitted;
    if (fin) a.unfinished[n] = 0;
    if (!a.first) a.pos_rows[n] += emitted;                    // the fed tokens that stand: the first and the accepted drafts, less what the cuts took
  }
  if (a.map != nullptr)                                        // step row n * Q + j holds the state of emitted token cnt - 1 + j where that token stands
    for (int j = 0; j < Q; ++j) a.map[(long)n * Q + j] = (!a.first && j < emitted) ? a.base[n] + cnt + j : a.dump;
  a.rec[n] = a.unfinished[n];
  a.rec[a.N + n] = a.count[n];
  a.rec[2 * a.N + n] = acc;
  a.rec[3 * a.N + n] = d;
}

}  // namespace

extern "C" int llmseg_lookup_draft(const int64_t* hist, int64_t ld_hist, const int32_t* hist_len, const int32_t* count, const int32_t* unfinished, int64_t N,
                                   int32_t k, int32_t max_ngram, int32_t max_new_tokens, int64_t V, int64_t pad_token, const int64_t* forced, int64_t ld_forced,
                                   int64_t* tok, int32_t* draft_len, void* stream) {
  LL_CHECK(hist && hist_len && count && unfinished && tok && draft_len, "lookup_draft: null pointer");
  LL_CHECK(((uintptr_t)hist & 7) == 0 && ((uintptr_t)forced & 7) == 0 && ((uintptr_t)tok & 7) == 0 && ((uintptr_t)hist_len & 3) == 0 && ((uintptr_t)count & 3) == 0 &&
           ((uintptr_t)unfinished & 3) == 0 && ((uintptr_t)draft_len & 3) == 0, "lookup_draft: a pointer is not aligned to its element type");
  LL_CHECK(N >= 1 && N <= 0x7fffffffL && V >= 1 && V <= 0x7fffffffL, "lookup_draft: need 1 <= N, V < 2^31 (N = %ld, V = %ld)", (long)N, (long)V);
  LL_CHECK(ld_hist >= 1 && ld_hist <= CAP, "lookup_draft: ld_hist must be in [1, %d], got %ld", CAP, (long)ld_hist);
  LL_CHECK(k >= 0 && k < QMAX, "lookup_draft: k must be in [0, %d], got %d", QMAX - 1, (int)k);
  LL_CHECK(max_ngram >= 1 && max_new_tokens >= 1, "lookup_draft: max_ngram and max_new_tokens must be >= 1 (got %d, %d)", (int)max_ngram, (int)max_new_tokens);
  LL_CHECK(forced == nullptr || ld_forced >= 1, "lookup_draft: ld_forced must be >= 1 with forced drafts");
  const DraftP a{hist, (long)ld_hist, hist_len, count, unfinished, (int)k, (int)max_ngram, (int)max_new_tokens, (long)V, (long)pad_token, forced, (long)ld_forced, tok, draft_len};
  LL_LAUNCH_KERNEL(lookup_draft_kernel, dim3((unsigned)N), dim3(LT), 0, (hipStream_t)stream, a);
  LL_LAUNCH_CHECK("lookup_draft");
  return LLMSEG_OK;
}

extern "C" int llmseg_lookup_accept(const void* logits, int64_t ldl, int64_t N, int32_t Q, int64_t V, const int64_t* tok, const int32_t* draft_len, int32_t first,
                                    int64_t eos_token, int32_t max_new_tokens, int64_t* hist, int64_t ld_hist, int32_t* hist_len, int32_t* pos_rows,
                                    int32_t* unfinished, int32_t* count, const int64_t* base, int64_t dump_row, int64_t* map, int32_t* rec, int32_t* argmax_ws,
                                    void* stream) {
  LL_CHECK(logits && hist && hist_len && pos_rows && unfinished && count && rec && argmax_ws, "lookup_accept: null pointer");
  LL_CHECK((tok != nullptr) == (draft_len != nullptr) && (map == nullptr || base != nullptr), "lookup_accept: tok and draft_len come as a pair, map needs base");
  LL_CHECK(((uintptr_t)logits & 1) == 0 && ((uintptr_t)hist & 7) == 0 && ((uintptr_t)tok & 7) == 0 && ((uintptr_t)base & 7) == 0 && ((uintptr_t)map & 7) == 0 &&
           (((uintptr_t)draft_len | (uintptr_t)hist_len | (uintptr_t)pos_rows | (uintptr_t)unfinished | (uintptr_t)count | (uintptr_t)rec | (uintptr_t)argmax_ws) & 3) == 0,
           "lookup_accept: a pointer is not aligned to its element type");
  LL_CHECK(N >= 1 && Q >= 1 && Q <= QMAX && N * Q <= 0x7fffffffL && V >= 1 && V <= 0x7fffffffL && ldl >= V, "lookup_accept: need N >= 1, 1 <= Q <= %d, 1 <= V < 2^31, ldl >= V", QMAX);
  LL_CHECK(Q == 1 || tok != nullptr, "lookup_accept: Q > 1 needs tok and draft_len");
  LL_CHECK(ld_hist >= 1 && ld_hist <= CAP && max_new_tokens >= 1, "lookup_accept: ld_hist must be in [1, %d] and max_new_tokens >= 1", CAP);
  LL_LAUNCH_KERNEL(lookup_argmax_kernel, dim3((unsigned)(N * Q)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ldl, (int)V, argmax_ws);
  LL_LAUNCH_CHECK("lookup_argmax");
  const AcceptP a{argmax_ws, tok, draft_len, (int)N, (int)Q, (int)max_new_tokens, (int)first, (long)eos_token, hist, (long)ld_hist, hist_len, pos_rows, unfinished, count,
                  base, (long)dump_row, map, rec};
  LL_LAUNCH_KERNEL(lookup_accept_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  LL_LAUNCH_CHECK("lookup_accept");
  return LLMSEG_OK;
}
