// Decode step (one new token per sequence): RoPE of q and k at the device-side position, k / v appended to the cache, and
// softmax(q K^T * scale) V over the pos + 1 cached keys, in one launch (+ a merge when the keys of a head are split over workgroups).
// A CU takes only ~16 B/clk of missing lines, so the ~170 KB of K and V rows of one head (330 keys) are spread over `splits` workgroups
// until the launch covers the chip.  16 lanes own one key (8 dims each, one 16-byte load per K and V row); every 16-lane group runs an
// online softmax over its keys with all of a trip's K and V rows requested together (one HBM round trip per 64 keys per workgroup).
// The three entry points -- one position for every sequence, one position per sequence, and one position per sequence over a beam-indexed
// cache -- are one launch function over one kernel: RoPE, the append to [n][pos], the split count, the 16-lane key groups, the trip of 64
// keys, the online softmax and the merge exist once.  A fourth entry point runs the same step on an MXFP8 cache (E4M3 bytes + one E8M0 scale byte per 32
// dims, mxfp8.h): one more compile-time instance of the kernel, in which only the append, the load and the unpack differ.
#include "common.h"
#include "mxfp8.h"
#include <algorithm>

namespace {

struct DecP {
  const bf16_t* qkv; long ld;
  const float *cs, *sn;
  bf16_t *kc, *vc; long cstride;
  const int32_t* pos_dev; long pos_stride;           // position of sequence n: pos_dev[n * pos_stride] (0: one position for every sequence)
  int heads, splits;
  float scale;
  bf16_t* out; long ldo;
  float* part;                                         // [N][heads][splits][130]: 128 unnormalised outputs, running max, running sum
  // TABLE only: key t < pos of row n is read from the physical cache row src[n * ld_src + t].  (Last, so that the plain instance finds every argument it reads
  // where it always was.)
  const int32_t* src; long ld_src;
  // MX8 only: kc / vc are E4M3 bytes [n][t][heads * 128] (cstride in bytes), ksc / vsc their scale bytes [n][t][heads * 4] (sstride per sequence)
  uint8_t *ksc, *vsc; long sstride;
};

// Eight E4M3 bytes under scale byte sb -> the eight fp32 values element * 2^e.  From scale byte 10 on every non-zero result is a normal number (2^-9 * 2^-117 =
// 2^-126), so the hardware's packed E4M3 -> fp32 conversion (OCP encoding on gfx950, exact) and an exact ldexp give the value whatever the denormal mode; below
// that the integer decode of mxfp8.h, which flushes what is not a normal bf16 to +0.  Both equal the bf16 x_hat the quantiser writes.  (The code 0x80, -0, is
// never stored by the quantiser or the append.)
typedef float mx8_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void mx8_unpack8(uint32_t lo, uint32_t hi, int sb, float* f) {
  if (sb >= 10) {
    const int e = sb - 127;
    const mx8_f2 a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
    const mx8_f2 c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
    f[0] = ldexpf(a.x, e); f[1] = ldexpf(a.y, e); f[2] = ldexpf(b.x, e); f[3] = ldexpf(b.y, e);
    f[4] = ldexpf(c.x, e); f[5] = ldexpf(c.y, e); f[6] = ldexpf(d.x, e); f[7] = ldexpf(d.y, e);
  } else {
    uint32_t w[4];
    mx8_decode8(lo, hi, sb, w);
    unpack8(make_uint4(w[0], w[1], w[2], w[3]), f);
  }
}

// TABLE (beam search over a cache that is never moved): a beam's history lives wherever its ancestors wrote it, and re-ordering the beams
// re-orders the int32 table (a few KB), not 32 layers of K and V.  The table entry of a key is uniform over the 16 lanes that own the key: one
// 4-byte load per lane (the lanes of a group hit one address), issued ahead of the trip's K and V requests; no LDS stage.  A table that names
// every row's own row gives the bits of the plain instance, which carries no trace of the table: the choice is made at compile time.
// MX8 (the packed cache): the new token's k and v take part in this step as the bf16 values in LDS, exactly as in the bf16 instances; slot [n][pos] receives
// their MXFP8 rounding (lanes 0-15 of the owner's first wave encode k, lanes 16-31 v: four lanes per block of 32, as in the quantiser); every earlier key is
// 8 bytes per lane + the key's scale word (the head's four scale bytes), unpacked to the fp32 values the x_hat cache would give (mx8_unpack8).  Lane mapping,
// trip, split and merge are untouched, so the instance gives the bits of the bf16 instance on the cache of x_hat.
template <bool TABLE, bool MX8>
__global__ __launch_bounds__(256) void decode_attn_kernel(DecP p) {
  constexpr int HD = 128, UN = 4;
  __shared__ float qs[HD];
  __shared__ __align__(16) bf16_t knew[HD], vnew[HD];
  __shared__ float red[4][HD], rm[4], rl[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, c = tid & 15;
  const int h = blockIdx.x / p.splits, sp = blockIdx.x - h * p.splits, n = blockIdx.y;
  const long D = (long)p.heads * HD;
  const int pos = p.pos_dev[(long)n * p.pos_stride], nk = pos + 1;      // workgroup-uniform: a scalar load
  const int per = ((nk + p.splits - 1) / p.splits + 15) & ~15;
  const int j0 = sp * per, j1 = min(nk, j0 + per);
  const bool owner = pos >= j0 && pos < j1;              // the workgroup whose key range holds the new token appends it
  const bf16_t* row = p.qkv + (long)n * p.ld + (long)h * HD;
  bf16_t* kb = p.kc + (long)n * p.cstride + (long)h * HD;      // the row's OWN physical row: the append, and the reads without a table
  bf16_t* vb = p.vc + (long)n * p.cstride + (long)h * HD;
  const bf16_t* kh = p.kc + (long)h * HD;                       // TABLE: physical row 0, the reads add src[n][j] * cstride
  const bf16_t* vh = p.vc + (long)h * HD;
  const uint8_t *k8 = reinterpret_cast<const uint8_t*>(p.kc) + (long)h * HD, *v8 = reinterpret_cast<const uint8_t*>(p.vc) + (long)h * HD;      // MX8: physical row 0
  const long SD = (long)p.heads * 4;                            // MX8: scale bytes per cache slot
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
        if constexpr (!MX8) { kb[(long)pos * D + i] = o1; kb[(long)pos * D + i + 64] = o2; }
      }
    }
  } else if (tid < 192 && owner) {
    const int i = tid - 128;
    const bf16_t v1 = row[2 * D + i], v2 = row[2 * D + i + 64];
    vnew[i] = v1; vnew[i + 64] = v2;
    if constexpr (!MX8) { vb[(long)pos * D + i] = v1; vb[(long)pos * D + i + 64] = v2; }
  }
  __syncthreads();
  if constexpr (MX8) {
    if (owner && tid < 32) {                               // the append: slot [n][pos] <- the MXFP8 rounding of the new k (lanes 0-15) and v (lanes 16-31)
      const bool isv = tid >= 16;
      const uint4 nv = *reinterpret_cast<const uint4*>((isv ? vnew : knew) + c * 8);
      uint32_t w[4] = {nv.x, nv.y, nv.z, nv.w}, lo, hi;
      uint32_t amax = mx8_amax8(w);
      amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
      amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2));
      const int sb = mx8_scale_byte(amax);
      mx8_encode8(w, sb, lo, hi);
      uint8_t* q8 = reinterpret_cast<uint8_t*>(isv ? p.vc : p.kc) + (long)n * p.cstride + (long)pos * D + (long)h * HD;
      *reinterpret_cast<uint2*>(q8 + c * 8) = make_uint2(lo, hi);
      if ((c & 3) == 0) (isv ? p.vsc : p.ksc)[(long)n * p.sstride + (long)pos * SD + h * 4 + (c >> 2)] = (uint8_t)sb;
    }
  }
  float q[8], acc[8], m = -1e30f, l = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) { q[e] = qs[c * 8 + e]; acc[e] = 0.f; }
  for (int jb = j0; jb < j1; jb += 16 * UN) {
    uint4 kk[UN], vv[UN];
    uint32_t ksw[UN], vsw[UN];                            // MX8: kk / vv hold 8 bytes in .x / .y until the unpack, ksw / vsw the key's scale words
    long phys[UN];
    if constexpr (TABLE) {                              // the trip's table entries first: the K and V addresses wait for them
      const int32_t* srow = p.src + (long)n * p.ld_src;
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int j = jb + u * 16 + g;
        phys[u] = (j < j1 && j != pos) ? (long)srow[j] : 0L;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = jb + u * 16 + g;
      kk[u] = make_uint4(0, 0, 0, 0); vv[u] = kk[u];
      if constexpr (MX8) { ksw[u] = 0u; vsw[u] = 0u; }
      if (j < j1) {
        if (j == pos) { kk[u] = *reinterpret_cast<const uint4*>(knew + c * 8); vv[u] = *reinterpret_cast<const uint4*>(vnew + c * 8); }
        else if constexpr (MX8) {
          const long prow = TABLE ? phys[u] : (long)n;
          const long off = prow * p.cstride + (long)j * D + c * 8, soff = prow * p.sstride + (long)j * SD + h * 4;
          const uint2 k2 = *reinterpret_cast<const uint2*>(k8 + off), v2 = *reinterpret_cast<const uint2*>(v8 + off);
          kk[u].x = k2.x; kk[u].y = k2.y; vv[u].x = v2.x; vv[u].y = v2.y;
          ksw[u] = *reinterpret_cast<const uint32_t*>(p.ksc + soff); vsw[u] = *reinterpret_cast<const uint32_t*>(p.vsc + soff);
        } else {
          if constexpr (TABLE) {
            const long off = phys[u] * p.cstride + (long)j * D + c * 8;
            kk[u] = *reinterpret_cast<const uint4*>(kh + off); vv[u] = *reinterpret_cast<const uint4*>(vh + off);
          } else { kk[u] = *reinterpret_cast<const uint4*>(kb + (long)j * D + c * 8); vv[u] = *reinterpret_cast<const uint4*>(vb + (long)j * D + c * 8); }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = jb + u * 16 + g;
      float kf[8], vf[8], s = 0.f;
      if (MX8 && j != pos && j < j1) {                     // a cached key of the packed cache (the new token's and a key beyond j1 are bf16 as in the other instances)
        const int sh = 8 * (c >> 2);
        mx8_unpack8(kk[u].x, kk[u].y, (int)((ksw[u] >> sh) & 0xffu), kf);
        mx8_unpack8(vv[u].x, vv[u].y, (int)((vsw[u] >> sh) & 0xffu), vf);
      } else {
        unpack8(kk[u], kf);
        unpack8(vv[u], vf);
      }
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

__global__ __launch_bounds__(128) void decode_attn_merge_kernel(const float* __restrict__ part, int heads, int splits, bf16_t* __restrict__ out, long ldo) {
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

struct Mx8Scales { void *k, *v; int64_t stride_n; };      // the packed cache's scale bytes; the bf16 entry points pass none

// `table`: the entry point reads through `src` (a null `src` is then an error, not the plain route); after the checks it is `src != nullptr`.
// `mx`: the packed cache (llmseg_decode_attn_mxfp8), whose caches hold bytes: 8-byte rows instead of 16-byte ones, and the checks of its scales.
int decode_attn_launch(bool table, const Mx8Scales* mx, const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                       const int32_t* pos_dev, long pos_stride, const int32_t* src, int64_t ld_src, int64_t capacity, int64_t N, int32_t heads, int32_t head_dim,
                       float scale, void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream) {
  const char* who = mx ? "decode_attn_mxfp8" : table ? "decode_attn_beams" : "decode_attn";
  LL_CHECK(qkv && cos && sin && kcache && vcache && pos_dev && out && N > 0 && N < 65536 && heads > 0, "%s: bad arguments", who);
  LL_CHECK(head_dim == 128, "%s: head_dim 128 only%s", who, table ? "" : " (use llmseg_rope_kv_append + llmseg_attn_fwd otherwise)");
  if (mx) {
    LL_CHECK((ld & 7) == 0 && AL16(qkv) && (cache_stride_n & 7) == 0 && ((uintptr_t)kcache & 7) == 0 && ((uintptr_t)vcache & 7) == 0,
             "decode_attn_mxfp8: qkv 16-byte aligned, the byte caches and their sequence stride 8-byte aligned");
    LL_CHECK(mx->k && mx->v && ((uintptr_t)mx->k & 3) == 0 && ((uintptr_t)mx->v & 3) == 0 && (mx->stride_n & 3) == 0 && mx->stride_n >= (int64_t)heads * 4,
             "decode_attn_mxfp8: scales must be 4-byte aligned with a sequence stride %% 4 == 0 of at least heads * 4 bytes");
    LL_CHECK(cache_stride_n >= (int64_t)heads * 128, "decode_attn_mxfp8: cache_stride_n %ld < heads * 128", (long)cache_stride_n);
    LL_CHECK(pos_stride == 0 || pos_stride == 1, "decode_attn_mxfp8: pos_stride must be 0 (one position) or 1 (one per sequence)");
  } else
    LL_CHECK((ld & 7) == 0 && (cache_stride_n & 7) == 0 && AL16(qkv) && AL16(kcache) && AL16(vcache), "%s: 16-byte alignment required", who);
  if (table) {
    LL_CHECK(src && ((uintptr_t)src & 3) == 0, "%s: src must be a 4-byte aligned int32 table", who);
    LL_CHECK(capacity > 0 && ld_src >= capacity, "%s: ld_src %ld < capacity %ld", who, (long)ld_src, (long)capacity);
  }
  int splits = 1;
  if (scratch) {
    splits = (int)std::min<int64_t>(16, std::max<int64_t>(1, 256 / (N * heads)));
    while (splits > 1 && (int64_t)N * heads * splits * 130 * 4 > scratch_bytes) --splits;
  }
  DecP p{(const bf16_t*)qkv, (long)ld, cos, sin, (bf16_t*)kcache, (bf16_t*)vcache, (long)cache_stride_n, pos_dev, pos_stride, heads, splits, scale,
         (bf16_t*)out, (long)ldo, (float*)scratch, src, (long)ld_src, mx ? (uint8_t*)mx->k : nullptr, mx ? (uint8_t*)mx->v : nullptr, mx ? (long)mx->stride_n : 0L};
  const dim3 grid(heads * splits, (unsigned)N);
  if (mx && table) LL_LAUNCH_KERNEL((decode_attn_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else if (mx) LL_LAUNCH_KERNEL((decode_attn_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else if (table) LL_LAUNCH_KERNEL((decode_attn_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else LL_LAUNCH_KERNEL((decode_attn_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
  LL_LAUNCH_CHECK(who);
  if (splits > 1) {
    LL_LAUNCH_KERNEL(decode_attn_merge_kernel, dim3(heads, (unsigned)N), dim3(128), 0, (hipStream_t)stream, (const float*)scratch, heads, splits,
                     (bf16_t*)out, (long)ldo);
    LL_LAUNCH_CHECK(mx ? "decode_attn_mxfp8_merge" : table ? "decode_attn_beams_merge" : "decode_attn_merge");
  }
  return LLMSEG_OK;
}

// ---- Q tokens per sequence in one step (generate(prompt_lookup_num_tokens=): the last emitted token and up to Q - 1 drafts) ----
// Query j of sequence n sits at position pos + j and attends to keys 0 .. pos + j.  The lane mapping is the one above -- 16 lanes own a key, 8 dims each, a trip
// of 64 keys with every K and V row requested together -- and a cached row, once in registers, serves all QN queries: QN * 8 query values, QN * 8 accumulators
// and QN running (max, sum) pairs per lane (78 registers at QN = 1, 166 at 4, 256 at 7, 256 + 38 AGPRs at 8, no spills: one to six waves per SIMD, of which the
// workgroup needs one).  The QN new keys and values never come from the
// cache: EVERY workgroup of the head rotates them into LDS and takes keys pos .. pos + QN - 1 from there, so no workgroup reads a slot that another one writes
// in this launch; the workgroup of split 0 alone stores them, with the bits QN successive llmseg_decode_attn_rows steps store (the same rope_lo / rope_hi, the
// same f2bf; v is a copy).  Key split and merge are the existing scheme with the partials laid out per STEP ROW n * QN + j, which is what the merge kernel
// above reads for N * QN rows.  A query with no key in a split leaves (max, sum) = (-1e30, 0): the merge weighs it with exp(-1e30 - M) = 0.
// Rejected drafts: after the step the accept launch moves pos to pos + a + 1 <= pos + QN, so slots at or beyond the new position hold keys of tokens that are
// not part of the sequence.  That is sound for the reason the prefill's comment gives: the next step writes QN slots from the new position on before any
// query's key count reaches them (query j reads keys < pos' from the cache and keys pos' .. pos' + j from LDS), so a stale slot is overwritten before it is read.
struct ChunkP {
  const bf16_t* qkv; long ld;
  const float *cs, *sn;
  bf16_t *kc, *vc; long cstride;
  const int32_t* pos_dev;
  int heads, splits, capacity;
  float scale;
  bf16_t* out; long ldo;
  float* part;                                         // [N * QN][heads][splits][130]
};

template <int QN>
__global__ __launch_bounds__(256) void decode_attn_chunk_kernel(ChunkP p) {
  constexpr int HD = 128, UN = 4;
  __shared__ float qs[QN][HD];
  __shared__ __align__(16) bf16_t knew[QN][HD], vnew[QN][HD];
  __shared__ float red[4][QN][HD], rm[4][QN], rl[4][QN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, c = tid & 15;
  const int h = blockIdx.x / p.splits, sp = blockIdx.x - h * p.splits, n = blockIdx.y;
  const long D = (long)p.heads * HD;
  const int pos = p.pos_dev[n], nk = pos + QN;            // workgroup-uniform: a scalar load.  Keys 0 .. pos + QN - 1, query j sees those <= pos + j
  const int per = ((nk + p.splits - 1) / p.splits + 15) & ~15;
  const int j0 = sp * per, j1 = min(nk, j0 + per);
  bf16_t* kb = p.kc + (long)n * p.cstride + (long)h * HD;
  bf16_t* vb = p.vc + (long)n * p.cstride + (long)h * HD;
  // the QN new tokens: q and k rotated at pos + j, v copied, all into LDS; split 0 stores k and v (a slot at or beyond the capacity is not written)
  for (int t = tid; t < QN * 192; t += 256) {
    const int j = t / 192, r = t - j * 192, i = r & 63;
    const bf16_t* row = p.qkv + ((long)n * QN + j) * p.ld + (long)h * HD;
    const int pj = pos + j;
    const bool store = sp == 0 && pj < p.capacity;
    if (r < 128) {
      const bf16_t* src = row + (r < 64 ? 0 : D);
      const float a = bf2f(src[i]), b = bf2f(src[i + 64]);
      const long ti = (long)min(pj, p.capacity - 1) * 64 + i;
      const float cv = p.cs[ti], sv = p.sn[ti];
      const bf16_t o1 = f2bf(rope_lo(a, b, cv, sv)), o2 = f2bf(rope_hi(a, b, cv, sv));
      if (r < 64) { qs[j][i] = bf2f(o1); qs[j][i + 64] = bf2f(o2); }
      else {
        knew[j][i] = o1; knew[j][i + 64] = o2;
        if (store) { kb[(long)pj * D + i] = o1; kb[(long)pj * D + i + 64] = o2; }
      }
    } else {
      const bf16_t v1 = row[2 * D + i], v2 = row[2 * D + i + 64];
      vnew[j][i] = v1; vnew[j][i + 64] = v2;
      if (store) { vb[(long)pj * D + i] = v1; vb[(long)pj * D + i + 64] = v2; }
    }
  }
  __syncthreads();
  float q[QN][8], acc[QN][8], m[QN], l[QN];
#pragma unroll
  for (int jq = 0; jq < QN; ++jq) {
    m[jq] = -1e30f; l[jq] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { q[jq][e] = qs[jq][c * 8 + e]; acc[jq][e] = 0.f; }
  }
  for (int jb = j0; jb < j1; jb += 16 * UN) {
    uint4 kk[UN], vv[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = jb + u * 16 + g;
      kk[u] = make_uint4(0, 0, 0, 0); vv[u] = kk[u];
      if (j < j1) {
        if (j >= pos) { kk[u] = *reinterpret_cast<const uint4*>(&knew[j - pos][c * 8]); vv[u] = *reinterpret_cast<const uint4*>(&vnew[j - pos][c * 8]); }
        else { kk[u] = *reinterpret_cast<const uint4*>(kb + (long)j * D + c * 8); vv[u] = *reinterpret_cast<const uint4*>(vb + (long)j * D + c * 8); }
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = jb + u * 16 + g;
      float kf[8], vf[8];
      unpack8(kk[u], kf);
      unpack8(vv[u], vf);
#pragma unroll
      for (int jq = 0; jq < QN; ++jq) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(q[jq][e], kf[e], s);
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        const bool valid = j < j1 && j <= pos + jq;
        s = valid ? s * p.scale : -1e30f;
        const float mn = fmaxf(m[jq], s), corr = __expf(m[jq] - mn), pj = valid ? __expf(s - mn) : 0.f;
        l[jq] = l[jq] * corr + pj;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[jq][e] = acc[jq][e] * corr + pj * vf[e];
        m[jq] = mn;
      }
    }
  }
  // per query: the four key groups of a wave, then the four waves
#pragma unroll
  for (int jq = 0; jq < QN; ++jq) {
    float mw = fmaxf(m[jq], __shfl_xor(m[jq], 16));
    mw = fmaxf(mw, __shfl_xor(mw, 32));
    const float f = __expf(m[jq] - mw);
    float lq = l[jq] * f;
    lq += __shfl_xor(lq, 16); lq += __shfl_xor(lq, 32);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = acc[jq][e] * f;
      a += __shfl_xor(a, 16); a += __shfl_xor(a, 32);
      if (lane < 16) red[wave][jq][c * 8 + e] = a;
    }
    if (lane == 0) { rm[wave][jq] = mw; rl[wave][jq] = lq; }
  }
  __syncthreads();
  for (int t = tid; t < QN * HD; t += 256) {
    const int jq = t >> 7, d = t & 127;
    const float M = fmaxf(fmaxf(rm[0][jq], rm[1][jq]), fmaxf(rm[2][jq], rm[3][jq]));
    float L = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const float e = __expf(rm[w][jq] - M); L += e * rl[w][jq]; o += e * red[w][jq][d]; }
    const long srow = (long)n * QN + jq;
    if (p.splits == 1) p.out[srow * p.ldo + (long)h * HD + d] = f2bf(o / L);
    else {
      float* pp = p.part + ((srow * p.heads + h) * p.splits + sp) * 130;
      pp[d] = o;
      if (d == 0) { pp[128] = M; pp[129] = L; }
    }
  }
}

template <int QN>
void decode_attn_chunk_instance(const dim3& grid, hipStream_t stream, const ChunkP& p) {
  LL_LAUNCH_KERNEL((decode_attn_chunk_kernel<QN>), grid, dim3(256), 0, stream, p);
}

}  // namespace

// Q tokens per sequence: qkv [N * Q][ld], step row n * Q + j = token j of sequence n at position pos_rows_dev[n] + j
extern "C" int llmseg_decode_attn_chunk(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                        const int32_t* pos_rows_dev, int64_t capacity, int64_t N, int32_t Q, int32_t heads, int32_t head_dim, float scale,
                                        void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream) {
  LL_CHECK(qkv && cos && sin && kcache && vcache && pos_rows_dev && out && N > 0 && N < 65536 && heads > 0, "decode_attn_chunk: bad arguments");
  LL_CHECK(head_dim == 128, "decode_attn_chunk: head_dim 128 only");
  LL_CHECK(Q >= 1 && Q <= LLMSEG_DECODE_CHUNK_MAX && N * Q < 65536, "decode_attn_chunk: Q must be in [1, %d] and N * Q < 65536, got Q = %d", LLMSEG_DECODE_CHUNK_MAX, (int)Q);
  LL_CHECK((ld & 7) == 0 && (cache_stride_n & 7) == 0 && AL16(qkv) && AL16(kcache) && AL16(vcache), "decode_attn_chunk: 16-byte alignment required");
  LL_CHECK(capacity >= Q && capacity <= 0x7fffffffL && cache_stride_n >= capacity * (int64_t)heads * 128,
           "decode_attn_chunk: need Q <= capacity and cache_stride_n >= capacity * heads * 128 (capacity %ld, stride %ld)", (long)capacity, (long)cache_stride_n);
  LL_CHECK(ld >= 3 * (int64_t)heads * 128 && ldo >= (int64_t)heads * 128, "decode_attn_chunk: ld %ld / ldo %ld too small for %d heads", (long)ld, (long)ldo, (int)heads);
  int splits = 1;
  if (scratch) {
    splits = (int)std::min<int64_t>(16, std::max<int64_t>(1, 256 / (N * heads)));
    while (splits > 1 && (int64_t)N * Q * heads * splits * 130 * 4 > scratch_bytes) --splits;
  }
  const ChunkP p{(const bf16_t*)qkv, (long)ld, cos, sin, (bf16_t*)kcache, (bf16_t*)vcache, (long)cache_stride_n, pos_rows_dev, heads, splits, (int)capacity, scale,
                 (bf16_t*)out, (long)ldo, (float*)scratch};
  const dim3 grid(heads * splits, (unsigned)N);
  switch (Q) {
    case 1: decode_attn_chunk_instance<1>(grid, (hipStream_t)stream, p); break;
    case 2: decode_attn_chunk_instance<2>(grid, (hipStream_t)stream, p); break;
    case 3: decode_attn_chunk_instance<3>(grid, (hipStream_t)stream, p); break;
    case 4: decode_attn_chunk_instance<4>(grid, (hipStream_t)stream, p); break;
    case 5: decode_attn_chunk_instance<5>(grid, (hipStream_t)stream, p); break;
    case 6: decode_attn_chunk_instance<6>(grid, (hipStream_t)stream, p); break;
    case 7: decode_attn_chunk_instance<7>(grid, (hipStream_t)stream, p); break;
    default: decode_attn_chunk_instance<8>(grid, (hipStream_t)stream, p); break;
  }
  LL_LAUNCH_CHECK("decode_attn_chunk");
  if (splits > 1) {
    LL_LAUNCH_KERNEL(decode_attn_merge_kernel, dim3(heads, (unsigned)(N * Q)), dim3(128), 0, (hipStream_t)stream, (const float*)scratch, heads, splits, (bf16_t*)out, (long)ldo);
    LL_LAUNCH_CHECK("decode_attn_chunk_merge");
  }
  return LLMSEG_OK;
}

extern "C" int llmseg_decode_attn(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                  const int32_t* pos_dev, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                                  void* scratch, int64_t scratch_bytes, void* stream) {
  return decode_attn_launch(false, nullptr, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_dev, 0, nullptr, 0, 0, N, heads, head_dim, scale, out, ldo, scratch, scratch_bytes,
                            stream);
}

// one position per sequence (prompts of unequal length): the same kernel, which reads pos_rows_dev[n]
extern "C" int llmseg_decode_attn_rows(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                       const int32_t* pos_rows_dev, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                                       void* scratch, int64_t scratch_bytes, void* stream) {
  return decode_attn_launch(false, nullptr, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_rows_dev, 1, nullptr, 0, 0, N, heads, head_dim, scale, out, ldo, scratch,
                            scratch_bytes, stream);
}

// ... over a beam-indexed cache: key t < pos of row n is read from the physical row src[n][t]
extern "C" int llmseg_decode_attn_beams(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                        const int32_t* pos_rows_dev, const int32_t* src, int64_t ld_src, int64_t capacity, int64_t N, int32_t heads,
                                        int32_t head_dim, float scale, void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream) {
  return decode_attn_launch(true, nullptr, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_rows_dev, 1, src, ld_src, capacity, N, heads, head_dim, scale, out, ldo, scratch,
                            scratch_bytes, stream);
}

// the same step on an MXFP8 cache (E4M3 bytes + E8M0 scale bytes): pos_stride 0 = one position for every sequence, 1 = one per sequence; src nullable
extern "C" int llmseg_decode_attn_mxfp8(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                        void* kscale, void* vscale, int64_t scale_stride_n, const int32_t* pos_dev, int64_t pos_stride, const int32_t* src,
                                        int64_t ld_src, int64_t capacity, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                                        void* scratch, int64_t scratch_bytes, void* stream) {
  const Mx8Scales mx{kscale, vscale, scale_stride_n};
  return decode_attn_launch(src != nullptr, &mx, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_dev, (long)pos_stride, src, ld_src, capacity, N, heads, head_dim,
                            scale, out, ldo, scratch, scratch_bytes, stream);
}
