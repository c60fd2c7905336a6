// Decode step (one new token per sequence): RoPE of q and k at the device-side position, k / v appended to the cache, and
// softmax(q K^T * scale) V over the pos + 1 cached keys, in one launch (+ a merge when the keys of a head are split over workgroups).
// A CU takes only ~16 B/clk of missing lines, so the ~170 KB of K and V rows of one head (330 keys) are spread over `splits` workgroups
// until the launch covers the chip.  16 lanes own one key (8 dims each, one 16-byte load per K and V row); every 16-lane group runs an
// online softmax over its keys with all of a trip's K and V rows requested together (one HBM round trip per 64 keys per workgroup).
// The three entry points -- one position for every sequence, one position per sequence, and one position per sequence over a beam-indexed
// cache -- are one launch function over one kernel: RoPE, the append to [n][pos], the split count, the 16-lane key groups, the trip of 64
// keys, the online softmax and the merge exist once.
#include "common.h"
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
};

// TABLE (beam search over a cache that is never moved): a beam's history lives wherever its ancestors wrote it, and re-ordering the beams
// re-orders the int32 table (a few KB), not 32 layers of K and V.  The table entry of a key is uniform over the 16 lanes that own the key: one
// 4-byte load per lane (the lanes of a group hit one address), issued ahead of the trip's K and V requests; no LDS stage.  A table that names
// every row's own row gives the bits of the plain instance, which carries no trace of the table: the choice is made at compile time.
template <bool TABLE>
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
      if (j < j1) {
        if (j == pos) { kk[u] = *reinterpret_cast<const uint4*>(knew + c * 8); vv[u] = *reinterpret_cast<const uint4*>(vnew + c * 8); }
        else {
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

// `table`: the entry point reads through `src` (a null `src` is then an error, not the plain route); after the checks it is `src != nullptr`
int decode_attn_launch(bool table, const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                       const int32_t* pos_dev, long pos_stride, const int32_t* src, int64_t ld_src, int64_t capacity, int64_t N, int32_t heads, int32_t head_dim,
                       float scale, void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream) {
  const char* who = table ? "decode_attn_beams" : "decode_attn";
  LL_CHECK(qkv && cos && sin && kcache && vcache && pos_dev && out && N > 0 && N < 65536 && heads > 0, "%s: bad arguments", who);
  LL_CHECK(head_dim == 128, "%s: head_dim 128 only%s", who, table ? "" : " (use llmseg_rope_kv_append + llmseg_attn_fwd otherwise)");
  LL_CHECK((ld & 7) == 0 && (cache_stride_n & 7) == 0 && AL16(qkv) && AL16(kcache) && AL16(vcache), "%s: 16-byte alignment required", who);
  if (table) {
    LL_CHECK(src && ((uintptr_t)src & 3) == 0, "decode_attn_beams: src must be a 4-byte aligned int32 table");
    LL_CHECK(capacity > 0 && ld_src >= capacity, "decode_attn_beams: ld_src %ld < capacity %ld", (long)ld_src, (long)capacity);
  }
  int splits = 1;
  if (scratch) {
    splits = (int)std::min<int64_t>(16, std::max<int64_t>(1, 256 / (N * heads)));
    while (splits > 1 && (int64_t)N * heads * splits * 130 * 4 > scratch_bytes) --splits;
  }
  DecP p{(const bf16_t*)qkv, (long)ld, cos, sin, (bf16_t*)kcache, (bf16_t*)vcache, (long)cache_stride_n, pos_dev, pos_stride, heads, splits, scale,
         (bf16_t*)out, (long)ldo, (float*)scratch, src, (long)ld_src};
  const dim3 grid(heads * splits, (unsigned)N);
  if (table) LL_LAUNCH_KERNEL(decode_attn_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else LL_LAUNCH_KERNEL(decode_attn_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
  LL_LAUNCH_CHECK(who);
  if (splits > 1) {
    LL_LAUNCH_KERNEL(decode_attn_merge_kernel, dim3(heads, (unsigned)N), dim3(128), 0, (hipStream_t)stream, (const float*)scratch, heads, splits,
                     (bf16_t*)out, (long)ldo);
    LL_LAUNCH_CHECK(table ? "decode_attn_beams_merge" : "decode_attn_merge");
  }
  return LLMSEG_OK;
}

}  // namespace

extern "C" int llmseg_decode_attn(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                  const int32_t* pos_dev, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                                  void* scratch, int64_t scratch_bytes, void* stream) {
  return decode_attn_launch(false, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_dev, 0, nullptr, 0, 0, N, heads, head_dim, scale, out, ldo, scratch, scratch_bytes,
                            stream);
}

// one position per sequence (prompts of unequal length): the same kernel, which reads pos_rows_dev[n]
extern "C" int llmseg_decode_attn_rows(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                       const int32_t* pos_rows_dev, int64_t N, int32_t heads, int32_t head_dim, float scale, void* out, int64_t ldo,
                                       void* scratch, int64_t scratch_bytes, void* stream) {
  return decode_attn_launch(false, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_rows_dev, 1, nullptr, 0, 0, N, heads, head_dim, scale, out, ldo, scratch,
                            scratch_bytes, stream);
}

// ... over a beam-indexed cache: key t < pos of row n is read from the physical row src[n][t]
extern "C" int llmseg_decode_attn_beams(const void* qkv, int64_t ld, const float* cos, const float* sin, void* kcache, void* vcache, int64_t cache_stride_n,
                                        const int32_t* pos_rows_dev, const int32_t* src, int64_t ld_src, int64_t capacity, int64_t N, int32_t heads,
                                        int32_t head_dim, float scale, void* out, int64_t ldo, void* scratch, int64_t scratch_bytes, void* stream) {
  return decode_attn_launch(true, qkv, ld, cos, sin, kcache, vcache, cache_stride_n, pos_rows_dev, 1, src, ld_src, capacity, N, heads, head_dim, scale, out, ldo, scratch,
                            scratch_bytes, stream);
}
