// MXFP8 quantiser of the KV cache: bf16 rows -> E4M3 bytes + one E8M0 scale byte per 32 elements (+ x_hat = element * 2^e in bf16), one launch over
// batch x rows rows with a batch stride and a row stride per operand and an optional device-side first row per batch.  Four lanes own one block of 32
// (one 16-byte load each); the block's amax crosses them by two shuffles, so a block is read whole before any of it is written: x_hat may alias x.
#include "common.h"
#include "mxfp8.h"

namespace {

struct KvqP {
  const bf16_t* x; long x_bs, x_rs;
  uint8_t* q; long q_bs, q_rs;
  uint8_t* sc; long s_bs, s_rs;
  bf16_t* xh; long h_bs, h_rs;
  const int32_t* row0; long row0_stride;
  long rows, chunks, total;                            // chunks = D / 8 per row; total = batch * rows * chunks lanes of work
};

__global__ __launch_bounds__(256) void kv_quantize_mxfp8_kernel(KvqP p) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const bool active = idx < p.total;                   // (total % 4 == 0: the four lanes of a block are active together)
  long b = 0, r = 0, c = 0;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (active) {
    const long row = idx / p.chunks;
    c = idx - row * p.chunks;
    b = row / p.rows;
    r = row - b * p.rows + (p.row0 ? (long)p.row0[b * p.row0_stride] : 0L);
    const uint4 v = *reinterpret_cast<const uint4*>(p.x + b * p.x_bs + r * p.x_rs + c * 8);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
  uint32_t amax = mx8_amax8(w);
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2));
  if (!active) return;
  const int sb = mx8_scale_byte(amax);
  uint32_t lo, hi;
  mx8_encode8(w, sb, lo, hi);
  if (p.q) {
    *reinterpret_cast<uint2*>(p.q + b * p.q_bs + r * p.q_rs + c * 8) = make_uint2(lo, hi);
    if ((c & 3) == 0) p.sc[b * p.s_bs + r * p.s_rs + (c >> 2)] = (uint8_t)sb;
  }
  if (p.xh) *reinterpret_cast<uint4*>(p.xh + b * p.h_bs + r * p.h_rs + c * 8) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

extern "C" int llmseg_kv_quantize_mxfp8(const void* x, int64_t x_stride_b, int64_t x_stride_r, void* q, int64_t q_stride_b, int64_t q_stride_r, void* scale,
                                        int64_t s_stride_b, int64_t s_stride_r, void* x_hat, int64_t h_stride_b, int64_t h_stride_r, const int32_t* row0_dev,
                                        int64_t row0_stride, int64_t batch, int64_t rows, int64_t D, void* stream) {
  LL_CHECK(x && AL16(x), "kv_quantize_mxfp8: x must be a 16-byte aligned bf16 pointer");
  LL_CHECK((q != nullptr) == (scale != nullptr), "kv_quantize_mxfp8: q and scale are given or omitted as a pair");
  LL_CHECK(q || x_hat, "kv_quantize_mxfp8: no output (q + scale, x_hat or both)");
  LL_CHECK(batch >= 1 && rows >= 1 && D >= 32 && (D & 31) == 0 && batch * rows <= (1L << 40) / D, "kv_quantize_mxfp8: batch %ld, rows %ld >= 1 and D %ld %% 32 == 0 required",
           (long)batch, (long)rows, (long)D);
  const bool many = batch > 1;
  LL_CHECK((x_stride_r & 7) == 0 && (x_stride_b & 7) == 0 && x_stride_r >= D && (!many || x_stride_b >= rows * x_stride_r),
           "kv_quantize_mxfp8: x strides (%ld, %ld): %% 8 == 0, row stride >= D, batch stride >= rows * row stride", (long)x_stride_b, (long)x_stride_r);
  if (q) {
    LL_CHECK(((uintptr_t)q & 7) == 0 && (q_stride_r & 7) == 0 && (q_stride_b & 7) == 0 && q_stride_r >= D && (!many || q_stride_b >= rows * q_stride_r),
             "kv_quantize_mxfp8: q 8-byte aligned, strides (%ld, %ld): %% 8 == 0, row stride >= D, batch stride >= rows * row stride", (long)q_stride_b, (long)q_stride_r);
    LL_CHECK(s_stride_r >= D / 32 && (!many || s_stride_b >= rows * s_stride_r), "kv_quantize_mxfp8: scale strides (%ld, %ld): row stride >= D / 32, batch stride >= rows * row stride",
             (long)s_stride_b, (long)s_stride_r);
  }
  if (x_hat)
    LL_CHECK(AL16(x_hat) && (h_stride_r & 7) == 0 && (h_stride_b & 7) == 0 && h_stride_r >= D && (!many || h_stride_b >= rows * h_stride_r),
             "kv_quantize_mxfp8: x_hat 16-byte aligned, strides (%ld, %ld): %% 8 == 0, row stride >= D, batch stride >= rows * row stride", (long)h_stride_b, (long)h_stride_r);
  LL_CHECK(!row0_dev || ((((uintptr_t)row0_dev) & 3) == 0 && (row0_stride == 0 || row0_stride == 1)), "kv_quantize_mxfp8: row0_dev 4-byte aligned with stride 0 or 1");
  KvqP p{(const bf16_t*)x, (long)x_stride_b, (long)x_stride_r, (uint8_t*)q, (long)q_stride_b, (long)q_stride_r, (uint8_t*)scale, (long)s_stride_b, (long)s_stride_r,
         (bf16_t*)x_hat, (long)h_stride_b, (long)h_stride_r, row0_dev, (long)row0_stride, (long)rows, (long)(D / 8), (long)(batch * rows * (D / 8))};
  const long blocks = (p.total + 255) / 256;
  LL_CHECK(blocks < (1L << 31), "kv_quantize_mxfp8: too many rows for one launch");
  LL_LAUNCH_KERNEL(kv_quantize_mxfp8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  LL_LAUNCH_CHECK("kv_quantize_mxfp8");
  return LLMSEG_OK;
}
