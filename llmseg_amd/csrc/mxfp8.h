// MXFP8 (OCP Microscaling: E4M3 elements, one E8M0 scale byte per block of 32) on bf16 bits: the rule of include/llmseg_hip.h in integer work, shared by
// the quantiser (kv_quant.hip) and the decode step on the packed cache (decode_attn.hip), so that what one writes is what the other reads.  No floating-point
// operation: nothing here depends on the denormal mode, and the same functions compile for the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MX8_FN __host__ __device__ __forceinline__
#else
#define MX8_FN inline
#endif

// scale byte e + 127 of a block whose largest |x| has the bf16 bits `amax` (sign cleared): e = the smallest integer >= -127 with amax <= 448 * 2^e.
// A normal amax = m * 2^E takes e = E - 8 when m <= 1.75 (mantissa field <= 96), else E - 7; zero and subnormal amax take e = -127.
MX8_FN int mx8_scale_byte(uint32_t amax) {
  const int ef = (int)(amax >> 7), sb = ef - 8 + ((amax & 0x7fu) > 96u ? 1 : 0);
  return ef == 0 || sb < 0 ? 0 : sb;
}

// E4M3 code of the bf16 bits u under the block's scale byte sb: |x| / 2^e = sig * 2^s is rounded to the nearest multiple of the quantum of its binade
// (2^-9 below 2^-6), ties to even; a carry out of the mantissa lands in the next exponent by plain addition.  -0 and everything that rounds to 0 is +0.
MX8_FN uint32_t mx8_encode(uint32_t u, int sb) {
  const uint32_t a = u & 0x7fffu;
  const int ef = (int)(a >> 7);
  const uint32_t sig = (a & 0x7fu) | (ef ? 0x80u : 0u);
  if (sig == 0) return 0;
  const int s = (ef ? ef : 1) - 7 - sb;                   // |x| / 2^e = sig * 2^s, sig < 256
  const int p = 31 - __builtin_clz(sig);
  const int ey = p + s;                                   // floor(log2 |y|)
  const int be = (ey > -6 ? ey : -6) + 7;                 // exponent field of the binade y is rounded in (1: the subnormals share the quantum of 2^-6)
  int shift = be - 10 - s;                                // the quantum is 2^(be - 10)
  uint32_t r;
  if (shift <= 0) r = sig << -shift;                      // (>= -3: a bf16 subnormal with fewer than four significant bits)
  else {
    if (shift > 16) shift = 16;                           // sig < 2^8: everything from 10 on rounds to 0
    r = (sig + ((1u << (shift - 1)) - 1u) + ((sig >> shift) & 1u)) >> shift;
  }
  uint32_t code = ((uint32_t)(be - 1) << 3) + r;          // r in [8, 16] for a normal y, [0, 8] below 2^-6: 16 and 8 carry into the exponent field
  if (code > 0x7eu) code = 0x7eu;                         // never taken under the block's own scale (|y| <= 448): 0x7f is the NaN code
  return code ? code | ((u >> 8) & 0x80u) : 0u;
}

// bf16 bits of element * 2^e (exact: four significant bits); a result below the smallest normal bf16 is flushed to +0
MX8_FN uint32_t mx8_decode(uint32_t b, int sb) {
  const uint32_t mag = b & 0x7fu;
  int ex;
  uint32_t mb;
  if (mag >= 8u) { ex = (int)(mag >> 3) + sb - 7; mb = (mag & 7u) << 4; }
  else {                                                  // an E4M3 subnormal k * 2^-9: normalised by hand
    const int p = mag >= 4u ? 2 : mag >= 2u ? 1 : 0;
    ex = p + sb - 9; mb = (mag << (7 - p)) & 0x7fu;
  }
  return mag != 0u && ex >= 1 ? ((b & 0x80u) << 8) | ((uint32_t)ex << 7) | mb : 0u;
}

// eight elements (8 bytes, element i in byte i) -> eight packed bf16 in the layout a 16-byte load of the bf16 row would give
// Two code bytes at bits 0-7 and 16-23 of p, both normal E4M3 (magnitude >= 8) under sb >= 7 -> their packed bf16: exponent and mantissa fields of the code sit
// four bits below bf16's, and the scale adds (sb - 7) to the exponent field; no carry leaves a half (0x7f0 + 0x7800 < 0x8000).
MX8_FN uint32_t mx8_decode_pair_normal(uint32_t p, uint32_t k2) { return (((p & 0x007f007fu) << 4) + k2) | ((p & 0x00800080u) << 8); }

MX8_FN void mx8_decode8(uint32_t lo, uint32_t hi, int sb, uint32_t* w) {
  // the common case in one test per word: (magnitude & 0x78) + 0x78 reaches bit 7 exactly when the exponent field is not zero
  if (sb >= 7 && ((((lo & 0x78787878u) + 0x78787878u) & ((hi & 0x78787878u) + 0x78787878u)) & 0x80808080u) == 0x80808080u) {
    const uint32_t k2 = (uint32_t)(sb - 7) * 0x00800080u;
    w[0] = mx8_decode_pair_normal((lo & 0xffu) | ((lo << 8) & 0x00ff0000u), k2);
    w[1] = mx8_decode_pair_normal(((lo >> 16) & 0xffu) | ((lo >> 8) & 0x00ff0000u), k2);
    w[2] = mx8_decode_pair_normal((hi & 0xffu) | ((hi << 8) & 0x00ff0000u), k2);
    w[3] = mx8_decode_pair_normal(((hi >> 16) & 0xffu) | ((hi >> 8) & 0x00ff0000u), k2);
    return;
  }
  w[0] = mx8_decode(lo & 0xffu, sb) | (mx8_decode((lo >> 8) & 0xffu, sb) << 16);
  w[1] = mx8_decode((lo >> 16) & 0xffu, sb) | (mx8_decode(lo >> 24, sb) << 16);
  w[2] = mx8_decode(hi & 0xffu, sb) | (mx8_decode((hi >> 8) & 0xffu, sb) << 16);
  w[3] = mx8_decode((hi >> 16) & 0xffu, sb) | (mx8_decode(hi >> 24, sb) << 16);
}

// largest |x| (bf16 bits, sign cleared) of eight packed bf16
MX8_FN uint32_t mx8_amax8(const uint32_t* w) {
  uint32_t m = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t a = w[i] & 0x7fffu, b = (w[i] >> 16) & 0x7fffu;
    m = a > m ? a : m;
    m = b > m ? b : m;
  }
  return m;
}

// eight packed bf16 under scale byte sb -> their 8 code bytes (lo, hi) and, in place, the eight x_hat
MX8_FN void mx8_encode8(uint32_t* w, int sb, uint32_t& lo, uint32_t& hi) {
  uint32_t c[8];
  for (int i = 0; i < 4; ++i) {
    c[2 * i] = mx8_encode(w[i] & 0xffffu, sb);
    c[2 * i + 1] = mx8_encode(w[i] >> 16, sb);
    w[i] = mx8_decode(c[2 * i], sb) | (mx8_decode(c[2 * i + 1], sb) << 16);
  }
  lo = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  hi = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
}
