"""The MXFP8 rule of include/llmseg_hip.h (E4M3 elements, one E8M0 scale byte per block of 32) on the CPU, by integer work on bf16 bits, and the inputs the
tests of the quantiser and of the decode step on the packed cache share.  No import of the HIP library.

`quantize` is the rule; `float8_reference` is the same rule spelled with `torch.float8_e4m3fn` of x / 2^e (tests/test_kv_mxfp8_cpu.py pins the two against each
other and against hand cases); `blocks` builds the block kinds a quantiser can get wrong."""
import torch

BF = torch.bfloat16
BLOCK = 32
NAN_CODE, NAN_SCALE = 0x7F, 0xFF                           # what poisoned cache bytes hold: the E4M3 NaN code under the E8M0 NaN scale
_MSB = torch.tensor([0] + [k.bit_length() - 1 for k in range(1, 256)], dtype=torch.int32)


def bits(x):
    """bf16 tensor -> its bit patterns as int32 in [0, 65536)"""
    assert x.dtype == BF
    return x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def from_bits(u):
    return (u & 0xFFFF).to(torch.int32).where(u < 0x8000, u - 0x10000).to(torch.int16).view(BF)


def scale_byte(amax_bits):
    """|bf16| bits of a block's amax -> e + 127: e = E - 8 for a mantissa field <= 96 (m <= 1.75), else E - 7; never below -127; zero and subnormal amax: -127"""
    ef, man = amax_bits >> 7, amax_bits & 0x7F
    sb = (ef - 8 + (man > 96).to(torch.int32)).clamp(min=0)
    return torch.where(ef == 0, torch.zeros_like(sb), sb)


def encode(u, sb):
    """bf16 bits u under scale byte sb (broadcastable) -> E4M3 codes, int32"""
    a = u & 0x7FFF
    ef = a >> 7
    sig = (a & 0x7F) | torch.where(ef > 0, 0x80, 0)
    s = ef.clamp(min=1) - 7 - sb                           # |x| / 2^e = sig * 2^s
    ey = _MSB[sig.long()] + s
    be = ey.clamp(min=-6) + 7
    shift = be - 10 - s
    up = torch.bitwise_left_shift(sig, (-shift).clamp(min=0, max=8))
    sh = shift.clamp(min=1, max=16)
    down = torch.bitwise_right_shift(sig + torch.bitwise_left_shift(torch.ones_like(sh), sh - 1) - 1 + (torch.bitwise_right_shift(sig, sh) & 1), sh)
    code = (((be - 1) << 3) + torch.where(shift <= 0, up, down)).clamp(max=0x7E)
    code = torch.where(sig == 0, torch.zeros_like(code), code)
    return torch.where(code == 0, code, code | ((u >> 8) & 0x80))


def decode(code, sb):
    """E4M3 codes under scale byte sb -> the bf16 bits of element * 2^e; below the smallest normal bf16: +0"""
    mag = code & 0x7F
    p = (mag >= 2).to(torch.int32) + (mag >= 4).to(torch.int32)
    normal = mag >= 8
    ex = torch.where(normal, (mag >> 3) + sb - 7, p + sb - 9)
    mb = torch.where(normal, (mag & 7) << 4, torch.bitwise_left_shift(mag, 7 - p) & 0x7F)
    out = ((code & 0x80) << 8) | (ex.clamp(min=0) << 7) | mb
    return torch.where((mag != 0) & (ex >= 1), out, torch.zeros_like(out))


def quantize(x):
    """x bf16 [..., D], D % 32 == 0 -> (codes uint8 [..., D], scale bytes uint8 [..., D / 32], x_hat bf16 [..., D])"""
    assert x.dtype == BF and x.shape[-1] % BLOCK == 0
    u = bits(x).view(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    sb = scale_byte((u & 0x7FFF).amax(-1))
    code = encode(u, sb[..., None])
    return code.to(torch.uint8).view(x.shape), sb.to(torch.uint8), from_bits(decode(code, sb[..., None])).view(x.shape)


def dequantize(q, scale):
    """(codes uint8 [..., D], scale bytes uint8 [..., D / 32]) -> x_hat bf16 [..., D]"""
    c = q.to(torch.int32).view(*q.shape[:-1], q.shape[-1] // BLOCK, BLOCK)
    return from_bits(decode(c, scale.to(torch.int32)[..., None])).view(q.shape)


def float8_reference(x, sb):
    """torch.float8_e4m3fn of x / 2^e under the given scale bytes -> (codes uint8 with -0 stored as +0, x_hat fp64 = element * 2^e)"""
    e = sb.to(torch.int32) - 127
    xb = x.float().view(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    y = torch.ldexp(xb, -e[..., None])                     # exact: a power of two, and |y| <= 448
    f8 = y.to(torch.float8_e4m3fn)
    code = f8.view(torch.uint8)
    code = torch.where(code == 0x80, torch.zeros_like(code), code)
    return code.view(x.shape), torch.ldexp(f8.double(), e[..., None].double()).view(x.shape)


def blocks(n, seed):
    """n blocks of 32 bf16 values [n, 32], cycling through the kinds: random over ~30 binades; all zero; amax = 448 * 2^k exactly and the next bf16 above it
    (m = 1.7578125); ties of the E4M3 grid (1.0625, 1.1875, 2^-10 scaled into the block's binade); bf16-subnormal and tiny elements beside a large amax; -0 and
    values that round to zero with a negative sign; a block whose amax is a bf16 subnormal"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, BLOCK, generator=g) * torch.exp2(torch.randint(-15, 15, (n, 1), generator=g).float())
    k = torch.randint(-12, 12, (n,), generator=g).float()
    kind = torch.arange(n) % 8
    for i in range(n):
        s = float(torch.exp2(k[i]))
        if kind[i] == 1:
            x[i] = 0.0
        elif kind[i] == 2:                                  # amax on the boundary: e = E - 8, y = 448
            x[i] = x[i].clamp(-1, 1) * s
            x[i, 5] = -448.0 * s / 256
        elif kind[i] == 3:                                  # the next bf16 above it: e = E - 7
            x[i] = x[i].clamp(-1, 1) * s
            x[i, 7] = 1.7578125 * s
        elif kind[i] == 4:                                  # amax = 256 s: e = k, so y = x / s hits the grid's ties
            x[i, :8] = torch.tensor([256.0, 1.0625, 1.1875, -1.0625, 2.0 ** -10, 3 * 2.0 ** -10, -(2.0 ** -10), 2.0 ** -9]) * s
            x[i, 8:] = x[i, 8:].clamp(-1, 1) * s
        elif kind[i] == 5:                                  # bf16 subnormals and tiny normals beside a large amax
            x[i, :4] = torch.tensor([2.0 ** -133, -(2.0 ** -130), 2.0 ** -126, 100.0])
        elif kind[i] == 6:
            x[i, :4] = torch.tensor([-0.0, -(2.0 ** -40), 0.0, 1.0])
        elif kind[i] == 7 and i % 16 == 7:                  # the whole block below the normal range: scale byte 0
            x[i] = torch.randint(-127, 128, (BLOCK,), generator=g).float() * 2.0 ** -133
    return x.to(BF)


def rows(shape, D, seed):
    """bf16 [*shape, D] made of `blocks`"""
    n = D // BLOCK
    for d in shape:
        n *= d
    return blocks(n, seed).view(*shape, D)
