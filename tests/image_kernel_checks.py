"""The raw-pixel kernels of csrc/image.hip (`llmseg_image_resize_u8`, `llmseg_image_resize_u8_filter`, `llmseg_clip_preprocess`, `llmseg_mask_union`):
case tables, references, the workspace decoder and the mutants.  CPU only; the HIP library is not imported here.

References.  Resampling: oracle/pil_resize.py (BILINEAR) and tests/image_frontend_checks.py (BICUBIC), both pinned against `PIL.Image.resize`.  The
header's "bit-identical to Pillow" holds per channel: Pillow premultiplies RGBA / LA images before resampling, the kernel does not, so the reference of 2
and 4 channels is the restatement applied to every channel on its own (which is what the restatements do with a [H, W, C] array).
`resample_m` / `taps_m` / `clip_m` / `union_m` restate the same arithmetic once more with a switch per mutant; tests/test_image_kernels_cpu.py proves that
without a mutant they equal the references on every case, and that every mutant changes something on every case it is declared for.

Every comparison of this suite is exact (bytes, int32 table entries, bf16 bit patterns): no constant is measured."""
import collections
import math

import numpy as np

from oracle import pil_resize
from tests import image_frontend_checks as fc

BILINEAR, BICUBIC = 0, 1                                   # LLMSEG_RESAMPLE_*
FILTERS = (BILINEAR, BICUBIC)
FNAME = {BILINEAR: "bilinear", BICUBIC: "bicubic"}
MAX_KSIZE = {BILINEAR: 64, BICUBIC: 256}                   # image.hip: MAX_TAPS / MAX_TAPS_CUBIC
BITS = 22
SENTINEL = 0xA5                                            # every byte of an input buffer outside the window
GUARD = 256                                                # bytes either side of every output and workspace buffer


# ------------------------------------------------------------------------------------------------------------------------ layout of the workspace
def align256(v):
    return (v + 255) & ~255


def ksize(filt, in_size, out_size):
    return int(math.ceil((2.0 if filt == BICUBIC else 1.0) * max(in_size / out_size, 1.0))) * 2 + 1


def accepted(filt, in_h, in_w, out_h, out_w):
    return ksize(filt, in_w, out_w) <= MAX_KSIZE[filt] and ksize(filt, in_h, out_h) <= MAX_KSIZE[filt]


def resize_workspace(filt, in_h, in_w, out_h, out_w, ch):
    """llmseg_image_resize_filter_workspace: horizontal table, vertical table, the uint8 intermediate [in_h][out_w][ch], each rounded up to 256 bytes."""
    return align256(out_w * (ksize(filt, in_w, out_w) + 2) * 4) + align256(out_h * (ksize(filt, in_h, out_h) + 2) * 4) + align256(in_h * out_w * ch)


def clip_workspace(h, w, size):
    nh, nw = fc.clip_resized_size(h, w, size)
    return align256(size * (ksize(BICUBIC, w, nw) + 2) * 4) + align256(size * (ksize(BICUBIC, h, nh) + 2) * 4) + align256(h * size * 3)


def decode_table(ws, offset, rows, ks):
    """ws uint8 [bytes] (the workspace after a call) -> (first index int32 [rows], count int32 [rows], taps int32 [rows, ks]) of the table at byte `offset`."""
    t = np.frombuffer(np.ascontiguousarray(ws[offset:offset + rows * (ks + 2) * 4]).tobytes(), dtype=np.int32).reshape(rows, ks + 2)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2:].copy()


def ref_coeffs(filt, in_size, out_size):
    return pil_resize.coeffs(in_size, out_size) if filt == BILINEAR else fc.coeffs(in_size, out_size)


def ref_resize(filt, img, out_h, out_w):
    """img uint8 [h, w, ch] -> uint8 [out_h, out_w, ch] by the pinned restatements (always a new array)."""
    out = pil_resize.resize_bilinear_u8(img, out_h, out_w) if filt == BILINEAR else fc.resize_bicubic_u8(img, out_h, out_w)
    return np.array(out, copy=True)


def table_diff(a, b):
    """entries that differ between two (first, count, taps) triples; a different shape counts as one"""
    if any(x.shape != y.shape for x, y in zip(a, b)):
        return 1
    return int(sum((np.asarray(x, np.int64) != np.asarray(y, np.int64)).sum() for x, y in zip(a, b)))


# --------------------------------------------------------------------------------------------------------------------- the tap-table sweep (A)
BIG_PAIRS = [(640, 335), (427, 224), (1500, 224), (2250, 336), (1024, 683), (333, 1024), (97, 28)]
BOUNDARY_OK = {BILINEAR: [(31, 1)], BICUBIC: [(127, 2), (63, 1)]}           # ksize 63; 255, 253
BOUNDARY_REFUSED = {BILINEAR: [(32, 1), (64, 2)], BICUBIC: [(128, 2), (64, 1)]}   # ksize 65, 65; 257, 257


def sweep_pairs(filt):
    """(in, out) of the horizontal sweep; a pair with in == out takes the copy route and writes no table"""
    return [(i, o) for i in range(1, 25) for o in range(1, 25)] + BOUNDARY_OK[filt] + BIG_PAIRS


def vertical_pairs(filt):
    return [(1, 5), (5, 1), (2, 3), (3, 2), (7, 24), (24, 7), (23, 24), (24, 23), (13, 1), (1, 24), (17, 16), (4, 24), (24, 5)] + BOUNDARY_OK[filt] + \
        [(640, 335), (427, 224), (333, 1024), (97, 28), (1500, 224)]


# ------------------------------------------------------------------------------------------- the restatement with one switch per mutant (E)
def _filter(filt, x, a):
    x = -x if x < 0.0 else x
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def taps_m(filt, in_size, out_size, mut=""):
    """`ref_coeffs` restated; mut in TABLE_MUTANTS changes one thing"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = (1.0 if filt == BILINEAR or mut == "support" else 2.0) * fs
    ks = int(math.ceil(support)) * 2 + 1
    a = -0.75 if mut == "a075" else -0.5
    ss = 1.0 / fs
    xmin = np.zeros(out_size, np.int32); cnt = np.zeros(out_size, np.int32); kk = np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = (xx + (0.0 if mut == "centre" else 0.5)) * scale
        lo = int(center - support + 0.5)
        if mut != "lo":
            lo = max(lo, 0)
        hi = min(int(center + support + 0.5), in_size)
        n = max(min(hi - lo, ks), 0)
        w = [_filter(filt, (x + lo - center + 0.5) * ss, a) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0 and mut != "nonorm":
            w = [v / ww for v in w]
        xmin[xx], cnt[xx] = lo, n
        kk[xx, :n] = [int(-0.5 + v * (1 << BITS)) if v < 0 and mut != "neground" else int(0.5 + v * (1 << BITS)) for v in w]
    return xmin, cnt, kk


def _pass_m(src, tab, horiz, mut):
    """src int64 [rows, cols, ch] -> the pass along the columns (horiz) or the rows, with the kernel's clip8 and its int32 -> uint8 store"""
    xmin, cnt, kk = tab
    s = np.moveaxis(src, 1 if horiz else 0, 0)
    if horiz and mut == "choff":
        s = np.repeat(s[..., :1], s.shape[-1], axis=-1)                    # every channel reads channel 0
    out = np.empty((len(xmin),) + s.shape[1:], np.int64)
    for xx in range(len(xmin)):
        n = int(cnt[xx])
        acc = np.tensordot(kk[xx, :n].astype(np.int64), s[xmin[xx]:xmin[xx] + n], axes=(0, 0)) + (0 if mut == "noround" else 1 << (BITS - 1))
        out[xx] = acc >> BITS
    if mut != "noclamp0":
        out = np.maximum(out, 0)
    if mut != "noclamp255":
        out = np.minimum(out, 255)
    return np.moveaxis(out & 0xFF, 0, 1 if horiz else 0)


def window(buf, off, stride, h, w, ch, dense=False):
    """the [h, w, ch] window of the flat byte buffer `buf` that starts at byte `off` with `stride` bytes between rows"""
    st = w * ch if dense else stride
    return np.stack([buf[off + y * st: off + y * st + w * ch].reshape(w, ch) for y in range(h)])


def resample_m(filt, buf, off, stride, h, w, ch, out_h, out_w, mut=""):
    """the resampler as the C ABI sees it: a window of a byte buffer -> uint8 [out_h, out_w, ch]; mut in IMAGE_MUTANTS changes one thing"""
    x = window(buf, off + (ch if mut == "shift" else 0), stride, h, w, ch, dense=mut == "dense").astype(np.int64)
    order = ("v", "h") if mut == "vfirst" else ("h", "v")
    for p in order:
        if p == "h" and out_w != w:
            x = _pass_m(x, taps_m(filt, w, out_w, mut if mut in TABLE_MUTANTS else ""), True, mut)
        if p == "v" and out_h != h:
            x = _pass_m(x, taps_m(filt, h, out_h, mut if mut in TABLE_MUTANTS else ""), False, mut)
    return x.astype(np.uint8)


# mutant -> what it is.  Table mutants are judged on the decoded tap tables, image mutants on the output bytes.
TABLE_MUTANTS = {
    "centre": "centre without its + 0.5",
    "support": "bilinear support used for bicubic",
    "a075": "a = -0.75 in the bicubic polynomial",
    "neground": "+0.5 rounding on negative taps",
    "lo": "first index not clamped at 0",
    "nonorm": "weights not normalised by their sum",
}
IMAGE_MUTANTS = {
    "centre": TABLE_MUTANTS["centre"],
    "vfirst": "vertical pass first",
    "noclamp0": "no clamp at 0",
    "noclamp255": "no clamp at 255",
    "noround": "no 2^21 rounding term",
    "dense": "window read with the dense stride",
    "shift": "window origin one pixel to the right",
    "choff": "channel offset dropped",
}


def table_mutant_applies(mut, filt, i, o):
    """a pair with i == o has no table.  With one input sample every row is {0, 1, 2^22} whatever the weights are; only the unclamped first index shows."""
    if i == o:
        return False
    up = i < o
    if mut == "lo":                                                             # int(centre - support + 0.5) <= -1 at output index 0
        return filt == BICUBIC or i >= 3 * o
    if mut == "nonorm":                                                        # a clipped edge row of an up-scale, any row of a down-scale
        return True
    if i == 1:
        return False
    if mut == "support":
        return filt == BICUBIC
    if mut == "a075":                                                          # two samples get 1/2 each whatever the polynomial
        return filt == BICUBIC and i >= 3
    if mut == "neground":                                                      # a negative tap that is no multiple of 2^-22: not at the exact-ratio grids of tiny sizes
        return filt == BICUBIC and min(i, o) >= 5 and max(i, o) % min(i, o) != 0
    if mut == "centre":
        return True
    raise KeyError(mut)


Case = collections.namedtuple("Case", "name filt h w oh ow ch content lead extra seed")


def _content(c):
    """the window's pixels, uint8 [h, w, ch]"""
    h, w, ch, kind = c.h, c.w, c.ch, c.content
    if kind == "random":
        return np.random.default_rng(c.seed).integers(0, 256, (h, w, ch), dtype=np.uint8)
    if kind in ("block0", "block1"):
        return np.ascontiguousarray(np.broadcast_to(fc.block_image(h, w, int(kind[-1]), block=3)[..., :1], (h, w, ch)))
    if kind.startswith("const"):
        return np.full((h, w, ch), int(kind[5:]), np.uint8)
    field, where = kind.split("@")                                             # "on@corner": one 255 on a 0 field; "off@edge": one 0 on a 255 field
    a = np.full((h, w, ch), 0 if field == "on" else 255, np.uint8)
    y, x = {"corner": (0, 0), "edge": (0, w // 2), "interior": (h // 2, w // 2)}[where]
    a[y, x] = 255 if field == "on" else 0
    return a


def make_input(c):
    """-> (buf uint8 [bytes], off, stride, img uint8 [h, w, ch]): the window inside a larger buffer of SENTINEL bytes, two spare rows above and one below; an odd `lead` puts the window at an odd byte of the buffer"""
    stride = c.w * c.ch + c.extra
    buf = np.full(((c.h + 3) * stride + c.lead + 16,), SENTINEL, np.uint8)
    off = 2 * stride + c.lead
    img = _content(c)
    for y in range(c.h):
        buf[off + y * stride: off + y * stride + c.w * c.ch] = img[y].reshape(-1)
    return buf, off, stride, img


GAP_SHAPES = [(1, 1, 1, 1, 3), (1, 7, 1, 20, 1), (37, 1, 1, 1, 3), (37, 53, 1, 1, 3), (127, 3, 2, 3, 3), (3, 127, 3, 2, 1), (64, 64, 32, 32, 3), (32, 32, 64, 64, 2),
              (96, 5, 32, 5, 4), (101, 100, 100, 101, 3), (100, 101, 101, 100, 1), (2, 2, 5, 5, 3), (5, 5, 2, 2, 3), (31, 31, 31, 7, 3), (31, 31, 7, 31, 3),
              (9, 300, 9, 7, 3), (1, 63, 1, 1, 3), (255, 2, 4, 2, 1)]
CLASS_SHAPES = {"up": (9, 11, 20, 23), "down": (23, 20, 9, 11), "horizontal": (7, 19, 7, 8), "vertical": (19, 7, 8, 7)}
CONTENTS = ["block0", "block1", "const0", "const1", "const254", "const255"] + [f"{f}@{p}" for f in ("on", "off") for p in ("corner", "edge", "interior")]


def resample_cases():
    """every case of B for both filters; `refused` ones (a tap count over the filter's limit) are checked as refusals.  lead = bytes in front of the window
    inside its row (odd: the window starts at an odd address), extra = bytes of the row behind the window (0: dense rows)."""
    cs = []
    for filt in FILTERS:
        f = FNAME[filt]
        for n, (h, w, oh, ow, ch) in enumerate(GAP_SHAPES):
            cs.append(Case(f"{f}-{h}x{w}-{oh}x{ow}-c{ch}", filt, h, w, oh, ow, ch, "random", 0, 0, 500 + n))
        for cls, (h, w, oh, ow) in CLASS_SHAPES.items():
            for ch in (1, 2, 3, 4):
                cs.append(Case(f"{f}-{cls}-c{ch}-odd-window", filt, h, w, oh, ow, ch, "random", 2 * ch + 1, 7, 600 + ch))
            for kind in CONTENTS:
                cs.append(Case(f"{f}-{cls}-{kind}", filt, h, w, oh, ow, 3, kind, 4, 5, 0))
        for ch in (1, 2, 3, 4):
            cs.append(Case(f"{f}-copy-c{ch}-strided", filt, 6, 9, 6, 9, ch, "random", 3, 11, 700 + ch))
        for (i, o) in BOUNDARY_OK[filt]:
            cs.append(Case(f"{f}-limit-h{i}-{o}", filt, 3, i, 3, o, 3, "random", 1, 2, 800 + i))
            cs.append(Case(f"{f}-limit-v{i}-{o}", filt, i, 3, o, 3, 2, "random", 1, 2, 900 + i))
    return cs


def case_refused(c):
    return not accepted(c.filt, c.h, c.w, c.oh, c.ow)


def image_mutant_applies(mut, c):
    do_h, do_v = c.ow != c.w, c.oh != c.h
    random, strided = c.content == "random", c.extra > 0 and c.h > 1
    up = c.oh > c.h and c.ow > c.w                                             # a step edge overshoots both ways when it is up-scaled
    if mut == "dense":
        return strided
    if mut == "shift":                                                         # one output pixel averages the shift away
        return random and (c.oh * c.ow > 1 or c.w == 1)
    if not (do_h or do_v):
        return False
    if mut == "centre":
        return random and max(c.h, c.w) > 1 and (c.w > 1 if do_h and not do_v else True) and (c.h > 1 if do_v and not do_h else True)
    if mut == "vfirst":
        return random and do_h and do_v and c.oh * c.ow * c.ch >= 300         # the order shows only in the intermediate's rounding: a few bytes in a hundred
    if mut == "noround":
        return random and c.h * c.w > 1
    if mut == "choff":
        return random and c.ch > 1 and do_h
    if mut == "noclamp0":                                                      # a 255 next to zeros under a negative lobe
        return c.filt == BICUBIC and (c.content.startswith("block") and up or c.content.startswith("on@"))
    if mut == "noclamp255":
        return c.filt == BICUBIC and (c.content.startswith("block") and up or c.content.startswith("off@"))
    raise KeyError(mut)


# ------------------------------------------------------------------------------------------------------------------------------ CLIP preprocess (C)
# fc.CLIP_CASES, then: size * long / short an exact integer (both orientations); the (113, 97, 7) -> 8 row of tests/test_image_frontend_cpu.py; a quotient just
# below an integer (7 * 113 / 99 = 7.99 -> 7 = size: the long side is resampled to the window itself); odd / even `top` and `left`; a tall and a wide image whose
# window lies far from both borders of the resampled axis
CLIP_EXTRA = [(448, 224, 28), (200, 300, 28), (113, 97, 7), (113, 99, 7), (99, 113, 7), (57, 28, 28), (58, 28, 28), (28, 57, 28), (28, 58, 28), (400, 50, 28), (50, 400, 28)]
CLIP_CASES = list(fc.CLIP_CASES) + CLIP_EXTRA


def clip_geometry(h, w, size, mut=""):
    short, long = (w, h) if w <= h else (h, w)
    q = size * long / short
    new_long = int(round(q)) if mut == "round" else int(q)
    nh, nw = (new_long, size) if w <= h else (size, new_long)
    r = 1 if mut == "origin" else 0
    return nh, nw, (nh - size + r) // 2, (nw - size + r) // 2


def clip_image(h, w, seed):
    return fc.random_image(h, w, seed)


def _bf16_bits(x32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x32)).to(torch.bfloat16).view(torch.int16).numpy()


def normalise_bits(win, mean, std, mut=""):
    """win uint8 [S, S, 3] -> int16 [3, S, S], the bf16 bit patterns: r = float32(double(u) / 255 as a product), (r - mean) / std in IEEE fp32, one rounding to bf16"""
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    if mut == "swap":
        m, s = m[::-1].copy(), s[::-1].copy()
    if mut == "u255f32":
        r = win.astype(np.float32) * np.float32(1.0 / 255.0)
    else:
        r = (win.astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
    v = (r - m) / s
    assert v.dtype == np.float32
    return _bf16_bits(v.transpose(2, 0, 1))


def clip_ref_bits(img, size, mean=fc.CLIP_MEAN, std=fc.CLIP_STD):
    return normalise_bits(fc.clip_window(img, size), mean, std)


def clip_m(img, size, mean=fc.CLIP_MEAN, std=fc.CLIP_STD, mut=""):
    """`clip_ref_bits` restated over `resample_m`'s passes with one switch per CLIP mutant"""
    h, w = img.shape[:2]
    nh, nw, top, left = clip_geometry(h, w, size, mut)
    x = img.astype(np.int64)
    if nw != w:
        x = _pass_m(x, taps_m(BICUBIC, w, nw), True, "")
    x = x[:, left:left + size]
    if mut == "toprow":                                                        # the rows handed on start one row late while the indices still count from the first
        x = np.concatenate([x[1:], x[-1:]], 0)
    if nh != h:
        xmin, cnt, kk = (t[top:top + size] for t in taps_m(BICUBIC, h, nh))
        x = _pass_m(x, (xmin, cnt, kk), False, "")
    else:
        x = x[top:top + size]
    return normalise_bits(x.astype(np.uint8), mean, std, mut)


CLIP_MUTANTS = {
    "origin": "crop origin (resized - size + 1) // 2",
    "round": "round instead of int for the long side",
    "swap": "mean / std of channels 0 and 2 swapped",
    "u255f32": "u / 255 in fp32 (u times the fp32 reciprocal)",
    "toprow": "window rows short by one at the top",
}
# u / 255 in fp32.  As one IEEE fp32 division it equals float32(double(u) * (1 / 255)) on all 256 bytes: that is no mutant.  As u * float32(1 / 255) it differs by one
# fp32 unit on 126 byte values, which bf16 hides under the CLIP statistics on every byte.  It shows where r - mean cancels: with mean = u0 / 256 the difference at
# u = u0 - 1 is a few fp32 units of a value near 2^-14.  U255 is that case: every byte value in every channel at size = h = w (no resampling) under U255_MEAN /
# U255_STD (both exact in fp32); tests/test_image_kernels_cpu.py recomputes the three elements that differ.
U255_SIZE = 16
U255_MEAN, U255_STD = (128 / 256, 223 / 256, 239 / 256), (1.0, 0.5, 0.25)


def u255_image():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return np.ascontiguousarray(np.stack([v, v[::-1], v.T], -1))


def clip_mutant_applies(mut, h, w, size):
    nh, nw, top, left = clip_geometry(h, w, size)
    if mut == "origin":
        return (nh - size) % 2 == 1 or (nw - size) % 2 == 1
    if mut == "round":
        return clip_geometry(h, w, size, "round")[:2] != (nh, nw)
    if mut in ("swap", "toprow"):
        return True
    if mut == "u255f32":
        return False                                                           # judged on U255_CASE alone
    raise KeyError(mut)


# ----------------------------------------------------------------------------------------------------------------------------------- mask union (D)
UNION_N = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 4095: (63, 65), 4096: (64, 64), 4097: (17, 241), 12610: (97, 130)}
UNION_K = (1, 2, 33)
MASK_VALUES = np.array([0, 1, 0x80, 0xFF], np.uint8)
UNION_SENTINEL = 0xFF                                      # every pixel of a mask that no selection row marks


def union_case(n, K):
    """-> (masks uint8 [K, H, W], sel uint8 [4, K]: none / single / random / random with bytes other than 1, sel_all uint8 [1, K]).  Every mask has a non-zero last
    pixel and a non-zero value other than 1, and about three quarters zeros."""
    H, W = UNION_N[n]
    g = np.random.default_rng(1000 * K + n)
    masks = MASK_VALUES[g.integers(0, 4, (K, n)) * (g.random((K, n)) < 0.3)]
    masks[:, -1] = 0x80
    if n > 1:
        masks[:, 0] = np.where(np.arange(K) % 2 == 0, 0xFF, 0)
    sel = np.zeros((4, K), np.uint8)
    sel[1, (n + K) % K] = 1
    sel[2] = g.random(K) < 0.5
    sel[2, 0] = 1
    sel[3] = np.array([0, 2, 0x80, 0xFF], np.uint8)[g.integers(0, 4, K)]
    sel[3, K - 1] = 0x80
    if K > 1:
        sel[2, K - 1] = 0
        sel[3, 0] = 0
    return masks.reshape(K, H, W), sel, np.ones((1, K), np.uint8)


def with_sentinel(masks, sel):
    """masks with every mask that no row of `sel` marks filled with UNION_SENTINEL: the kernel must not read them"""
    m = masks.copy()
    m[~(sel != 0).any(0)] = UNION_SENTINEL
    return m


def union_m(masks, sel, mut=""):
    K = masks.shape[0]
    n = masks[0].size
    flat = masks.reshape(K, n)
    on = flat == 1 if mut == "eq1" else flat != 0
    C = sel.shape[0]
    out = np.zeros((C, n), np.uint8)
    for c in range(C):
        row = sel[(c + 1) % C] if mut == "neighbour" else sel[c]
        out[c] = on[row != 0].any(0) if (row != 0).any() else 0
    if mut == "tail":
        out[:, n - n % 16:] = 0
    return out.reshape((C,) + masks.shape[1:])


UNION_MUTANTS = {"eq1": "== 1 instead of != 0", "neighbour": "selection row of the neighbouring output", "tail": "tail of fewer than 16 pixels dropped"}


def union_mutant_applies(mut, n, K):
    return {"eq1": True, "neighbour": True, "tail": n % 16 != 0}[mut]
