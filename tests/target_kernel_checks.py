"""Edge tables, exact references, structural emulations and mutants for the training-target kernels (csrc/targets.hip: llmseg_rle_decode,
llmseg_gt_resample, llmseg_mask_targets, llmseg_resize_aa, the one-pass llmseg_proposal_targets) and the validation-metric kernels (csrc/head.hip:
llmseg_intersection_union, llmseg_union_resize_iou).  tests/test_target_kernels_cpu.py shows that the references are the oracle's, that the emulations
equal them and that every mutant is rejected by the case MUTANTS names for it; tests/test_target_kernels_gpu.py runs the kernels on the same tables.

What "equal" means.  Integer outputs (masks, gtp, counts, areas, the six I/U counts) and the IoU / IoP divisions of those integers: exactly.  Proposal
maps: `exact_maps` evaluates sum_j wy sum_i wx m from the float64 tap tables in np.longdouble (64-bit significand).  Every term is >= 0, so the true value
v is also sum |term|.  The kernel adds at most `taps` products per axis in float64 (one rounding per product, one per addition, fewer with fused
multiply-adds): |kernel's double - v| <= (2 taps + 2) 2^-53 v to first order; the longdouble evaluation itself is within (2 taps + 2) 2^-64 v.
DELTA_TERMS = 2 taps + 4 covers both and the second-order terms.  A pixel is DECIDED when v (1 - d) and v (1 + d), d = DELTA_TERMS 2^-53, round to the same
bf16 through fp32 (both roundings are monotone, so everything between them rounds alike): there the kernel must give that bf16 bit for bit; elsewhere
either of the two.  At most UNDECIDED_MAX of a case's pixels may be undecided -- a condition on the inputs, checked on the reference alone."""
import functools
import zlib

import numpy as np
import torch

from llmseg_amd import targets as ht
from oracle import losses as olosses, targets as ot

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "exact_maps needs the x87 80-bit long double"
U53 = 2.0 ** -53
UNDECIDED_MAX = 1e-4
LIMITS = dict(ht.FUSED_LIMITS)
TG_ROWS, TG_MAXW, TG_WREG = 4, 2048, 12          # csrc/targets.hip
LDS_JUNK = 0xAA                                  # what the emulation finds in LDS bytes nobody staged (the hardware promises nothing)


# ------------------------------------------------------------------ tables ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def aa_tables(side, out):
    first, count, w = ht.aa_taps(side, out)
    return first, count, w, int(w.shape[1])


@functools.lru_cache(maxsize=None)
def gap_tables(side, out, step):
    """caller-made tables the C ABI also takes: ONE tap of weight 1 at y = step * o.  Between two windows lie step - 1 rows that no window reads:
    the only way to reach the fused kernel's counts-only tail (with antialiasing tables the last window of a slice always reaches the first row of
    the next: end[o] = int(c + s + .5) >= int(c + scale - s + .5) = first[o + 1] because s >= scale / 2)."""
    assert step * (out - 1) < side
    first = (np.arange(out) * step).astype(np.int32)
    return first, np.ones(out, np.int32), np.ones((out, 1), np.float64), 1


def tables_of(c):
    side = max(c["H"], c["W"])
    return gap_tables(side, c["out"], c["gap"]) if c.get("gap") else aa_tables(side, c["out"])


def n_slices(K, out):
    return int(min(max(1, 1024 // K), max(1, out // 16)))


def ring_of(taps):
    return 16 if taps + TG_ROWS <= 16 else 32


def fused_takes(c):
    taps = tables_of(c)[3]
    return c["out"] <= LIMITS["out_size"] and taps <= LIMITS["taps"] and c["W"] <= LIMITS["width"]


def slice_rows(c):
    """[(oy_a, oy_b, cnt_a, cnt_b)] of the fused kernel's grid.y"""
    y0 = tables_of(c)[0]
    ns, OS, H = n_slices(c["K"], c["out"]), c["out"], c["H"]
    res = []
    for s in range(ns):
        a, b = s * OS // ns, (s + 1) * OS // ns
        res.append((a, b, 0 if s == 0 else int(y0[a]), H if s == ns - 1 else min(H, int(y0[b]))))
    return res


def _case(name, H, W, out, n_masks=3, order=None, gts=((1.0, 1.0),), values=(1,), misalign=0, gap=0, gt_values=(0, 1), note=""):
    """order: None (identity over all masks) or a list of indices.  gts: (Hg / H, Wg / W) factors or explicit (Hg, Wg) ints."""
    K = n_masks if order is None else len(order)
    g = []
    for a, b in gts:
        g.append((a, b) if isinstance(a, int) and isinstance(b, int) and not isinstance(a, bool) else (max(1, int(round(H * a))), max(1, int(round(W * b)))))
    return dict(name=name, H=H, W=W, out=out, n_masks=n_masks, order=None if order is None else list(order), K=K, gts=g, values=tuple(values),
                misalign=misalign, gap=gap, gt_values=tuple(gt_values), note=note)


_ONE = ((1.0, 1.0),)
CASES = [
    # staging path
    _case("w40_scalar_staging", 24, 40, 16, note="W % 16 = 8: scalar staging, partial last chunk"),
    _case("w48_vector", 32, 48, 16, note="16-byte loads"),
    _case("w48_base_plus_8", 32, 48, 16, misalign=8, note="the same masks 8 bytes into a buffer: vec_ok false by address (masks AND gtp)"),
    _case("w1", 9, 1, 16), _case("w15", 12, 15, 16), _case("w17", 12, 17, 16),
    # taps and ring
    _case("side80_11taps", 80, 64, 16, note="register weights, RING 16"),
    _case("side81_13taps", 81, 64, 16, note="scalar weights, RING 32"),
    _case("side112_15taps", 112, 96, 16, note="windows of 14 rows: 14 + 3 staged ahead need more than 16 ring rows"),
    _case("side208_27taps", 208, 160, 16, note="the last tap count the entry point takes"),
    _case("side209_29taps", 209, 100, 16, note="refused: Python falls back to the three kernels"),
    # slices
    _case("out48_k2", 96, 80, 48, n_masks=2, note="ns 3, 16-row slices"),
    _case("out40_k3", 90, 64, 40, n_masks=3, note="ns 2"),
    _case("out100_k1", 150, 128, 100, n_masks=1, gts=_ONE, note="ns 6, slices of 16 and 17 rows; K = 1: the only block adds the gt area"),
    _case("out48_k400", 20, 20, 48, n_masks=400, note="ns 2, capped by K; upscaling"),
    _case("gap5_tail", 160, 32, 32, n_masks=2, gap=5, note="caller tables with gaps: rows 76..79 of slice 0 are counted by the tail only"),
    # padding
    _case("pad_below_8x64", 8, 64, 32, note="slice 1 lies in the padding: owns no rows, writes zeros"),
    _case("pad_right_64x8", 64, 8, 32, note="columns beyond W"),
    _case("h1", 1, 40, 16), _case("h3", 3, 40, 16), _case("h5", 5, 40, 16, note="nrows 4 + 1"), _case("1x1", 1, 1, 16, n_masks=1),
    # upscaling
    _case("up_10x12", 10, 12, 32, note="3 taps, repeated y0, ns 2"),
    # width limit
    _case("w2048", 4, 2048, 256, n_masks=2, note="17 taps, windows at xs up to 2036"),
    _case("w2049", 4, 2049, 256, n_masks=2, note="refused: falls back"),
    # byte values
    _case("bytes_0_255", 32, 48, 16, values=(255,)),
    _case("bytes_odd", 24, 40, 16, values=(2, 0x10, 0x80, 0x7f), n_masks=4, note="every non-zero byte is inside"),
    # order
    _case("order_perm", 32, 48, 16, n_masks=5, order=(3, 0, 4, 2, 1)),
    _case("order_drop", 24, 40, 16, n_masks=6, order=(4, 1, 5)),
    _case("order_dup", 32, 48, 16, n_masks=4, order=(2, 2, 0, 3, 2)),
    # ground truths
    _case("gt0", 32, 48, 16, gts=(), note="maps only, NULL outputs"),
    _case("gt4", 24, 40, 16, gts=((1.0, 1.0), (2.0, 2.0), (0.5, 0.5), (1.5, 0.7)), gt_values=(0, 1, 2, 255)),
    _case("gt5", 24, 40, 16, gts=((1.0, 1.0), (2.0, 0.5), (0.5, 2.0), (1, 1), (1.3, 1.3)), gt_values=(0, 1, 2, 255), note="host split: 4 fused + 1 mask_targets"),
    _case("gt9", 32, 48, 16, gts=((1.0, 1.0), (2.0, 1.5), (0.5, 0.5), (1.5, 0.7), (0.7, 1.5), (1.25, 1.25), (3.0, 0.3), (1.0, 2.0), (1.1, 0.9)), gt_values=(0, 1, 2, 255), note="host split: 4 + 5"),
]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


def _rng(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


@functools.lru_cache(maxsize=None)
def masks_of(name):
    """uint8 [n_masks, H, W].  Rectangles with holes (values from c['values']); mask 1 is empty when there are >= 3; every mask gets set pixels on each
    slice's first owned input row and on the row before it, so that a row counted twice or not at all changes a count."""
    c = CASE[name]
    if name == "w48_base_plus_8":
        return masks_of("w48_vector")
    rng = _rng(name)
    n, H, W = c["n_masks"], c["H"], c["W"]
    m = np.zeros((n, H, W), np.uint8)
    vals = np.array(c["values"], np.uint8)
    for k in range(n):
        ya, xa = int(rng.integers(0, max(1, H // 2))), int(rng.integers(0, max(1, W // 2)))
        yb, xb = int(rng.integers(ya + 1, H + 1)), int(rng.integers(xa + 1, W + 1))
        blob = (rng.random((yb - ya, xb - xa)) > 0.2)
        m[k, ya:yb, xa:xb] = blob * vals[rng.integers(0, len(vals), blob.shape)]
        for (_, _, ca, _) in slice_rows(c)[1:]:
            for y in (ca - 1, ca):
                if 0 <= y < H:
                    on = rng.random(W) > 0.3
                    on[k % W] = True
                    m[k, y] = np.where(on, vals[k % len(vals)], m[k, y])
        m[k, H - 1, W - 1] = vals[0]                                   # the last byte of the image
    if n >= 3:
        m[1] = 0
    if name == "w2048":
        m[:, :, 2036:] = vals[0]                                       # the windows at the right border see set pixels
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def gts_of(name):
    """list of uint8 [Hg, Wg] with values from c['gt_values'] (non-zero = object); the last of >= 2 is empty."""
    c = CASE[name]
    rng = _rng(name, 1)
    res = []
    vals = np.array(c["gt_values"], np.uint8)
    for i, (hg, wg) in enumerate(c["gts"]):
        g = vals[rng.integers(0, len(vals), (hg, wg))]
        if len(c["gts"]) >= 2 and i == len(c["gts"]) - 1:
            g = np.zeros_like(g)
        g.setflags(write=False)
        res.append(g)
    return res


def selected(name):
    c, m = CASE[name], masks_of(name)
    return m if c["order"] is None else m[np.array(c["order"])]


# ---------------------------------------------------------------- references ----------------------------------------------------------------
def ref_gtp(gt, H, W):
    """the ground truth on the proposals' grid: skimage's order-0 rule as the oracle restates it, then != 0"""
    return (ot.resize_nearest(gt, H, W) != 0).astype(np.uint8)


def ref_counts(segs, gtp):
    """-> counts int64 [K, 2] = (|seg & gt'|, |seg|), gt area, iou, iop (numpy divisions: 0 / 0 = nan)"""
    s = segs != 0
    cnt = np.stack([(s & (gtp != 0)[None]).reshape(len(s), -1).sum(1), s.reshape(len(s), -1).sum(1)], 1).astype(np.int64)
    G = int((gtp != 0).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        I, S = cnt[:, 0].astype(np.float64), cnt[:, 1].astype(np.float64)
        return cnt, G, I / (S + np.float64(G) - I), I / S


def _dense(first, count, w, limit):
    """[out, limit] longdouble: the taps as a matrix, samples at index >= limit (the zero padding) dropped"""
    D = np.zeros((len(first), limit), LD)
    for o in range(len(first)):
        for j in range(int(count[o])):
            if first[o] + j < limit:
                D[o, first[o] + j] = w[o, j]
    return D


def exact_maps(segs, out, tabs):
    """-> v longdouble [K, out, out] = sum_j wy[oy][j] sum_i wx[ox][i] (segs[k][y0 + j][x0 + i] != 0)"""
    first, count, w, _ = tabs
    K, H, W = segs.shape
    Dy, Dx = _dense(first, count, w, H), _dense(first, count, w, W)
    rows = np.matmul((segs != 0).astype(LD), Dx.T)                     # [K, H, out]
    return np.matmul(Dy[None], rows)                                   # [K, out, out]


def to_bf16_bits(v):
    """longdouble / float64 array -> the int16 bits of bf16(fp32(v)), both round-to-nearest-even"""
    f = np.asarray(v).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(f)).to(torch.bfloat16).view(torch.int16).numpy()


def delta_terms(taps):
    return 2 * taps + 4


def map_bounds(v, taps):
    """-> (lo, hi) int16 bits: the bf16 of v (1 - d) and of v (1 + d)"""
    d = LD(delta_terms(taps)) * LD(U53)
    return to_bf16_bits(v * (1 - d)), to_bf16_bits(v * (1 + d))


def maps_agree(bits, lo, hi):
    """number of pixels whose bits are neither bound (v >= 0: the bit patterns are ordered, and lo, hi are equal or neighbours)"""
    bits = np.asarray(bits)
    return int(((bits != lo) & (bits != hi)).sum())


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(v, lo, hi, undecided share, per ground truth (gtp, counts, area, iou, iop)); computed once, never modified"""
    c = CASE[name]
    segs, tabs = selected(name), tables_of(c)
    v = exact_maps(segs, c["out"], tabs)
    lo, hi = map_bounds(v, tabs[3])
    assert ((hi.astype(np.int32) - lo.astype(np.int32)) >= 0).all() and ((hi.astype(np.int32) - lo.astype(np.int32)) <= 1).all()
    per_gt = []
    for g in gts_of(name):
        gtp = ref_gtp(g, c["H"], c["W"])
        per_gt.append((gtp,) + ref_counts(segs, gtp))
    return dict(v=v, lo=lo, hi=hi, undecided=float((lo != hi).mean()), gts=per_gt)


def torch_maps(name):
    """oracle.targets.proposal_maps (torch's antialiased float64 interpolate of the zero-padded square), before the bf16 rounding"""
    c = CASE[name]
    segs = (selected(name) != 0).astype(np.float64)
    side = max(c["H"], c["W"])
    sq = np.pad(segs, ((0, 0), (0, side - c["H"]), (0, side - c["W"])))
    return ot.proposal_maps(np.ascontiguousarray(sq.transpose(1, 2, 0)), out=c["out"], dtype=torch.float64).numpy()


def torch_pin_terms(taps):
    """float64 rounding bound of torch's two passes against the exact value, in units of 2^-53 v: `taps` products and additions per pass (2 taps + 2, as
    for the kernel) plus the weights, which torch normalises with its own sequence of operations (w / total or w * (1 / total): <= 2 roundings on each of
    the two weights of a term, + 4)."""
    return 2 * taps + 6


# ------------------------------------------------------- emulation of the fused kernel -------------------------------------------------------
FUSED_MUTANTS = {
    "boundary_row_counted_twice": "out48_k2", "boundary_row_counted_never": "out100_k1", "tail_dropped": "gap5_tail", "ring16_always": "side208_27taps",
    "tap_beyond_w_weighs": "pad_right_64x8", "rows_beyond_h_read": "pad_below_8x64", "partial_chunk_dropped": "w40_scalar_staging",
    "fold_without_high_nibble": "bytes_odd", "fold_lowest_bit_only": "bytes_odd", "gt_area_by_every_k": "gt4", "order_ignored": "order_perm",
}


def _nzmask(w, mut):
    w = w.astype(np.uint32)
    if mut == "fold_lowest_bit_only":
        return w & np.uint32(0x01010101)
    if mut != "fold_without_high_nibble":
        w = w | (w >> np.uint32(4))
    w = w & np.uint32(0x0f0f0f0f)
    w = (w | (w >> np.uint32(2))) & np.uint32(0x03030303)
    return (w | (w >> np.uint32(1))) & np.uint32(0x01010101)


def _popc(w):
    return int(w.view(np.uint8).sum())                               # every byte is 0 or 1 after the fold


def emulate_fused(masks, order, gtp, H, W, OS, tabs, misaligned=False, mut=None):
    """numpy restatement of proposal_targets_kernel's STRUCTURE: grid (proposal, slice of output rows); per workgroup the ownership range
    [cnt_a, cnt_b), rows staged four at a time as 16-byte chunks (vector or scalar), byte fold + popcount of the owned rows, row sums into a ring indexed
    modulo RING (register window of 12 bytes from min(xs, 2047), or the scalar-weight loop), the vertical sum, the counts-only tail.  LDS starts as junk:
    `rows` full of LDS_JUNK, the ring full of NaN -- the result may not depend on a byte or a ring row that was never written.
    -> (float64 [K, OS, OS] before the rounding, counts int64 [n_gt, K, 2], gt_area int64 [n_gt])"""
    y0, ny, wgt, taps = tabs
    x0, nx = y0, ny
    n_gt = 0 if gtp is None else len(gtp)
    K = len(masks) if order is None else len(order)
    ns = n_slices(K, OS)
    RING = 16 if mut == "ring16_always" else ring_of(taps)
    flat = np.concatenate([np.ascontiguousarray(masks).reshape(-1), np.zeros((max(H, W) + taps + 2 * TG_ROWS) * W + 16, np.uint8)])      # what a read beyond the last mask finds
    out = np.zeros((K, OS, OS), np.float64)
    cnt, gcnt = np.zeros((max(n_gt, 1), K, 2), np.int64), np.zeros(max(n_gt, 1), np.int64)
    vec_ok = W % 16 == 0 and not misaligned
    wch = (W + 15) >> 4
    wch_staged = W >> 4 if (mut == "partial_chunk_dropped" and not vec_ok) else wch
    in_regs = taps <= TG_WREG
    xs, xn = x0.astype(np.int64), nx.astype(np.int64)
    cols = np.arange(OS)
    beyond_ok = mut == "tap_beyond_w_weighs"
    wreg = np.zeros((OS, TG_WREG))
    if in_regs:
        for i in range(min(TG_WREG, taps)):
            on = (i < xn) & ((xs + i < W) | beyond_ok)
            wreg[:, i] = np.where(on, wgt[:, i], 0.0)
    xstart = np.minimum(xs, TG_MAXW - 1)                                # xw + sh: the window's first byte
    for k in range(K):
        src = k if (order is None or mut == "order_ignored") else int(order[k])
        moff = src * H * W
        for s in range(ns):
            oy_a, oy_b = s * OS // ns, (s + 1) * OS // ns
            cnt_a = 0 if s == 0 else int(y0[oy_a])
            cnt_b = H if s == ns - 1 else min(H, int(y0[oy_b]))
            if mut == "boundary_row_counted_twice" and s != ns - 1:
                cnt_b = min(H, cnt_b + 1)
            if mut == "boundary_row_counted_never" and s != 0:
                cnt_a += 1
            rows = np.full((TG_ROWS, TG_MAXW + 16), LDS_JUNK, np.uint8)
            ring = np.full((RING, OS), np.nan)
            c_s, c_i, c_g = 0, [0] * 4, [0] * 4

            def stage(ya, nrows):
                nonlocal c_s
                for r in range(nrows):
                    y = ya + r
                    line = flat[moff + y * W: moff + y * W + W]
                    buf = np.zeros(wch * 16, np.uint8)
                    buf[:W] = line
                    rows[r, :wch_staged * 16] = buf[:wch_staged * 16]
                    if y < cnt_a or y >= cnt_b:
                        continue
                    n = _nzmask(buf[:wch_staged * 16].view("<u4"), mut)
                    c_s += _popc(n)
                    for g in range(n_gt):
                        q = np.zeros(wch * 16, np.uint8)
                        q[:W] = gtp[g][y]
                        qn = _nzmask(q[:wch_staged * 16].view("<u4"), mut)
                        c_i[g] += _popc(n & qn)
                        if k == 0 or mut == "gt_area_by_every_k":
                            c_g[g] += _popc(qn)

            def rowsums(ya, nrows):
                for r in range(nrows):
                    acc = np.zeros(OS)
                    if in_regs:
                        for i in range(TG_WREG):
                            acc = acc + np.where(rows[r, xstart + i] != 0, wreg[:, i], 0.0)
                    else:
                        for i in range(taps):
                            x = xs + i
                            on = (i < xn) & ((x < W) | beyond_ok)
                            acc = acc + np.where(on & (rows[r, np.minimum(x, TG_MAXW + 15)] != 0), wgt[:, i], 0.0)
                    ring[(ya + r) & (RING - 1)] = acc

            read_beyond = mut == "rows_beyond_h_read"
            next_y = 0 if s == 0 else int(y0[oy_a])
            for oy in range(oy_a, oy_b):
                ya = int(y0[oy])
                need = ya + int(ny[oy]) if read_beyond else min(H, ya + int(ny[oy]))
                while next_y < need:
                    nrows = TG_ROWS if read_beyond else min(TG_ROWS, H - next_y)
                    stage(next_y, nrows)
                    rowsums(next_y, nrows)
                    next_y += nrows
                acc = np.zeros(OS)
                for j in range(int(ny[oy])):
                    y = ya + j
                    if y >= H and not read_beyond:
                        break
                    acc = acc + wgt[oy, j] * ring[y & (RING - 1)]
                out[k, oy] = acc
            if mut != "tail_dropped":
                while next_y < cnt_b:
                    nrows = min(TG_ROWS, cnt_b - next_y)
                    stage(next_y, nrows)
                    next_y += nrows
            for g in range(n_gt):
                cnt[g, k, 0] += c_i[g]
                cnt[g, k, 1] += c_s
                if k == 0 or mut == "gt_area_by_every_k":
                    gcnt[g] += c_g[g]
    return out, cnt[:n_gt], gcnt[:n_gt]


def emulate_resize_aa(segs, out_size, tabs):
    """resize_aa_kernel: per pixel, the row sums in tap order (x < W && set), the vertical sum stopping at y >= H; float64"""
    y0, ny, w, taps = tabs
    K, H, W = segs.shape
    pad = np.zeros((K, H + taps + 1, W + taps + 1), bool)
    pad[:, :H, :W] = segs != 0
    acc = np.zeros((K, out_size, out_size))
    yy, xx = y0.astype(np.int64), y0.astype(np.int64)
    for j in range(taps):
        row = np.zeros((K, out_size, out_size))
        ys = np.minimum(yy + j, H + taps)
        for i in range(taps):
            xs_ = np.minimum(xx + i, W + taps)
            on = (i < ny)[None, None, :] & pad[:, ys][:, :, xs_]
            row = row + np.where(on, w[:, i][None, None, :], 0.0)
        live = ((j < ny) & (yy + j < H))[None, :, None]
        acc = acc + np.where(live, w[:, j][None, :, None] * row, 0.0)
    return acc


def emulate_nearest_index(out_n, in_n, mut=None):
    zoom = np.float64(in_n) / np.float64(out_n)
    cc = (np.arange(out_n, dtype=np.float64) + 0.5) * zoom - 0.5
    return np.clip(np.floor(cc if mut == "nearest_floor_c" else cc + 0.5), 0, in_n - 1).astype(np.int32)


def emulate_gt_resample(gt, H, W, mut=None):
    gy, gx = emulate_nearest_index(H, gt.shape[0], mut), emulate_nearest_index(W, gt.shape[1], mut)
    return (gt[gy][:, gx] != 0).astype(np.uint8)


def emulate_mask_targets(segs, gtp):
    s, g = segs != 0, gtp != 0
    return np.stack([(s & g[None]).reshape(len(s), -1).sum(1), s.reshape(len(s), -1).sum(1)], 1).astype(np.int64), int(g.sum())


def emulate_route(name, mut=None):
    """what `proposals_and_targets_dense` computes for the case: the fused pass for <= 4 ground truths + mask_targets for the rest, or the three
    kernels where the fused entry point refuses.  -> (bf16 bits [K, out, out], counts [C, K, 2], gt areas [C], iou [C, K], iop [C, K])"""
    c = CASE[name]
    m, tabs, gts = masks_of(name), tables_of(c), gts_of(name)
    order = None if c["order"] is None else np.array(c["order"])
    gtp = [emulate_gt_resample(g, c["H"], c["W"], mut) for g in gts]
    if fused_takes(c):
        n = min(len(gtp), LIMITS["n_gt"])
        val, cnt, area = emulate_fused(m, order, gtp[:n] if n else None, c["H"], c["W"], c["out"], tabs, misaligned=bool(c["misalign"]), mut=mut)
        cnt, area = list(cnt), list(area)
        rest = gtp[n:]
    else:
        val, cnt, area, rest = emulate_resize_aa(selected(name), c["out"], tabs), [], [], gtp
    for g in rest:
        cc, a = emulate_mask_targets(selected(name), g)
        cnt.append(cc); area.append(a)
    C_ = len(gtp)
    cnt = np.stack(cnt) if C_ else np.zeros((0, c["K"], 2), np.int64)
    area = np.array(area, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        I, S = cnt[:, :, 0].astype(np.float64), cnt[:, :, 1].astype(np.float64)
        G = area.astype(np.float64)[:, None]
        iou, iop = I / (S + G - I), I / S
    return to_bf16_bits(val), cnt, area, iou, iop


def route_differs(name, got):
    """-> list of what differs between a route's result (bits, counts, areas, iou, iop) and the reference of the case (empty: equal)"""
    ref = reference(name)
    bits, cnt, area, iou, iop = got
    bad = []
    n_bad = maps_agree(bits, ref["lo"], ref["hi"])
    if n_bad:
        bad.append(f"{n_bad} map pixels")
    for g, (gtp, rc, ra, riou, riop) in enumerate(ref["gts"]):
        if not np.array_equal(cnt[g], rc):
            bad.append(f"counts of ground truth {g}")
        if int(area[g]) != ra:
            bad.append(f"area of ground truth {g}: {int(area[g])} != {ra}")
        if not (np.array_equal(iou[g], riou, equal_nan=True) and np.array_equal(iop[g], riop, equal_nan=True)):
            bad.append(f"iou / iop of ground truth {g}")
    return bad


ROUTE_MUTANTS = dict(FUSED_MUTANTS, nearest_floor_c="gt4")


# ----------------------------------------------------------- standalone kernels -----------------------------------------------------------
RESIZE_CASES = {"out300_side20": (2, 20, 17, 300), "out16_side209": (2, 209, 100, 16)}      # K, H, W, out: a second column block; beyond the fused limit
MASK_TARGET_CASES = {"hw1": (1, 1, 1, 3, 2), "hw4096": (70, 64, 64, 32, 100), "hw4097": (3, 241, 17, 300, 9), "k1": (1, 37, 53, 37, 53)}      # K, H, W, Hg, Wg
GT_RESAMPLE_CASES = {"1x1_to_5x7": (5, 7, 1, 1), "up": (37, 53, 12, 20), "down": (12, 20, 37, 53), "same": (24, 40, 24, 40), "mixed": (64, 9, 9, 64)}      # H, W, Hg, Wg


def standalone_masks(tag, K, H, W):
    rng = _rng(tag)
    m = (rng.random((K, H, W)) > 0.5) * np.array([1, 255, 2, 0x80], np.uint8)[rng.integers(0, 4, (K, H, W))]
    if K >= 3:
        m[1] = 0
    return m.astype(np.uint8)


def standalone_gt(tag, Hg, Wg):
    return np.array([0, 1, 2, 255], np.uint8)[_rng(tag, 2).integers(0, 4, (Hg, Wg))]


# ---- rle_decode
def _runs_of(mask):
    return [int(v) for v in ht.rle_counts({"size": list(mask.shape), "counts": ot.rle_encode(mask)["counts"]})]


@functools.lru_cache(maxsize=None)
def rle_cases():
    """name -> (H, W, [run lengths per mask]).  Run lists, not strings: the string codec has its own suite."""
    rng = _rng("rle")
    res = {}
    m = (rng.random((37, 53)) > 0.6).astype(np.uint8)
    sparse = (rng.random((37, 53)) > 0.98).astype(np.uint8)
    res["37x53_mixed_run_counts"] = (37, 53, [_runs_of(m), [37 * 53], [0, 37 * 53], _runs_of(sparse), [5, 1, 37 * 53 - 6]])
    res["1x1"] = (1, 1, [[1], [0, 1]])
    res["k1_1x9"] = (1, 9, [[2, 3, 4]])
    res["k1_9x1"] = (9, 1, [[0, 4, 5]])
    # runs that end before H W (malformed): pycocotools, and the oracle, leave the rest zero -- after an even AND after an odd number of runs
    res["short_even_runs"] = (6, 7, [[3, 4], [0, 5, 2, 9]])
    res["short_odd_runs"] = (6, 7, [[3, 4, 5], [10]])
    return res


def rle_reference(name, hwk):
    H, W, runs = rle_cases()[name]
    out = np.stack([ot.rle_decode({"size": [H, W], "counts": r}) for r in runs], -1 if hwk else 0)
    return np.ascontiguousarray(out)


def rle_inputs(name):
    _, _, runs = rle_cases()[name]
    ends = np.concatenate([np.cumsum(r, dtype=np.uint64).astype(np.uint32) for r in runs])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
    return ends, offs


def emulate_rle_decode(name, hwk, mut=None, fixed=True):
    """rle_decode_kernel: per output byte the first run whose end exceeds p = x H + y; its index's parity.  Beyond the last run: zero (`fixed`), or the
    parity of the run count, what the kernel did before this suite."""
    H, W, runs = rle_cases()[name]
    ends, offs = rle_inputs(name)
    K = len(runs)
    y, x = np.mgrid[0:H, 0:W]
    p = (y * W + x if mut == "row_major_walk" else x * H + y).astype(np.uint32)
    planes = []
    for k in range(K):
        e = ends[offs[k]:offs[k + 1]]
        idx = np.searchsorted(e, p, side="right")
        v = (idx & 1).astype(np.uint8)
        if fixed:
            v[idx == len(e)] = 0
        planes.append(v)
    lay = hwk if mut != "hwk_swapped" else not hwk                     # the mutant fills the caller's buffer in the other layout's order
    return np.ascontiguousarray(np.stack(planes, -1 if lay else 0)).reshape((H, W, K) if hwk else (K, H, W))


RLE_MUTANTS = {"row_major_walk": "37x53_mixed_run_counts", "hwk_swapped": "37x53_mixed_run_counts", "parity_beyond_the_last_run": "short_odd_runs"}

# ---- intersection_union
IU_GRID_CAP = 2048 * 4096                                            # 2048 workgroups x 256 threads x 16 elements: above it the stride loop runs twice
IU_CASES = {"n1": (1, 255), "n255": (255, 255), "n4097": (4097, 255), "n4097_ignore7": (4097, 7), "above_grid_cap": (IU_GRID_CAP + 4097, 255)}


def iu_inputs(name):
    n, _ = IU_CASES[name]
    rng = _rng("iu" + name)
    vals = np.array([0, 1, 2, 255, 7], np.uint8)
    return vals[rng.integers(0, 5, n)], vals[rng.integers(0, 5, n)]


def iu_reference(pred, tgt, ignore):
    i, u, t = olosses.intersection_and_union(torch.from_numpy(pred.astype(np.int64)), torch.from_numpy(tgt.astype(np.int64)), 2, ignore)
    return torch.cat([i, u, t]).double().numpy().astype(np.int64)


def emulate_iu(pred, tgt, ignore, mut=None):
    """inter_union_kernel's rule: drop target == ignore; P_c / T_c count values < 2; I_c where pred == target; U = P + T - I"""
    ig = 255 if mut == "ignore_fixed_255" else ignore
    live = tgt != ig
    in_p = np.ones(len(tgt), bool) if mut == "ignored_counted_into_union" else live
    p, t = pred.astype(np.int64), tgt.astype(np.int64)
    I = np.array([(live & (p == c) & (t == c)).sum() for c in (0, 1)])
    P = np.array([(in_p & (p == c)).sum() for c in (0, 1)])
    T = np.array([(live & (t == c)).sum() for c in (0, 1)])
    return np.concatenate([I, P + T - I, T]).astype(np.int64)


IU_MUTANTS = {"ignore_fixed_255": "n4097_ignore7", "ignored_counted_into_union": "n4097"}

# ---- union_resize_iou: name -> (H, W, K, Hg, Wg, out_h, out_w (None: the ground truth's size), ignore, select kind)
URI_CASES = {
    "k1_3to7": (3, 3, 1, 7, 7, 7, 7, 255, "bytes"),
    "k3_7to3": (7, 7, 3, 3, 3, 3, 3, 255, "bytes"),
    "k300_select_bytes": (20, 24, 300, 16, 18, 40, 33, 255, "bytes"),
    "300to427": (300, 300, 3, 427, 427, 427, 427, 255, "bytes"),
    "1024to683": (1024, 8, 3, 683, 8, 683, 5, 255, "bytes"),
    "up_y_down_x_ignore7": (12, 40, 5, 30, 17, 29, 23, 7, "bytes"),
    "fp32_index_14x21_to_46x69": (14, 21, 3, 23, 18, 46, 69, 255, "bytes"),      # floor(dst * fp32(in / out)) differs from the float64 product at 1 row, 2 columns
    "argmax_form": (37, 53, 9, 74, 106, None, None, 255, "one_hot"),
    "nothing_selected": (16, 16, 4, 16, 16, 32, 32, 255, "none"),
}


def uri_inputs(name):
    H, W, K, Hg, Wg, oh, ow, ignore, kind = URI_CASES[name]
    rng = _rng("uri" + name)
    segs = np.where(rng.random((H, W, K)) > (0.6 if K < 50 else 0.99), np.array([1, 2, 255, 0x80], np.uint8)[rng.integers(0, 4, (H, W, K))], 0).astype(np.uint8)
    gt = np.array([0, 1, 1, 0, 2, 255, 7], np.uint8)[rng.integers(0, 7, (Hg, Wg))]
    if kind == "bytes":
        sel = np.array([0, 1, 2, 255, 0, 0], np.uint8)[rng.integers(0, 6, K)]
        sel[0] = 2                                                     # an EVEN non-zero byte selects (the header: select[k] != 0)
        if K >= 3:
            sel[1], sel[2] = 0, 255
        if K >= 300:
            sel[:] = 0
            sel[[0, 255, 256, 299]] = (2, 1, 2, 255)                   # beyond the 256 threads that stage `select`
    elif kind == "one_hot":
        sel = np.zeros(K, np.uint8)
        sel[int(rng.integers(0, K))] = 1
    else:
        sel = np.zeros(K, np.uint8)
    return segs, sel, gt, (Hg if oh is None else oh, Wg if ow is None else ow), ignore


def uri_reference(segs, sel, gt, out_hw, ignore):
    """torch on the CPU: union of the proposals with select != 0, F.interpolate(mode='nearest') of it and of the ground truth, 2-class I/U"""
    import torch.nn.functional as F
    pred = torch.from_numpy(((segs != 0) & (sel != 0)[None, None, :]).any(-1).astype(np.float32))[None, None]
    g = torch.from_numpy(gt.astype(np.float32))[None, None]
    if tuple(pred.shape[-2:]) != tuple(out_hw):
        pred = F.interpolate(pred, size=tuple(out_hw), mode="nearest")
    if tuple(g.shape[-2:]) != tuple(out_hw):
        g = F.interpolate(g, size=tuple(out_hw), mode="nearest")
    i, u, t = olosses.intersection_and_union(pred[0, 0].long(), g[0, 0].long(), 2, ignore)
    return torch.cat([i, u, t]).double().numpy().astype(np.int64)


def _src_index(n_out, n_in, f64=False):
    if f64:
        return np.minimum(np.floor(np.arange(n_out, dtype=np.float64) * (np.float64(n_in) / np.float64(n_out))).astype(np.int64), n_in - 1)
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def emulate_uri(segs, sel, gt, out_hw, ignore, mut=None):
    """union_resize_iou_kernel: fp32 source indices, p = any(select != 0 and seg != 0), the ground truth's byte as the class"""
    H, W, K = segs.shape
    f64 = mut == "f64_source_index"
    sy, sx = _src_index(out_hw[0], H, f64), _src_index(out_hw[1], W, f64)
    gy, gx = _src_index(out_hw[0], gt.shape[0], f64), _src_index(out_hw[1], gt.shape[1], f64)
    s = (sel & 1) if mut == "select_and_1" else (sel != 0)
    p = ((segs != 0) & (s != 0)[None, None, :]).any(-1)[sy][:, sx].astype(np.uint8).reshape(-1)
    t = gt[gy][:, gx].reshape(-1)
    return emulate_iu(p, t, ignore, mut if mut in IU_MUTANTS else None)


URI_MUTANTS = {"select_and_1": "k1_3to7", "f64_source_index": "fp32_index_14x21_to_46x69", "ignored_counted_into_union": "k3_7to3", "ignore_fixed_255": "up_y_down_x_ignore7"}
