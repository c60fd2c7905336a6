"""The seven device steps of SAM "everything" mode -- sam_postprocess / sam_mask_stats / sam_binarize / nms (csrc/head.hip) and mask_small_regions /
mask_boxes / sam_preprocess (csrc/image.hip): case tables, high-precision references, fp32 emulations and mutants.  No GPU code here:
tests/test_amg_kernels_cpu.py proves on the CPU that the references, emulations and bounds can fail, tests/test_amg_kernels_gpu.py holds the kernels to
the same tables.  What was measured is in profiles/amg_parity.md."""
import functools

import numpy as np
import torch

from oracle import amg as oamg

F32, F64 = np.float32, np.float64

# ============================================================ 1. post-processing ============================================================
# (img_size, input_size, original_size), why
GEOMETRIES = [
    (1024, (683, 1024), (427, 640), "the pipeline test's geometry"),
    (1024, (1024, 1024), (1024, 1024), "identity second stage"),
    (1024, (1024, 768), (1365, 1024), "portrait, up-scaling, ow = 4 x 256"),
    (1024, (512, 1024), (7, 13), "tiny: one partial workgroup both ways"),
    (1024, (1024, 1020), (257, 256), "ow one workgroup, oh = 4 x 64 + 1"),
    (1024, (1020, 1024), (64, 257), "oh = POST_ROWS, one column in the second x-block"),
    (1024, (1024, 4), (300, 1), "one output column"),
    (1024, (2, 1024), (1, 513), "one output row"),
    (512, (512, 384), (200, 150), "another img_size"),
]
THRESHOLDS = [(0.0, 1.0), (0.25, 0.5)]                  # (mask threshold, stability offset)
N_LOGITS = 4
FIELDS = ("smooth", "frame", "all-5", "all+5")
STATS_INIT = [0, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
N_BAND_MAX = 4
SEEDS = [100, 614, 1096, 103, 104, 105, 106, 107, 108]    # of the smooth field, per geometry: chosen so that N_BAND_MAX holds (a condition on the reference alone)
SEL = [2, 0, 3, 1, 2]                                   # binarize: a permutation of the candidates with one repeated

# The bound on |kernel - fp64 reference| per element is POST_C * 2^-24 * max|low|.  Roundings (unit roundoff u = 2^-24) along the longest path of ONE
# bilinear stage, value = w_y0 (w_x0 v00 + w_x1 v01) + w_y1 (w_x0 v10 + w_x1 v11):
#   1  w_x0 = 1 - frac_x (frac itself, src - floor(src), is exact; the fp64 reference uses 1 - frac unrounded)
#   1  w_x0 * v00
#   1  the inner sum
#   1  w_y0 = 1 - frac_y
#   1  w_y0 * (inner)
#   1  the outer sum
# = 6, each relative to a quantity of magnitude <= max|v| because the weights are non-negative and sum to 1 (a convex combination: it also carries
# an error of its inputs through without growing it).  Two stages: 6 u max|low| from the first, passed through the second, plus the second's own 6.
POST_C = 12
EMU_MAX, MUT_MIN = 0.5, 2.0                             # the convention of tests/gemm_checks.py


def post_bound(low):
    return POST_C * 2.0 ** -24 * float(np.abs(low).max())


def geometry_id(g):
    return f"img{g[0]}-{g[1][0]}x{g[1][1]}-to-{g[2][0]}x{g[2][1]}"


def to_nested(raster):
    """[n, 65536] raster -> the mask decoder's nested row order (the permutation of tests/sam_decoder_checks.py)"""
    n = raster.shape[0]
    return np.ascontiguousarray(raster.reshape(n, 64, 2, 2, 64, 2, 2).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, 65536))


@functools.lru_cache(maxsize=None)
def logits(gi):
    """fp32 [4, 65536] raster: smooth +-12 field, a one-pixel positive frame (corner pixel exactly 1 = threshold 0 + offset 1), all -5, all +5"""
    rng = np.random.default_rng(SEEDS[gi])
    coarse = torch.as_tensor(rng.standard_normal((1, 1, 33, 33)))
    smooth = torch.nn.functional.interpolate(coarse, (256, 256), mode="bicubic", align_corners=True)[0, 0].numpy()
    smooth = smooth * (12.0 / np.abs(smooth).max())
    frame = np.full((256, 256), -5.9)                    # (not dyadic: no interpolated value lands on a threshold by construction)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = 6.3
    frame[0, 0] = 1.0                                    # a value exactly AT thr + off = 1: `>` and `>=` differ here, and only here
    out = np.stack([smooth, frame, np.full((256, 256), -5.0), np.full((256, 256), 5.0)]).astype(F32).reshape(N_LOGITS, 65536)
    out.setflags(write=False)
    return out


def bil_coords(n_out, n_in, size_in, size_out, clamp_src=True, clamp_i1=True):
    """torch's upsample_bilinear2d source coordinates for fp32 input, align_corners=False: scale = fp32(size_in) / fp32(size_out),
    src = max(0, scale * (o + 0.5) - 0.5) in fp32.  torch's kernels (its vectorised CPU build and the GPU one alike) compile the product and the
    subtraction into ONE fused multiply-add, i.e. one rounding: that is what test_amg_kernels_cpu.py reads back from F.interpolate, weight by weight,
    and what is written here (the product of a 24-bit and a 12-bit number and the subtraction are exact in float64; one rounding to fp32 follows).
    -> i0, i1 int, w0, w1 fp32 (w1 = src - i0 exact, w0 = 1 - w1 rounded)"""
    scale = F32(size_in) / F32(size_out)
    o = np.arange(n_out, dtype=F64)
    src = (F64(scale) * (o + 0.5) - 0.5).astype(F32)
    if clamp_src:
        src = np.maximum(F32(0), src)
    assert src.dtype == F32
    i0 = src.astype(np.int32)                           # truncation, as the C cast
    i1 = i0 + ((i0 < n_in - 1) if clamp_i1 else 1)
    w1 = src - i0.astype(F32)
    w0 = F32(1) - w1
    return i0, i1.astype(np.int32), w0, w1


def torch_weights(n_in, n_out):
    """what F.interpolate itself uses along one axis, read back exactly: on an input that alternates 0, 1 the output is w1 (i0 even) or w0 (i0 odd),
    with no rounding of its own.  -> (torch's output fp32 [n_out], the same from bil_coords)"""
    v = (np.arange(n_in) % 2).astype(F32)
    x = torch.from_numpy(v.copy()).view(1, 1, n_in, 1).repeat(1, 1, 1, 2).contiguous()
    got = torch.nn.functional.interpolate(x, (n_out, 2), mode="bilinear", align_corners=False)[0, 0, :, 0].numpy()
    i0, i1, w0, w1 = bil_coords(n_out, n_in, n_in, n_out)
    return got, w0 * v[i0] + w1 * v[i1]


def _interp_matrix(n_out, n_in, size_in, size_out):
    i0, i1, _, w1 = bil_coords(n_out, n_in, size_in, size_out)
    m = np.zeros((n_out, n_in), F64)
    r = np.arange(n_out)
    np.add.at(m, (r, i0), 1.0 - w1.astype(F64))
    np.add.at(m, (r, i1), w1.astype(F64))
    return m


def post_reference(low_raster, geom):
    """fp64 [n, oh, ow]: `Sam.postprocess_masks` = bilinear 256 -> img, crop to input_size, bilinear -> original_size, with torch's fp32 coordinates and
    the interpolation in float64 (both stages are linear and separable: rows and columns as matrices, composed in float64)."""
    img, (ih, iw), (oh, ow) = geom[:3]
    ay = _interp_matrix(oh, ih, ih, oh) @ _interp_matrix(img, 256, 256, img)[:ih]
    ax = _interp_matrix(ow, iw, iw, ow) @ _interp_matrix(img, 256, 256, img)[:iw]
    low = low_raster.astype(F64).reshape(-1, 256, 256)
    return np.einsum("ya,nab,xb->nyx", ay, low, ax, optimize=True)


@functools.lru_cache(maxsize=None)
def reference(gi):
    ref = post_reference(logits(gi), GEOMETRIES[gi])
    ref.setflags(write=False)
    return ref


def _low_addr(Y, X, nested, swap=False):
    """flat index of low-resolution pixel (Y, X): raster, or the nested order ((y 64 + x) 4 + dy1 2 + dx1) 4 + dy2 2 + dx2"""
    if not nested:
        return Y * 256 + X
    tok = (Y >> 2) * 64 + (X >> 2)
    dy1, dx1, dy2, dx2 = (Y >> 1) & 1, (X >> 1) & 1, Y & 1, X & 1
    if swap:
        dy1, dx1, dy2, dx2 = dx1, dy1, dx2, dy2
    return (tok * 4 + dy1 * 2 + dx1) * 4 + dy2 * 2 + dx2


def _bilinear_f32(v00, v01, v10, v11, wy0, wy1, wx0, wx1):
    """w_y0 (w_x0 v00 + w_x1 v01) + w_y1 (w_x0 v10 + w_x1 v11), one fp32 rounding per operation, no fused multiply-add"""
    top = wx0 * v00 + wx1 * v01
    bot = wx0 * v10 + wx1 * v11
    out = wy0 * top + wy1 * bot
    assert out.dtype == F32
    return out


def post_emulation(low, geom, nested=False, mutant=None):
    """fp32 [n, oh, ow]: the kernel's arithmetic in numpy float32 (its per-pixel evaluation of the four stage-1 samples performs the same operations as
    evaluating the img x img intermediate once).  `low` is [n, 65536] in the layout `nested` says.  Out-of-range reads of a mutant see 0."""
    img, (ih, iw), (oh, ow) = geom[:3]
    cs, ci = mutant != "src_not_clamped", mutant != "i1_not_clamped"
    s_in, s_out = (img, 256) if mutant == "scale1_inverted" else (256, img)
    n = low.shape[0]
    lowp = np.concatenate([low.astype(F32), np.zeros((n, 1), F32)], 1)          # index 65536 = "out of range"
    a0, a1, u0, u1 = bil_coords(img, 256, s_in, s_out, cs, ci)

    def fetch(Y, X):
        ok = (Y[:, None] < 256) & (X[None, :] < 256)
        addr = _low_addr(np.minimum(Y, 255)[:, None], np.minimum(X, 255)[None, :], nested, mutant == "nested_bits_swapped")
        return lowp[:, np.where(ok, addr, 65536)]
    s1 = _bilinear_f32(fetch(a0, a0), fetch(a0, a1), fetch(a1, a0), fetch(a1, a1), u0[None, :, None], u1[None, :, None], u0[None, None, :], u1[None, None, :])
    if mutant == "crop_dropped":
        ih, iw = img, img
    s1p = np.zeros((n, img + 1, img + 1), F32)
    s1p[:, :img, :img] = s1
    y0, y1, wy0, wy1 = bil_coords(oh, ih, ih, oh, cs, ci)
    x0, x1, wx0, wx1 = bil_coords(ow, iw, iw, ow, cs, ci)
    y0, y1, x0, x1 = (np.minimum(t, img) for t in (y0, y1, x0, x1))

    def at(Y, X):
        return s1p[:, Y[:, None], X[None, :]]
    return _bilinear_f32(at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1), wy0[None, :, None], wy1[None, :, None], wx0[None, None, :], wx1[None, None, :])


def stats_of(P, thr, off, mutant=None):
    """[n, oh, ow] values -> int64 [n, 7] = |P > thr + off|, |P > thr - off|, |P > thr|, min x, min y, max x, max y of P > thr (STATS_INIT when empty).
    The thresholds are the kernel's: thr + off and thr - off in fp32."""
    P = np.asarray(P)
    gt = (lambda a, b: a >= b) if mutant == "ge_at_threshold" else (lambda a, b: a > b)
    t_hi, t_lo, t = F32(thr) + F32(off), F32(thr) - F32(off), F32(thr)
    out = np.empty((P.shape[0], 7), np.int64)
    for k in range(P.shape[0]):
        m = gt(P[k], t)
        row = [int(gt(P[k], t_hi).sum()), int(gt(P[k], t_lo).sum()), int(m.sum())]
        if m.any():
            ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
            box = [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])]
            if mutant == "box_max_exclusive":
                box = [box[0], box[1], box[2] + 1, box[3] + 1]
            if mutant == "box_xy_swapped":
                box = [box[1], box[0], box[3], box[2]]
        else:
            box = STATS_INIT[3:]
        out[k] = row + box
    return out


def band(ref, thr, off, bound):
    """per mask and threshold, the reference pixels within `bound` of it: -> (n_band int [n, 3], on_extreme bool [n]: a band pixel of the mask threshold
    lies on an extreme row or column of the reference box, where it may move the box; for an empty reference mask, any band pixel)"""
    n = ref.shape[0]
    nb = np.zeros((n, 3), np.int64)
    edge = np.zeros((n,), bool)
    st = stats_of(ref, thr, off)
    for j, t in enumerate((F32(thr) + F32(off), F32(thr) - F32(off), F32(thr))):
        nb[:, j] = (np.abs(ref - F64(t)) <= bound).reshape(n, -1).sum(1)
    for k in range(n):
        if nb[k, 2]:
            b = np.abs(ref[k] - F64(F32(thr))) <= bound
            x0, y0, x1, y1 = st[k, 3:]
            edge[k] = True if st[k, 2] == 0 else bool(b[[y0, y1], :].any() or b[:, [x0, x1]].any())
    return nb, edge


def stats_agree(got, ref, thr, off, bound):
    """the issue's comparison of a [n, 7] statistics table with the fp64 reference values: -> list of complaints (empty = agree)"""
    want = stats_of(ref, thr, off)
    nb, edge = band(ref, thr, off, bound)
    bad = []
    for k in range(ref.shape[0]):
        for j in range(3):
            if abs(int(got[k, j]) - int(want[k, j])) > nb[k, j]:
                bad.append(f"mask {k} count {j}: {int(got[k, j])} vs {int(want[k, j])}, {nb[k, j]} pixels in the band")
        if not edge[k] and [int(v) for v in got[k, 3:]] != [int(v) for v in want[k, 3:]]:
            bad.append(f"mask {k} box: {got[k, 3:].tolist()} vs {want[k, 3:].tolist()}")
    return bad


# mutant of the emulation -> (geometry index, nested) of a case that kills it
POST_MUTANTS = {
    "i1_not_clamped": (1, False),          # input 1024 x 1024 reaches stage-1 rows 1022 / 1023, whose second sample is row 256
    "src_not_clamped": (1, False),         # the frame: extrapolation across the first row
    "scale1_inverted": (0, False),
    "crop_dropped": (0, False),            # 683 of 1024 rows
    "nested_bits_swapped": (0, True),
    "ge_at_threshold": (1, False),         # identity second stage: the four output pixels that copy low[0, 0] = 1 exactly
    "box_max_exclusive": (3, False),
    "box_xy_swapped": (5, False),          # 64 x 257
}


@functools.lru_cache(maxsize=None)
def post_mutant_ratio(mutant, gi, nested):
    """-> (worst |mutant - reference| / bound, the statistics tables differ from the unmutated emulation's)"""
    low = logits(gi)
    g = GEOMETRIES[gi]
    lay = to_nested(low) if nested else low
    val_mut = mutant if mutant not in ("ge_at_threshold", "box_max_exclusive", "box_xy_swapped") else None
    st_mut = mutant if val_mut is None else None
    emu = post_emulation(lay, g, nested, val_mut)
    ratio = float(np.abs(emu.astype(F64) - reference(gi)).max() / post_bound(low))
    base = post_emulation(lay, g, nested)
    differ = any(not np.array_equal(stats_of(emu, t, o, st_mut), stats_of(base, t, o)) for t, o in THRESHOLDS)
    return ratio, differ


# ================================================================= 2. NMS =================================================================
def nms_reference(boxes, order, thr, mutant=None):
    """`oracle.amg.nms` on boxes[order] with the ranking given (numpy fp32; pinned against the oracle by the CPU test): -> bool [n] keep flags"""
    b = np.asarray(boxes, F32)[np.asarray(order, np.int64)]
    n = len(b)
    one = F32(1 if mutant == "plus_one_areas" else 0)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    dead = np.zeros(n, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            if dead[i] and mutant != "dead_box_suppresses":
                continue
            r = b[i + 1:]
            iw = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]) + one, F32(0))
            ih = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]) + one, F32(0))
            inter = iw * ih
            union = area[i] + area[i + 1:] - (F32(0) if mutant == "union_without_inter" else inter)
            iou = inter / union
            dead[i + 1:] |= (iou >= F32(thr)) if mutant == "ge_at_threshold" else (iou > F32(thr))
    return ~dead


def _rand_boxes(rng, n, lo, span, wmin, wmax):
    xy = rng.integers(lo, lo + span, (n, 2))
    wh = rng.integers(wmin, wmax, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(F32)


def _nms_cases():
    """name -> (boxes fp32 [m, 4] integer coordinates < 4096, order int32 [n], thr, scores or None)"""
    c = {}
    c["n1"] = (np.array([[3, 4, 10, 20]], F32), [0], 0.5, None)
    c["n2_identical_pair"] = (np.array([[3, 4, 10, 20]] * 2, F32), [0, 1], 0.5, None)
    for n in (1023, 1024, 1025, 1026):
        rng = np.random.default_rng(n)
        b = _rand_boxes(rng, n, 0, 300, 5, 200)
        order = rng.permutation(n)
        b[order[-1]] = b[order[0]]                      # the last in rank repeats the first: suppressed by a thread 1023 (or 1024 + 0) places away
        c[f"n{n}"] = (b, order, 0.7, None)
    rng = np.random.default_rng(3000)
    i = np.arange(3000)
    x = (i % 200) * 18 + rng.integers(0, 5, 3000)
    y = (i // 200) * 230
    c["n3000_dense_chains"] = (np.stack([x, y, x + 100, y + 100], 1).astype(F32), rng.permutation(3000), 0.5, None)
    rng = np.random.default_rng(8192)
    c["n8192_limit"] = (_rand_boxes(rng, 8192, 0, 600, 20, 200), rng.permutation(8192), 0.5, None)
    half, quarter = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], F32), np.array([[0, 0, 10, 10], [0, 0, 5, 5]], F32)
    c["iou_equals_thr_0.5"] = (half, [0, 1], 0.5, None)                                                  # IoU 50 / 100: strict test keeps both
    c["iou_equals_thr_0.25"] = (quarter, [0, 1], 0.25, None)
    c["iou_one_step_above_thr_0.5"] = (half, [0, 1], float(np.nextafter(F32(0.5), F32(0))), None)       # the IoU is the next fp32 above the threshold
    c["iou_one_step_above_thr_0.25"] = (quarter, [0, 1], float(np.nextafter(F32(0.25), F32(0))), None)
    z = np.array([[5, 5, 5, 30], [0, 0, 40, 40], [5, 5, 5, 30], [2, 2, 38, 41], [7, 0, 7, 0], [100, 100, 140, 150]], F32)
    c["zero_area_boxes"] = (z, [0, 1, 2, 3, 4, 5], 0.5, None)                                            # 0 / 0 = NaN: not suppressed
    c["two_identical_zero_area"] = (np.array([[9, 9, 9, 9]] * 2, F32), [0, 1], 0.5, None)
    rng = np.random.default_rng(77)
    b = _rand_boxes(rng, 400, 0, 200, 5, 120)
    c["order_is_a_subset"] = (b, rng.permutation(400)[:150], 0.3, None)
    b = _rand_boxes(rng, 300, 0, 200, 5, 120)
    b[100:120] = b[0:20]
    s = rng.random(300).astype(F32)
    s[200:230] = s[0]
    s[50:60] = s[1]
    c["equal_scores_stable_sort"] = (b, np.argsort(-s, kind="stable"), 0.3, s)
    # a chain: 0 suppresses 1, 1 would suppress 2, 0 does not reach 2
    c["chain_of_three"] = (np.array([[0, 0, 100, 100], [30, 0, 130, 100], [60, 0, 160, 100]], F32), [0, 1, 2], 0.5, None)
    return {k: (b, np.asarray(o, np.int32), t, s) for k, (b, o, t, s) in c.items()}


NMS_CASES = _nms_cases()
NMS_LIMIT = 8192
NMS_MUTANTS = {"ge_at_threshold": "iou_equals_thr_0.5", "dead_box_suppresses": "chain_of_three", "union_without_inter": "n2_identical_pair",
               "plus_one_areas": "zero_area_boxes"}


@functools.lru_cache(maxsize=None)
def nms_oracle(name):
    """kept candidates, in rank order, as `oracle.amg.nms` decides them (scores = minus the rank: `order` is the ranking)"""
    b, order, thr, _ = NMS_CASES[name]
    kept = oamg.nms(torch.as_tensor(b[order.astype(np.int64)]), -torch.arange(len(order), dtype=torch.float64), thr)
    return order[kept.numpy()]


# ====================================================== 3. small regions and boxes ======================================================
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 255), (64, 256), (64, 257), (97, 130), (40, 1030)]
MIN_AREAS = (0, 1, 4, 30, None)                          # None = H * W + 1
RUNS = (3, 4, 5, 29, 30, 31)                             # min_area - 1, min_area, min_area + 1 for min_area 4 and 30


def _p_empty(H, W, rng):
    return np.zeros((H, W), bool)


def _p_full(H, W, rng):
    return np.ones((H, W), bool)


def _p_checker(H, W, rng):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0


def _p_serpentine(H, W, rng):
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def _p_spiral(H, W, rng):
    """a one-pixel path that walks inwards, turning right whenever the cell two ahead is taken: one long component, and the zeros are one too"""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    moved = True
    while moved:
        moved = False
        for _ in range(2):                               # straight on, or one right turn
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                y, x, moved = ny, nx, True
                m[y, x] = True
                break
            dy, dx = dx, -dy
    return m


def _p_blobs(H, W, rng):
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    base = torch.rand((1, 1, H // 8 + 2, W // 8 + 2), generator=g)
    m = torch.nn.functional.interpolate(base, (H, W), mode="bilinear")[0, 0] > 0.5
    m ^= torch.rand((H, W), generator=g) > 0.97          # speckle: one-pixel holes and islands
    return m.numpy()


def _p_zigzag(H, W, rng):
    """diagonal-only contact across the 256-column boundary: (y, 255) and (y + 1, 256), alternating down the whole height"""
    m = np.zeros((H, W), bool)
    b = 256 if W > 256 else max(1, W // 2)
    for y in range(H):
        m[y, min(W - 1, b - 1 + (y & 1))] = True
    return m


def _lay_runs(m, value, y, x_lo, x_hi, runs):
    """write runs of `value` of the given lengths on every other row from y, columns [x_lo, x_hi), two columns apart: -> first row not used"""
    x = x_lo
    for n in runs:
        if x + n > x_hi:
            y, x = y + 2, x_lo
        m[y, x:x + n] = value
        x += n + 2
    return y + 2


def _p_exact(H, W, rng):
    """islands and holes of min_area - 1, min_area, min_area + 1 pixels, and a ring that only holes-before-islands keeps"""
    m = np.zeros((H, W), bool)
    if H == 1 or W == 1:                                 # a line: runs of ones and of zeros, the zero runs are holes of their own
        v, p = m.reshape(-1), 0
        for n in RUNS:
            v[p:p + n] = True
            p += 2 * n
        v[p:] = True                                     # (the gaps 3, 4, 5, 29, 30, 31 long lie between ones)
        return m
    y = _lay_runs(m, True, 1, 1, W - 1, RUNS)
    rows = 2 * (sum(RUNS) + 2 * len(RUNS)) // (W - 4) + 6
    m[y:y + rows + 2] = True
    y2 = _lay_runs(m, False, y + 1, 2, W - 2, RUNS)
    assert y2 <= y + rows + 1
    y = y + rows + 4
    m[y:y + 4, 3:15] = True                              # ring of 28 pixels around a hole of 20: 48 pixels once the hole is filled
    m[y + 1:y + 3, 4:14] = False
    assert y + 5 < H
    return m


def _islands(H, W, sizes):
    """small horizontal islands; the first pixel of island k + 1 comes later in raster order but further LEFT than that of island k"""
    m = np.zeros((H, W), bool)
    if H == 1 or W == 1:
        v, p = m.reshape(-1), 1
        for n in sizes:
            v[p:p + n] = True
            p += n + 2
        return m
    for k, n in enumerate(sizes):
        x = W - 5 - 7 * k - n
        m[2 + 3 * k, x:x + n] = True
    return m


def _p_small_strict(H, W, rng):
    return _islands(H, W, (1, 3, 2))


def _p_small_tie2(H, W, rng):
    return _islands(H, W, (3, 3, 1))


def _p_small_tie3(H, W, rng):
    return _islands(H, W, (2, 3, 3, 3))


PATTERNS = {"empty": _p_empty, "full": _p_full, "checkerboard": _p_checker, "serpentine": _p_serpentine, "spiral": _p_spiral, "blobs": _p_blobs,
            "zigzag": _p_zigzag, "exact_sizes": _p_exact, "small_strict_largest": _p_small_strict, "small_tie_of_two": _p_small_tie2,
            "small_tie_of_three": _p_small_tie3, "blobs_as_0_255": _p_blobs}


def _fits(name, H, W):
    if name == "exact_sizes":
        return (H == 1 or W == 1) and H * W >= 300 or (H >= 40 and W >= 40)
    if name.startswith("small_"):
        return H * W >= 300 and (H == 1 or W == 1 or (H >= 16 and W >= 40))
    return True


@functools.lru_cache(maxsize=None)
def region_masks(shape):
    """-> (names, uint8 [K, H, W]): every pattern that fits the shape; the last is stored as 0 / 255"""
    H, W = shape
    rng = np.random.default_rng(H * 10007 + W)
    names = [n for n in PATTERNS if _fits(n, H, W)]
    ms = np.stack([PATTERNS[n](H, W, rng) for n in names]).astype(np.uint8)
    ms[names.index("blobs_as_0_255")] *= 255
    ms.setflags(write=False)
    return names, ms


def min_area_of(a, shape):
    return shape[0] * shape[1] + 1 if a is None else a


_FULL8, _CROSS4 = np.ones((3, 3), np.int32), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.int32)


def remove_small_regions(mask, area_thresh, mode, mutant=None):
    """`oracle.amg.remove_small_regions` restated with switches for the mutants (pinned against the oracle itself by the CPU test)"""
    from scipy import ndimage
    holes = mode == "holes"
    working = (holes ^ mask).astype(np.uint8)
    regions, n = ndimage.label(working, structure=_CROSS4 if mutant == "connectivity_4" else _FULL8)
    sizes = np.bincount(regions.ravel(), minlength=n + 1)[1:]
    small = [i + 1 for i, sz in enumerate(sizes) if (sz <= area_thresh if mutant == "le_at_min_area" else sz < area_thresh)]
    if len(small) == 0:
        return mask, False
    fill = [0] + small
    if holes and mutant == "keep_largest_in_holes" and len(small) == n:
        fill.remove(int(np.argmax(sizes)) + 1)
    if not holes:
        fill = [i for i in range(n + 1) if i not in fill]
        if len(fill) == 0:
            fill = [n - int(np.argmax(sizes[::-1])) if mutant == "ties_keep_last" else int(np.argmax(sizes)) + 1]
    return np.isin(regions, fill), True


def clean_reference(mask, min_area, mutant=None):
    """holes then islands, as `postprocess_small_regions` applies them: -> (bool [H, W], changed)"""
    m = np.asarray(mask) != 0
    modes = ("islands", "holes") if mutant == "islands_before_holes" else ("holes", "islands")
    m, c1 = remove_small_regions(m, min_area, modes[0], mutant)
    m, c2 = remove_small_regions(m, min_area, modes[1], mutant)
    return m, bool(c1 or c2)


@functools.lru_cache(maxsize=None)
def region_reference(shape, min_area):
    """the ORACLE's answer for every mask of the shape: -> (bool [K, H, W], changed bool [K], boxes int64 [K, 4], areas int64 [K])"""
    _, ms = region_masks(shape)
    out, ch = [], []
    for m in ms:
        f, c1 = oamg.remove_small_regions(m != 0, min_area, "holes")
        f, c2 = oamg.remove_small_regions(f, min_area, "islands")
        out.append(f)
        ch.append(bool(c1 or c2))
    out = np.stack(out)
    return out, np.array(ch), oamg.masks_to_boxes(torch.as_tensor(out)).numpy().astype(np.int64), out.reshape(len(out), -1).sum(1)


# mutant of the reference -> (shape, pattern, min_area) of a case that kills it
REGION_MUTANTS = {
    "connectivity_4": ((64, 257), "zigzag", 4),
    "le_at_min_area": ((97, 130), "exact_sizes", 30),
    "ties_keep_last": ((64, 257), "small_tie_of_two", 4),
    "keep_largest_in_holes": ((1, 1), "empty", None),
    "islands_before_holes": ((97, 130), "exact_sizes", 30),
}


def flood_fill_labels(fg):
    """8-connected component sizes by a plain flood fill: -> (labels int [H, W] numbered by first pixel in raster order, from 1; sizes)"""
    H, W = fg.shape
    lab, sizes = np.zeros((H, W), np.int64), []
    for y0 in range(H):
        for x0 in range(W):
            if fg[y0, x0] and not lab[y0, x0]:
                sizes.append(0)
                lab[y0, x0], stack = len(sizes), [(y0, x0)]
                while stack:
                    y, x = stack.pop()
                    sizes[-1] += 1
                    for yy in range(max(0, y - 1), min(H, y + 2)):
                        for xx in range(max(0, x - 1), min(W, x + 2)):
                            if fg[yy, xx] and not lab[yy, xx]:
                                lab[yy, xx] = len(sizes)
                                stack.append((yy, xx))
    return lab, sizes


# ============================================================ 4. sam_preprocess ============================================================
PRE_SIZES = [((16, 48), 64), ((1, 1), 64), ((64, 63), 64), ((1024, 1023), 1024)]          # (h, w), img_size


def pre_image(h, w):
    """uint8 [h, w, 3]: walking the pixels in raster order every channel runs through all 256 values (from a different start)"""
    i = np.arange(h * w).reshape(h, w, 1)
    return ((i + np.array([0, 85, 170]).reshape(1, 1, 3)) % 256).astype(np.uint8)


def bf16_bits(x):
    """round-to-nearest-even of float64 values straight to bfloat16 (8 significant bits), ONE rounding: -> the int16 bit patterns"""
    x = np.asarray(x, F64)
    m, e = np.frexp(x)                                   # x = m 2^e, 0.5 <= |m| < 1
    r = np.ldexp(np.rint(m * 256.0), e - 8)              # m * 256 is exact, rint rounds half to even
    f = r.astype(F32)
    assert np.array_equal(f.astype(F64), r)
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def pre_table():
    """int16 [256, 3] bf16 bits of (v - mean) / std: -> (fp64 route, fp32 route)"""
    v = np.arange(256).reshape(256, 1)
    mean, std = np.array(oamg.PIXEL_MEAN), np.array(oamg.PIXEL_STD)
    r64 = (v.astype(F64) - mean) / std
    r32 = (v.astype(F32) - mean.astype(F32)) / std.astype(F32)
    assert r32.dtype == F32
    return bf16_bits(r64), bf16_bits(r32.astype(F64))


# (value, channel) pairs on which the fp32 route and the fp64 reference round to different bf16 values (double rounding), with both candidates: none
PRE_TIES = {}


def pre_reference(h, w, S):
    """int16 [3, S, S] bit patterns: the fp64 table looked up per pixel, +0.0 in the padding"""
    t64, _ = pre_table()
    img = pre_image(h, w)
    out = np.zeros((3, S, S), np.int16)
    for c in range(3):
        out[c, :h, :w] = t64[img[:, :, c], c]
    return out
