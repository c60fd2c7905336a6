"""Forward glue, decode and head kernels (llmseg_amd/csrc/pointwise.hip, decode_attn.hip, the pull-back, cosine and dice / BCE kernels of head.hip) on every dispatch route: a case
table, input builders, fp64 references, LOCAL tolerances, fp32 / bf16 emulations of what the kernels round, and mutants (fp64 results of subtly
wrong problems) that the tolerances must reject.

Everything here runs on the CPU (no import of the HIP library).  tests/test_forward_kernels_cpu.py proves that the tolerance passes the emulations
with a 2x margin and rejects every applicable mutant by at least 2x on every case; tests/test_forward_kernels_gpu.py holds the kernels to the same
rule.  Case, ratio, the two bound forms and their constants are those of tests/backward_kernel_checks.py.

Outputs are compared over the whole buffer the call is handed: the slack of a strided output, rows a row_map skips and rows in front of a row
offset hold NaN in the reference (a sentinel that must stay), the parts of an in-place buffer the op must not touch hold their input and take the
bound zero.  Tolerances, per element:
  bf16 outputs          |got - ref| <= C_BF16 * 2^-8 * (|ref| + sigma_row); zero where the reference is exactly zero or a pure copy
  RMS norm              the operation itself rounds x * rstd to bf16 before the weight multiply (HF LlamaRMSNorm).  Where the fp64 value of x * rstd lies
                        within 2^-21 |x * rstd| of a bf16 rounding boundary (fp32 resolution of a product with an approximated rsqrt: a few ulps of 2^-24)
                        either neighbour is a correct result, so |w| * ulp_bf16 is added to the bound of that element (about 1 element in 6000)
  GELU, x <= -3         + 0.5 |x| (1.5e-7 + 2^-24): the kernel's erf is Abramowitz-Stegun 7.1.26 with a stated absolute error of 1.5e-7, and 1 - p e^(-z^2)
                        is rounded to fp32 next to 1 (spacing 2^-24); 1 + erf(x / sqrt 2) is that small difference, so its error is absolute
  fp32 sums             f32_bound(n, sum |t_i|) with C_SUM (pull-back, wsum, dice, BCE)
  dlogits (dice / BCE)  the same form with n = 2 terms and C_DLOGITS
  cosine                f32_bound(D, sum_d |t_d e_d| / (|t| |e|)) with C_COS
  align / regression    losses and d_t: f32_bound with C_SUM; d_e and d_pred: the same form with C_DE, C_DPRED.  The terms of the KL loss, d_e and d_t include those of
                        the exponent cos_k / tau, itself a D-term sum that moves softmax_k by softmax_k * d(cos_k / tau) (align_kernel_formula: A and G)

Two bounds carry a term beyond the plain form, and the emulation alone needs each (worst emulation ratio over the table without / with it):
  RMS tie term          0.631 / 0.445, both at norm-2048x2048_rms.  1293 of the 6.7 M RMS elements of the table sit on such a boundary; there the fp32 product of
                        the emulation rounds to the other bf16 neighbour than the fp64 one, a full bf16 ulp of x * rstd times w
  pull-back coordinate  26.1 / 0.249, both at pullback-g16_S33_seam.  A tap weight is the fractional part of the fp32 coordinate (p + 0.5) * (g / S) - 0.5 <= g, so it is
  term                  known to g * 2^-23 absolutely; where S / g is no power of two a weight of 1e-2 carries that error relatively 1e-4, which no multiple of
                        2^-24 sum |t| covers.  The term is g * 2^-23 * sum_pixels m (wx + wy): the first-order effect of that coordinate error on m * wx * wy.
                        At S / g a power of two (64 / 256, 16 / 64, 8 / 64, 32 / 32) the coordinates are exact and the emulation meets the plain bound (0.02)
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses as olosses
from tests.backward_kernel_checks import C_BF16, C_SUM, EMU_MAX, MUT_MIN, Case, bf16_bound, cdiv, f32_bound, ratio      # noqa: F401  (re-exported)

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
NAN = float("nan")
JUNK = 7.0                      # what the slack of a strided INPUT holds (finite: a kernel that reads it is wrong, not NaN)
LOG2E = 1.4426950408889634
GRID_CAP = 8192 * 256           # threads of a capped streaming grid: one chunk each per sweep
C_DLOGITS = 43.0                # dice / BCE gradient, element-wise fp32 through __expf and reciprocals: smallest integer for which the emulation stays <= EMU_MAX
                                # (the worst, 0.49: dice-M3_HW4096 at a logit near -30, where sigmoid = 1 / e^30 alone makes the element: the fp32 product
                                # 30 * log2(e) = 43.3 is rounded to half an ulp of 2^-18, which leaves e^30 with a relative error of up to 22 * 2^-24)
PLAIN = False                   # True: the RMS tie term and the pull-back coordinate term are left off (the CPU test recomputes what the emulation then reaches)
C_DE = 3.0                      # align_reg_loss d_e, element-wise, n = D + 2 (the cosine's dot product, then two products): smallest integer for which the emulation stays
                                # <= EMU_MAX (the worst, 0.480: align-K256_D256_grads_items3)
C_DPRED = 4.0                   # align_reg_loss d_pred, element-wise, n = 2: likewise (the worst, 0.463: align-K37_D200_grads_items3; a difference, a fast exponential of
                                # g - 1, three products and a division on one element)
C_COS = 1.0                     # cosine scores: smallest integer for which the emulation stays <= EMU_MAX (the worst, 0.066: cosine-K5_D64)
ACTS = {"relu": 1, "gelu": 2, "quickgelu": 3, "silu": 4, "sigmoid": 5}      # LLMSEG_ACT_*


def _g(case):
    return torch.Generator().manual_seed(case.seed)


def _T(t, emu):
    return t.to(F32 if emu else F64)


def _rb(t, emu):
    """the bf16 store of the kernels (emulation only)"""
    return t.to(BF).to(F64) if emu else t.to(F64)


def _exp(x, emu):
    """exp; emulated as the fast exponential: an fp32 exp2 of the fp32 product x * log2(e)"""
    return torch.exp2(x * LOG2E) if emu else torch.exp(x)


def _sigmoid(x, emu):
    return 1.0 / (1.0 + _exp(-x, emu))             # the reciprocal as an fp32 division


def _pad(t, ld, rows=None):
    """t [r, c] inside a NaN buffer [rows or r, ld]"""
    out = torch.full((rows or t.shape[0], ld), NAN, dtype=F64)
    out[:t.shape[0], :t.shape[1]] = t
    return out


# ------------------------------------------------------------------------------------------------ the dispatch, restated (route, launches)
def norm_route(rows, cols):
    nch = cols // 8
    if 64 <= rows < 2048 and 2048 <= cols <= 8192:
        cpt = cdiv(nch, 256)
        return f"wg_cpt{1 if cpt <= 1 else 2 if cpt <= 2 else 4}"
    cpl = cdiv(nch, 64)
    return f"wave_cpl{1 if cpl <= 1 else 2 if cpl <= 2 else 3 if cpl <= 3 else 4 if cpl <= 4 else 8 if cpl <= 8 else 16 if cpl <= 16 else 0}"


def norm_padded_width(rows, cols):
    """the columns the registers of this route's kernel hold per row (zero beyond cols): 64 lanes x CPL chunks x 8, or 256 threads x CPT x 8; the generic
    wave kernel (CPL = 0) walks the row and pads nothing"""
    rt = norm_route(rows, cols)
    n = int(rt[-1] if rt[-2] in "lt" else rt[-2:])
    return cols if n == 0 else (256 if rt.startswith("wg") else 64) * n * 8


def pullback_route(g, S):
    """the s256 kernel, or the generic one with the tap weights of a column in registers / recomputed per row (phi - plo >= 16 on some column)"""
    if S == 256 and g == 64:
        return "s256"
    f = np.float32
    scale = f(g) / f(S)
    worst = 0
    for sx in range(g):
        plo = max(0, int(math.floor((f(sx) - f(0.5)) / scale - f(0.5))) - 1)
        phi = min(S - 1, int(math.ceil((f(sx) + f(1.5)) / scale - f(0.5))) + 1)
        worst = max(worst, phi - plo)
    return "generic_fallback" if worst >= 16 else "generic_regs"


def decode_splits(N, heads, scratch_floats):
    """key splits of decode_attn: up to 16 until the launch covers the chip, cut to what the scratch holds (130 floats per (n, head, split)); 1 without scratch"""
    if not scratch_floats:
        return 1
    sp = min(16, max(1, 256 // (N * heads)))
    while sp > 1 and N * heads * sp * 130 > scratch_floats:
        sp -= 1
    return sp


def decode_scratch_floats(case):
    """floats of scratch the case hands over: what the key split asks for ("full"), room for 5 splits ("small") or none"""
    nh = case.N * case.heads
    return {"full": nh * min(16, max(1, 256 // nh)) * 130, "small": nh * 5 * 130, "none": 0}[case.scratch]


def sweeps(chunks):
    """trips of the grid-stride loop of a streaming kernel (grid capped at 8192 x 256 threads)"""
    return cdiv(chunks, min(GRID_CAP, cdiv(chunks, 256) * 256))


def route(case):
    """-> (kernel family and template argument, library launches) as the dispatch code decides them"""
    op, p = case.op, case.p
    if op == "norm":
        return norm_route(p["rows"], p["cols"]), 1
    if op == "pullback":
        return pullback_route(p["g"], p["S"]), 1 + 1 + 1        # mask_pullback alone, then upsample_maskpool = pull-back + ONE GEMM launch (no workspace: no split)
    if op == "dice":
        return "dice_bce+fold+bwd", 3
    if op == "align":
        return f"ny{max(1, min(8, p['D'] // 64)) if p['grads'] else 1}", 1 + (p["items"] if p["items"] > 1 else 0)      # batched: + one single launch per item (bit-equality)
    if op == "decode":
        sp = decode_splits(p["N"], p["heads"], decode_scratch_floats(case))
        return f"splits{sp}", (2 if sp > 1 else 1) + 1           # decode_attn (+ its merge), then rope_kv_append on a second set of buffers
    if op == "stride":
        return f"{p['kind']}_sweeps{sweeps(p['chunks'])}", 1
    return op, 1


# ----------------------------------------------------------------------------------------------------------------- the case table
def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # ---- norm: both sides of every switch (rows 64 and 2048, cols 2048 and 8192), every template argument
    shapes = [(r, c) for c in (8, 520, 1280, 1544, 2040, 2048, 2056, 4096, 8192, 8200) for r in (3, 64)]
    shapes += [(1, 2048), (5, 2048), (63, 2048), (1, 8192), (5, 8200), (63, 8192), (63, 4096), (5, 520), (1, 1280), (2047, 2048), (2048, 2048)]
    kinds = (("rms", 0), ("ln", 0), ("ln", 1))          # no RMS + bias: the RMS form has no bias (the kernel ignores one), and every caller passes None
    for i, (rows, cols) in enumerate(shapes):
        every = rows in (3, 64) or (rows, cols) == (63, 8192)              # RMS, LayerNorm and LayerNorm + bias on every route
        for k, (kind, bias) in enumerate(kinds):
            if not every and k != i % 3:
                continue
            ld, rmap = (1, 1) if every else ((0, 0), (1, 0), (0, 1), (1, 1))[(i // 3 + i) % 4]
            add("norm", f"{rows}x{cols}_{kind}{'_bias' if bias else ''}{'_ld' if ld else ''}{'_map' if rmap else ''}", 1, rows=rows, cols=cols, rms=int(kind == "rms"),
                bias=bias, ld=ld, map=rmap)
    # ---- rope: rows = several multiples of a T that is no power of two; heads = q and k of a packed q|k|v, or all of a plain tensor
    for hd, packed, ld in ((16, 1, 1), (64, 1, 0), (128, 1, 1), (128, 0, 0), (64, 0, 1)):
        add("rope", f"hd{hd}_{'qk_of_qkv' if packed else 'plain'}{'_ld' if ld else ''}", 1, hd=hd, packed=packed, ld=ld, N=3, T=5, nh=3)
    # ---- act
    for act in ACTS:
        for n, inplace in ((8, 1), (8 * 257, 0), (8 * 257, 1)):
            add("act", f"{act}_n{n}{'_inplace' if inplace else ''}", 1, act=act, n=n, inplace=inplace)
    # ---- swiglu, add_rows
    for rows, I, ld in ((5, 24, 1), (77, 512, 0), (1, 8, 1)):
        add("swiglu", f"{rows}x{I}{'_ld' if ld else ''}", 1, rows=rows, I=I, ld=ld)
    for ar, rep, cols in ((5, 3, 24), (5, 1, 24), (50, 3, 64)):
        add("add_rows", f"{ar * rep}rows_add{ar}x{cols}", 1, ar=ar, rep=rep, cols=cols)
    # ---- rope_kv_append and decode_attn (head_dim 128, cache capacity 130): every position class on the 16-split route (pos 16: nk = 17, 14 empty splits),
    # a split count between 2 and 15, one split because N * heads > 256, no scratch, a scratch that holds 5 of the 16 splits, scores up to +/-60
    for pos in (0, 15, 16, 63, 64, 65, 129):
        add("decode", f"N1_h2_pos{pos}", 3, N=1, heads=2, pos=pos, scratch="full", qscale=1.0)
    for name, l, kw in (("N3_h8_pos65", 3, dict(N=3, heads=8, pos=65, scratch="full")), ("N3_h8_pos129", 3, dict(N=3, heads=8, pos=129, scratch="full")),
                        ("N33_h8_pos63_onesplit", 2, dict(N=33, heads=8, pos=63, scratch="full")), ("N1_h2_pos64_noscratch", 2, dict(N=1, heads=2, pos=64, scratch="none")),
                        ("N1_h2_pos129_smallscratch", 3, dict(N=1, heads=2, pos=129, scratch="small")), ("N2_h4_pos129_scores60", 3, dict(N=2, heads=4, pos=129, scratch="full", qscale=25.0))):
        add("decode", name, l, **{"qscale": 1.0, **kw})
    # ---- cosine scores: one wave per proposal; K % 4 tails, D below, at and off the 64 lanes
    for K, D in ((1, 8), (5, 64), (37, 200), (256, 256), (64, 640)):
        add("cosine", f"K{K}_D{D}", 1, K=K, D=D)
    # ---- align (KL) + IoP regression losses: gridDim.y = 1, 1, 3, 4, 8 column chunks of the gradient pass, a ragged last chunk at D = 200
    for K, D in ((1, 8), (5, 64), (37, 200), (256, 256), (64, 640)):
        for grads, items in ((0, 1), (1, 1), (1, 3)):
            add("align", f"K{K}_D{D}{'_grads' if grads else ''}{'_items3' if items > 1 else ''}", 1 + (items if items > 1 else 0), K=K, D=D, grads=grads, items=items)
    add("align", "K37_D200_items3", 4, K=37, D=200, grads=0, items=3)
    # ---- the second trip of a grid-stride loop: 8192 * 256 + 8 chunks
    add("stride", "act_gelu", 1, kind="act", chunks=GRID_CAP + 8)
    add("stride", "swiglu", 1, kind="swiglu", chunks=GRID_CAP + 8, I=320)
    # ---- exact copies
    add("patchify", "p14_rowoff", 1, pp=14, B=2, H=28, W=42, ldo=592, extra=1, off=1)
    add("patchify", "p16_ldo", 1, pp=16, B=2, H=32, W=16, ldo=776, extra=0, off=0)
    add("patchify", "p16_dense", 1, pp=16, B=1, H=16, W=48, ldo=768, extra=0, off=0)
    for B, H, W, Cc in ((2, 3, 5, 8), (1, 1, 4, 16), (1, 6, 1, 8)):
        add("im2col3x3", f"{B}x{H}x{W}x{Cc}", 1, B=B, H=H, W=W, C=Cc)
    for strided in (0, 1):
        add("embed_splice", "strided_feats" if strided else "dense_feats", 1, strided=strided)
    add("gather_rows", "dup_unsorted_ld", 1, n=10, cols=24, ld=40)
    add("gather_rows", "dense", 1, n=10, cols=264, ld=264)
    # ---- mask pull-back and pooling
    for g, S in ((64, 256), (16, 64), (8, 64), (16, 33), (32, 32)):
        for first in ("hard", "seam"):
            add("pullback", f"g{g}_S{S}_{first}", 3, g=g, S=S, first=first, C=64)
    # ---- dice / BCE forward and backward
    for M in (1, 3):
        for HW in (1, 255, 257, 4096):
            add("dice", f"M{M}_HW{HW}", 3, M=M, HW=HW)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- norm
def norm_inputs(case):
    g = _g(case)
    r, c = case.rows, case.cols
    z = torch.randn(r, c, generator=g)
    off = torch.randn(r, 1, generator=g)
    off = torch.sign(off) * (0.7 + 0.5 * off.abs())                     # a mean of the order of the row's sigma on every row
    x = 0.005 * (z + off)                                               # small x: eps = 1e-5 is ~40 % of the variance
    if r >= 3:
        x[1] = 2.0 ** -8                                                # a constant row (a power of two: its fp32 sum is exact): variance 0, eps decides
    xb = (JUNK + 0.25 * torch.arange(c + 8 if case.ld else c)).repeat(r, 1)      # the slack of a strided x: finite and varied
    xb[:, :c] = x
    w = (1.0 + 0.5 * torch.randn(c, generator=g)).to(BF)
    b = (0.5 * torch.randn(c, generator=g)).to(BF) if case.bias else None
    out_rows, rm = r, None
    if case.map:
        out_rows = r + 3
        rm = (torch.randperm(out_rows - 1, generator=g)[:r] + 1).to(torch.int32)      # a permutation with gaps; output row 0 is never a target
        if r >= 3:
            rm[r - 1] = -1
        if r >= 5:
            rm[0] = -1
    return dict(x=xb.to(BF), w=w, b=b, eps=1e-5, row_map=rm, out_rows=out_rows, ldy=c + 16 if case.ld else c)


def norm_compute(case, inp, mut=None, emu=None):
    r, c = case.rows, case.cols
    x = inp["x"].reshape(-1)[:r * c].view(r, c) if mut == "ldx_taken_as_cols" else inp["x"][:, :c]
    x, w = _T(x, emu), _T(inp["w"], emu)
    eps = 0.0 if mut == "eps_dropped" else float(np.float32(inp["eps"]))
    div = norm_padded_width(r, c) if mut == "stats_over_padded_width" else c
    aux = {}
    if case.rms:
        rstd = ((x * x).sum(-1, keepdim=True) / div + eps).rsqrt()
        u = x * rstd
        ub = u.to(BF).to(u.dtype)                                       # the operation's own rounding (HF LlamaRMSNorm), in the reference too
        y = w * ub
        if not emu and mut is None:                                     # either neighbour is correct where u sits on a rounding boundary at fp32 resolution
            ulp = torch.exp2(torch.floor(torch.log2(ub.abs().clamp_min(1e-30))) - 7)
            tie = ((u - ub).abs() - ulp / 2).abs() <= 2.0 ** -21 * u.abs()
            aux["extra:y"] = w.abs() * ulp * tie * (0.0 if PLAIN else 1.0)
    else:
        mean = x.sum(-1, keepdim=True) / div
        xc = x - mean
        if mut == "variance_without_mean":
            var = (x * x).sum(-1, keepdim=True) / div
        else:
            var = ((xc * xc).sum(-1, keepdim=True) + (div - c) * mean * mean) / div      # the zero padding of the chunk enters the centred sum too
        y = xc * (var + eps).rsqrt() * w
        if inp["b"] is not None and mut != "bias_dropped":
            y = y + _T(inp["b"], emu)
    y = _rb(y, emu)
    rm = inp["row_map"]
    dst = torch.arange(r) if (rm is None or mut == "row_map_ignored") else rm.long()
    sel = dst >= 0
    if mut == "last_row_dropped":
        sel = sel.clone()
        sel[int(torch.nonzero(sel).flatten()[-1])] = False
    out = torch.full((inp["out_rows"], inp["ldy"]), NAN, dtype=F64)
    out[dst[sel], :c] = y[sel]
    if mut == "minus_one_written_to_row0":
        out[0, :c] = y[int(torch.nonzero(rm < 0).flatten()[0])]
    if mut == "last_chunk_dropped":
        out[:, c - 8:c] = NAN
    if "extra:y" in aux:
        e = torch.zeros_like(out)
        e[dst[sel], :c] = aux["extra:y"][sel]
        aux["extra:y"] = e
    aux["width:y"] = c
    return {"y": out}, aux


def norm_mutants(case):
    m = ["eps_dropped", "last_chunk_dropped", "last_row_dropped"]
    if not case.rms:
        m.append("variance_without_mean")
    if case.bias:
        m.append("bias_dropped")
    if norm_padded_width(case.rows, case.cols) >= 1.1 * case.cols:      # rstd moves by sqrt(width / cols) - 1 >= 4.9 %: twice the bound's 2^-6 |ref| at |ref| >= sigma.
                                                                        # Of the table's columns the registers of a route pad 8, 520, 1280, 1544 and 2056 by that much
        m.append("stats_over_padded_width")
    if case.map:
        m.append("row_map_ignored")
        if case.rows >= 3:
            m.append("minus_one_written_to_row0")
    if case.ld and case.rows > 1:
        m.append("ldx_taken_as_cols")
    return m


# ---------------------------------------------------------------------------------------------------------------------------- rope
def rope_inputs(case):
    g = _g(case)
    rows, hd = case.N * case.T, case.hd
    width = (3 if case.packed else 1) * case.nh * hd
    x = torch.randn(rows, width + (8 if case.ld else 0), generator=g).to(BF)
    ang = torch.rand(rows, hd // 2, generator=g) * 6.28                 # a table of `rows` positions: the kernel is handed the first T
    return dict(x=x, cos=ang.cos().float().contiguous(), sin=ang.sin().float().contiguous(), heads=(2 if case.packed else 1) * case.nh)


def rope_compute(case, inp, mut=None, emu=None):
    rows, hd, T, h2 = case.N * case.T, case.hd, case.T, case.hd // 2
    heads = inp["heads"]
    hrot = 3 * case.nh if mut == "v_rotated_too" else heads - 1 if mut == "last_head_dropped" else heads
    pos = torch.arange(rows) if mut == "position_not_wrapped" else torch.arange(rows) % T
    c, s = inp["cos"][pos][:, None].to(F64), inp["sin"][pos][:, None].to(F64)
    if mut == "sine_sign_flipped":
        s = -s
    x = inp["x"].to(F64)
    xv = x[:, :hrot * hd].reshape(rows, hrot, hd)
    a, b = (xv[..., 0::2], xv[..., 1::2]) if mut == "interleaved_pairs" else (xv[..., :h2], xv[..., h2:])
    if emu:                                                             # fmaf(a, c, -(b * s)): the inner product rounded to fp32, then one rounding of the sum
        o1 = (a * c - (b.float() * s.float()).double()).float().double()
        o2 = (b * c + (a.float() * s.float()).double()).float().double()
    else:
        o1, o2 = a * c - b * s, b * c + a * s
    o = torch.stack([o1, o2], -1).flatten(-2) if mut == "interleaved_pairs" else torch.cat([o1, o2], -1)
    out = x.clone()
    out[:, :hrot * hd] = _rb(o.reshape(rows, hrot * hd), emu)
    exact = torch.zeros_like(out, dtype=torch.bool)
    exact[:, heads * hd:] = True                                        # v and the slack: bit for bit what they were
    return {"x": out}, {"exact:x": exact}


def rope_mutants(case):
    m = ["position_not_wrapped", "sine_sign_flipped", "interleaved_pairs", "last_head_dropped"]
    if case.packed:
        m.append("v_rotated_too")
    return m


# ----------------------------------------------------------------------------------------------------------------------------- act
GELU_TAIL = 0.5 * (1.5e-7 + 2.0 ** -24)        # * |x| for x <= -3 (module docstring)


def act_values(n, g):
    if n == 8:
        return torch.tensor([-12.0, -3.5, -0.0, 0.0, 0.4375, 3.0, 12.0, -1.0])
    special = torch.tensor([0.0, -0.0, 0.0, -3.0, -3.5, -4.0, -4.5, -5.0, -5.5, -6.0, -7.0, -8.0, -10.0, -12.0, 12.0, 3.0])
    v = torch.cat([torch.linspace(-12, 12, n - len(special)), special])
    return torch.sort(v, descending=True).values                      # sorted: the 8 values of a chunk (a "row" of the bound) are of one magnitude; the last chunk
                                                                       # holds -12, where no activation is the identity (an in-place chunk left alone shows)


def act_inputs(case):
    return dict(x=act_values(case.n, _g(case)).to(BF))


def act_apply(v, act, emu, mut=None):
    """v fp32 (emulation) or fp64 -> the activation, before the bf16 store"""
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "gelu":
        if mut == "tanh_gelu":
            return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))
        if not emu:
            return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
        z = v.abs() * 0.70710678118654752
        t = 1.0 / (0.3275911 * z + 1.0)
        poly = t * (t * (t * (t * (t * 1.061405429 + -1.453152027) + 1.421413741) + -0.284496736) + 0.254829592)
        erfa = 1.0 - poly * _exp(-z * z, emu)
        return 0.5 * v * (1.0 + torch.copysign(erfa, v))
    if act == "quickgelu":
        return v * _sigmoid((1.0 if mut == "quickgelu_constant_1" else 1.702) * v, emu)
    if act == "silu":
        return v * _sigmoid(v, emu)
    return _sigmoid(v, emu)


def act_compute(case, inp, mut=None, emu=None):
    v = _T(inp["x"], emu)
    y = _rb(act_apply(v, case.act, emu, mut), emu).view(-1, 8).clone()
    if mut == "last_chunk_dropped":
        y[-1] = inp["x"].to(F64)[-8:] if case.inplace else NAN          # in place: the input stays
    aux = {}
    if case.act == "relu":
        aux["exact:y"] = torch.ones_like(y, dtype=torch.bool)
    if case.act == "gelu":
        aux["extra:y"] = torch.where(inp["x"].to(F64) <= -3.0, GELU_TAIL * inp["x"].to(F64).abs(), torch.zeros(())).view(-1, 8)
    return {"y": y}, aux


def act_mutants(case):
    m = ["last_chunk_dropped"] + (["quickgelu_constant_1"] if case.act == "quickgelu" else [])
    if case.act == "gelu" and case.n > 8:              # tanh-GELU is off by <= 5e-4 near |x| = 2..3: it shows against the sigma of a chunk of one magnitude, not of -12 .. 12
        m.append("tanh_gelu")
    return m


# ---------------------------------------------------------------------------------------------------------------- swiglu, add_rows
def swiglu_inputs(case):
    g = _g(case)
    I = case.I
    gu = torch.randn(case.rows, 2 * I + (8 if case.ld else 0), generator=g) * 2.0
    gu[:, 2 * I:] = JUNK
    return dict(gu=gu.to(BF), ldo=I + (16 if case.ld else 0))


def swiglu_compute(case, inp, mut=None, emu=None):
    rows, I = case.rows, case.I
    gu = inp["gu"].reshape(-1)[:rows * 2 * I].view(rows, 2 * I) if mut == "ldgu_taken_as_2I" else inp["gu"]
    a, u = _T(gu[:, :I], emu), _T(gu[:, I:2 * I], emu)
    if mut == "gate_up_swapped":
        a, u = u, a
    y = _rb(a / (1.0 + _exp(-a, emu)) * u, emu)
    if mut == "last_chunk_dropped":
        y[-1, -8:] = NAN
    return {"y": _pad(y, inp["ldo"])}, {"width:y": I}


def swiglu_mutants(case):
    return ["gate_up_swapped", "last_chunk_dropped"] + (["ldgu_taken_as_2I"] if case.ld and case.rows > 1 else [])


def addrows_inputs(case):
    g = _g(case)
    ar, cols = case.ar, case.cols
    return dict(x=torch.randn(ar * case.rep, cols, generator=g).to(BF), add=torch.randn(ar * case.rep, cols, generator=g).to(BF))     # the kernel is handed add[:ar]


def addrows_compute(case, inp, mut=None, emu=None):
    rows = case.ar * case.rep
    idx = torch.arange(rows) % (rows if mut == "added_row_indexed_by_row_mod_rows" else case.ar)
    y = _rb(_T(inp["x"], emu) + _T(inp["add"], emu)[idx], emu)
    if mut == "last_chunk_dropped":
        y[-1, -8:] = NAN
    return {"y": y}, {}


def addrows_mutants(case):
    return ["last_chunk_dropped"] + (["added_row_indexed_by_row_mod_rows"] if case.rep > 1 else [])


# ------------------------------------------------------------------------------------------------- the second trip of a stride loop
def stride_sample(chunks):
    """the chunks that are compared: every 4099th and the last 64 (the 8 of the second sweep among them)"""
    return torch.unique(torch.cat([torch.arange(0, chunks, 4099), torch.arange(chunks - 64, chunks)]))


def stride_inputs(case):
    g = _g(case)
    n8 = case.chunks
    if case.kind == "act":
        return dict(x=(torch.randn(n8 * 8, generator=g) * 3.0).to(BF), idx=stride_sample(n8))
    ich = case.I // 8
    assert n8 % ich == 0
    return dict(gu=(torch.randn(n8 // ich, 2 * case.I, generator=g) * 2.0).to(BF), idx=stride_sample(n8))


def stride_compute(case, inp, mut=None, emu=None):
    idx = inp["idx"]
    if case.kind == "act":
        y = act_apply(_T(inp["x"].view(-1, 8)[idx], emu), "gelu", emu)
    else:
        ich = case.I // 8
        row, c = idx // ich, idx % ich
        gu = inp["gu"].view(-1, 2, ich, 8)
        a, u = _T(gu[row, 0, c], emu), _T(gu[row, 1, c], emu)
        y = a / (1.0 + _exp(-a, emu)) * u
    y = _rb(y, emu).clone()
    if mut == "beyond_first_sweep_unwritten":
        y[idx >= GRID_CAP] = NAN
    return {"y": y}, {}


# ------------------------------------------------------------------------------------------------------------------- exact copies
def patchify_inputs(case):
    return dict(img=torch.randn(case.B, 3, case.H, case.W, generator=_g(case)).to(BF))


def patchify_compute(case, inp, mut=None, emu=None):
    B, p, H, W, ldo = case.B, case.pp, case.H, case.W, case.ldo
    gh, gw = H // p, W // p
    n, rpi = gh * gw, gh * gw + case.extra
    t = inp["img"].to(F64).view(B, 3, gh, p, gw, p)
    t = (t.permute(0, 2, 4, 3, 5, 1) if mut == "pixel_major_layout" else t.permute(0, 2, 4, 1, 3, 5)).reshape(B, n, 3 * p * p)
    out = torch.full((B, rpi, ldo), NAN, dtype=F64)
    off = 0 if mut == "row_off_ignored" else case.off
    out[:, off:off + n, :3 * p * p] = t
    if mut != "padding_left_unzeroed":
        out[:, off:off + n, 3 * p * p:] = 0.0
    return {"cols": out.view(B * rpi, ldo)}, {}


def patchify_mutants(case):
    return ["pixel_major_layout"] + (["padding_left_unzeroed"] if case.ldo > 3 * case.pp ** 2 else []) + (["row_off_ignored"] if case.off else [])


def im2col_inputs(case):
    return dict(x=torch.randn(case.B, case.H, case.W, case.C, generator=_g(case)).to(BF))


def im2col_compute(case, inp, mut=None, emu=None):
    B, H, W, Cc = case.B, case.H, case.W, case.C
    x = inp["x"].to(F64)
    if mut == "border_wraps":
        xp = torch.cat([x[:, -1:], x, x[:, :1]], 1)
        xp = torch.cat([xp[:, :, -1:], xp, xp[:, :, :1]], 2)
    else:
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.empty(B, H, W, 9, Cc, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            out[:, :, :, (kx * 3 + ky) if mut == "tap_order_transposed" else (ky * 3 + kx)] = xp[:, ky:ky + H, kx:kx + W]
    return {"cols": out.view(B * H * W, 9 * Cc)}, {}


SPLICE = dict(N=5, L=6, P=3, Hd=16, V=10)


def splice_inputs(case):
    g = _g(case)
    N, L, P, Hd, V = (SPLICE[k] for k in ("N", "L", "P", "Hd", "V"))
    ids = torch.randint(0, V, (N, L), generator=g)
    ids[0, 0] = -200                                  # the image token first
    ids[1, L - 1] = -200                              # ... and last
    ids[2, 2], ids[2, 3] = -200, -200                 # two in a row: the first wins, the second is an id below 0 (clamped)
    ids[3, 1], ids[3, 3], ids[3, 4] = -200, -5, V + 3       # ids below 0 and >= vocab are clamped
    ids[4, 2], ids[4, 5] = -200, -200                 # two apart
    buf = torch.randn(N, P + 1, Hd, generator=g).to(BF)     # strided: a CLS row in front of every image's block
    return dict(ids=ids, embed=torch.randn(V, Hd, generator=g).to(BF), buf=buf)


def splice_feats(case, inp):
    """-> (the flat tensor the kernel's feats pointer starts at, the stride between images in elements)"""
    Hd, P = SPLICE["Hd"], SPLICE["P"]
    if case.strided:
        return inp["buf"].reshape(-1)[Hd:], (P + 1) * Hd
    return inp["buf"][:, 1:].contiguous().reshape(-1), P * Hd


def splice_compute(case, inp, mut=None, emu=None):
    N, L, P, Hd, V = (SPLICE[k] for k in ("N", "L", "P", "Hd", "V"))
    flat, stride = splice_feats(case, inp)
    flat = torch.cat([flat.to(F64), torch.full((Hd * (P + 1),), JUNK, dtype=F64)])
    if mut == "feats_stride_ignored":
        stride = P * Hd
    emb, ids = inp["embed"].to(F64), inp["ids"]
    out = torch.empty(N, L - 1 + P, Hd, dtype=F64)
    for n in range(N):
        hits = torch.nonzero(ids[n] == -200).flatten().tolist()
        ip = hits[1] if (mut == "second_image_token_used" and len(hits) > 1) else hits[0]
        for t in range(L - 1 + P):
            if ip <= t < ip + P:
                out[n, t] = flat[n * stride + (t - ip) * Hd:n * stride + (t - ip + 1) * Hd]
            else:
                j = t if t < ip else t - P + (0 if mut == "ids_after_image_shifted_by_one" else 1)
                out[n, t] = emb[min(max(int(ids[n, min(j, L - 1)]), 0), V - 1)]
    return {"out": out.view(N * (L - 1 + P), Hd)}, {}


def splice_mutants(case):
    return ["second_image_token_used", "ids_after_image_shifted_by_one"] + (["feats_stride_ignored"] if case.strided else [])


def gather_inputs(case):
    g = _g(case)
    x = torch.randn(case.n, case.ld, generator=g).to(BF)
    return dict(x=x, idx=torch.tensor([3, 9, 0, 3, 7, 7, 1], dtype=torch.int64))


def gather_compute(case, inp, mut=None, emu=None):
    x = inp["x"].to(F64)
    x = x.reshape(-1)[:case.n * case.cols].view(case.n, case.cols) if mut == "ldx_taken_as_cols" else x[:, :case.cols]
    idx = inp["idx"]
    if mut == "index_sorted":
        idx = torch.sort(idx).values
    return {"out": x[idx].clone()}, {}


def gather_mutants(case):
    return ["index_sorted"] + (["ldx_taken_as_cols"] if case.ld > case.cols else [])


# -------------------------------------------------------------------------------------------------------- mask pull-back and pooling
def pullback_inputs(case):
    gen = _g(case)
    g, S, Cc = case.g, case.S, case.C
    segs = torch.zeros(3, S, S)
    if case.first == "hard":
        segs[0] = (torch.rand(S, S, generator=gen) > 0.7).float()
    else:                                             # 1 only in the row where the kernel's two halves meet, and on the four borders
        segs[0, (S + 1) // 2] = 1.0
        segs[0, 0], segs[0, -1], segs[0, :, 0], segs[0, :, -1] = 1.0, 1.0, 1.0, 1.0
    segs[1] = torch.rand(S, S, generator=gen)                          # a soft mask; segs[2] stays empty
    return dict(segs=segs.to(BF), feat=torch.randn(g * g, Cc, generator=gen).to(BF))


def bilinear_matrix(S, g, dtype, kind=None):
    """U [S, g]: weight of destination pixel p on source cell (F.interpolate bilinear, align_corners = False, clamped at the borders).  fp32: as the kernel
    computes it; kind: 'align_corners' or 'unclamped' (the mutants)"""
    f = (lambda v: torch.tensor(v, dtype=dtype))
    p = torch.arange(S, dtype=dtype)
    if kind == "align_corners":
        s = p * ((g - 1) / (S - 1)) if S > 1 else p * 0
    else:
        s = (p + 0.5) * (f(g) / f(S)) - 0.5
        if kind != "unclamped":
            s = s.clamp_min(0.0)
    c0 = torch.floor(s)
    l1 = s - c0
    c0 = c0.long()
    c1 = (c0 + 1).clamp_max(g - 1)
    U = torch.zeros(S, g + 1, dtype=dtype)                              # column g: the cell -1 of the unclamped mutant (its weight is lost)
    U.scatter_add_(1, torch.where(c0 < 0, g, c0)[:, None], (1 - l1)[:, None])
    U.scatter_add_(1, c1[:, None], l1[:, None])
    return U[:, :g]


def pullback_adjoint(segs64, g, S):
    """the fp64 adjoint of F.interpolate(bilinear, align_corners = False), taken by autograd"""
    x0 = torch.zeros(1, segs64.shape[0], g, g, dtype=F64, requires_grad=True)
    (F.interpolate(x0, size=(S, S), mode="bilinear", align_corners=False)[0] * segs64).sum().backward()
    return x0.grad[0].reshape(segs64.shape[0], g * g)


def pullback_compute(case, inp, mut=None, emu=None):
    g, S = case.g, case.S
    m = _T(inp["segs"], emu)
    feat = _T(inp["feat"], emu)
    if mut == "seam_row_dropped":
        m = m.clone()
        m[:, (S + 1) // 2] = 0
    if emu or mut in ("align_corners_weights", "border_clamp_dropped"):
        U = bilinear_matrix(S, g, F32 if emu else F64, {"align_corners_weights": "align_corners", "border_clamp_dropped": "unclamped"}.get(mut))
        pb = torch.einsum("py,kpq,qx->kyx", U, m, U).reshape(3, g * g)       # rows, then columns: the kernel's order
    else:
        pb = pullback_adjoint(m, g, S)
    wsum = pb.sum(-1)
    if mut == "wsum_from_mask_area":
        wsum = (m != 0).to(m.dtype).flatten(1).sum(-1)
    eps = 0.0 if mut == "normaliser_eps_missing" else float(np.float32(1e-8))
    wn = _rb(pb * (1.0 / (wsum + eps))[:, None], emu)
    pooled = _rb(wn.to(BF).to(feat.dtype) @ feat, emu)                  # the GEMM's operand IS the bf16 wn: its rounding is checked on wn, not again here
    out = {"wn": wn, "pb": pb.to(F64), "wsum": wsum.to(F64), "pooled": pooled}
    aux = {}
    if not emu and mut is None:
        taps = (math.ceil(2 * S / g) + 2) ** 2                          # pixels that reach one cell
        # all terms are >= 0: sum |t| is the sum.  A term is m * wx * wy with weights that are the fractional part of an fp32 coordinate <= g, known to
        # g * 2^-23 absolutely (not relatively: a small weight of a non-dyadic S / g carries the full coordinate error): + g 2^-23 sum m (wx + wy)
        U = bilinear_matrix(S, g, F64)
        ind = (U > 0).to(F64)
        coord = g * 2.0 ** -23 * (torch.einsum("py,kpq,qx->kyx", U, m, ind) + torch.einsum("py,kpq,qx->kyx", ind, m, U)).reshape(3, g * g)
        aux = {"bound:pb": f32_bound(taps, pb) + (0.0 if PLAIN else coord), "sum:wsum": (S * S, wsum)}
    return out, aux


def pullback_mutants(case):
    m = ["seam_row_dropped", "normaliser_eps_missing", "wsum_from_mask_area"]
    return m + (["align_corners_weights", "border_clamp_dropped"] if case.S > case.g else [])


# ----------------------------------------------------------------------------------------------------------------------- dice / BCE
DICE_G = (0.5, 2.0)
NUM_MASKS = 3.0


def dice_inputs(case):
    g = _g(case)
    M, HW = case.M, case.HW
    x = torch.rand(M, HW, generator=g) * 60.0 - 30.0
    if HW > 1:
        x[0, 0], x[0, -1] = 30.0, -30.0
    else:
        x[:, 0] = torch.tensor([0.75, -1.25, 2.5])[:M]      # the only pixel: unsaturated, so that both gradients have weight
    y = (torch.rand(M, HW, generator=g) > 0.5).float()
    if M == 3:
        y[1], y[2] = 0.0, 1.0                          # an all-zero and an all-one target
    return dict(x=x, y=y, g=torch.tensor(DICE_G))


def dice_formula(x, y, g0, g1, emu, mut=None):
    """the kernels' arithmetic -> (out [2], dx [M, HW]) and the terms the bounds are made of"""
    M, HW = x.shape
    keep = HW // 256 * 256 if mut == "hw_tail_dropped" else HW
    xs, ys = x[:, :keep], y[:, :keep]
    s = _sigmoid(xs, emu)
    sc = 1.0 if mut == "scale_missing" else 1000.0
    eps = 1e-6
    inv = 1.0 / float(np.float32(NUM_MASKS + 1e-8))
    Nn = 2.0 * (s * ys).sum(-1) / sc + eps
    D = s.sum(-1) / sc + ys.sum(-1) / sc + eps
    bce_t = xs.clamp_min(0.0) - xs * ys + torch.log1p(_exp(-xs.abs(), emu))
    hw = 1.0 if mut == "bce_not_averaged" else float(HW)
    out = torch.stack([((1.0 - Nn / D) * inv).sum(), (bce_t.sum(-1) / hw * inv).sum()])
    if mut == "g_swapped":
        g0, g1 = g1, g0
    gd, gb = (g0 * inv / (sc * D * D))[:, None], g1 * inv / hw
    nterm = 0.0 if mut == "dice_gradient_without_N" else Nn[:, None]
    dx = torch.full_like(x, NAN)
    dx[:, :keep] = -gd * (2.0 * ys * D[:, None] - nterm) * s * (1.0 - s) + gb * (s - ys)
    terms = dict(dice=((1.0 + 2.0 * Nn / D) * inv).sum(), bce=((xs.clamp_min(0.0) + (xs * ys).abs() + torch.log1p(torch.exp(-xs.abs()))).sum(-1) / hw * inv).sum(),
                 dx=gd.abs() * (2.0 * ys * D[:, None] + Nn[:, None]) * s * (1.0 - s) + abs(gb) * (s + ys))
    return out, dx, terms


def dice_compute(case, inp, mut=None, emu=None):
    x, y = _T(inp["x"], emu), _T(inp["y"], emu)
    g0, g1 = (float(np.float32(v)) for v in DICE_G)
    if emu or mut:
        out, dx, _ = dice_formula(x, y, g0, g1, emu, mut)
        return {"out": out.to(F64), "dx": dx.to(F64)}, {}
    xr = x.clone().requires_grad_(True)                                # the reference: the oracle's losses in fp64 and their autograd gradient
    ld, lb = olosses.dice(xr[:, None], y[:, None], NUM_MASKS), olosses.sigmoid_ce(xr[:, None], y[:, None], NUM_MASKS)
    (dx,) = torch.autograd.grad(g0 * ld + g1 * lb, xr)
    _, _, t = dice_formula(x, y, g0, g1, None)
    HW = case.HW
    # dice_m = 1 - N / D: N and D are sums of HW terms >= 0, so their relative error is that of the sum and N / D carries both; BCE: 3 terms per pixel
    bound = torch.stack([f32_bound(HW + 1, t["dice"]), f32_bound(3 * HW, t["bce"])])
    return {"out": torch.stack([ld, lb]).detach(), "dx": dx}, {"bound:out": bound, "bound:dx": f32_bound(2, t["dx"], c=C_DLOGITS)}


def dice_mutants(case):
    m = ["bce_not_averaged", "g_swapped", "dice_gradient_without_N"]
    if case.HW % 256:
        m.append("hw_tail_dropped")
    if case.HW == 1:
        # the 1/1000 scale only moves eps = 1e-6 against the sums (the loss is a ratio of two sums that carry the same scale), so its effect falls as 1 / HW:
        # it is within fp32 resolution of the loss from 255 pixels on, and no tolerance can protect it at a realistic HW.  It shows on one pixel.
        m.append("scale_missing")
        m.remove("bce_not_averaged")                   # HW = 1: the mean is the sum
    return m


# -------------------------------------------------------------------------------------------------------------------- cosine scores
def cosine_inputs(case):
    g = _g(case)
    return dict(t=(torch.randn(case.D, generator=g) + 0.3).to(BF), e=(torch.randn(case.K, case.D, generator=g) * torch.rand(case.K, 1, generator=g) * 4 + 0.3).to(BF))


def cosine_compute(case, inp, mut=None, emu=None):
    t, e = _T(inp["t"], emu), _T(inp["e"], emu)
    if mut == "last_lane_group_dropped":               # the columns beyond the last multiple of 64
        t, e = t[:case.D // 64 * 64], e[:, :case.D // 64 * 64]
    dot, ne, nt = (e * t).sum(-1), (e * e).sum(-1).sqrt(), (t * t).sum().sqrt()
    sim = dot / (ne * (1.0 if mut == "target_norm_missing" else nt))
    if mut == "last_row_dropped":
        sim = sim.clone()
        sim[-1] = NAN
    aux = {"bound:sim": f32_bound(case.D, (e * t).abs().sum(-1) / (ne * nt), c=C_COS)} if not emu and mut is None else {}
    return {"sim": sim.to(F64)}, aux


def cosine_mutants(case):
    return ["target_norm_missing", "last_row_dropped"] + (["last_lane_group_dropped"] if case.D % 64 else [])      # D < 64: nothing is left, 0 / 0


# ------------------------------------------------------------------------------------------------------------ align_reg_loss
TAU = 0.05


def align_inputs(case):
    g = _g(case)
    R, K, D = case.items, case.K, case.D
    e = (torch.randn(R, K, D, generator=g) * (0.5 + torch.rand(R, K, 1, generator=g) * 3) + 0.2).to(BF)
    t = (torch.randn(R, D, generator=g) + 0.2).to(BF)
    gi, gp = torch.rand(R, K, generator=g), torch.rand(R, K, generator=g)
    if K >= 5:
        gi[:, ::3] = 0.0                               # exact zeros, and one dominant entry (softmax of gt / tau: e^20 over a zero)
        gi[:, 1] = 1.0
    return dict(e=e, t=t, gi=gi, gp=gp, pr=torch.rand(R, K, generator=g).to(BF))


def align_kernel_formula(e, t, gi, pr, gp, tau, emu):
    """one item, the kernel's arithmetic -> (out [2], d_e, d_t, d_pred) and the quantities the bounds are made of"""
    K, D = e.shape
    tn = (t * t).sum().sqrt()
    ne = (e * e).sum(-1).sqrt()
    cs = (e * t).sum(-1) / (ne * tn)
    a, b = cs / tau, gi / tau
    lse_s = a.max() + torch.log(_exp(a - a.max(), emu).sum())
    lse_g = b.max() + torch.log(_exp(b - b.max(), emu).sum())
    lg, ls = b - lse_g, a - lse_s
    pg, ps = _exp(lg, emu), _exp(ls, emu)
    kl = torch.where(pg > 0, pg * (lg - ls), torch.zeros_like(pg)).sum()
    w = _exp(gp - 1.0, emu)
    rg = ((pr - gp) * (pr - gp) * w).sum() / K * 50.0
    d_pred = 2.0 * (pr - gp) * w * 50.0 / K
    gk, ie, itn = ((ps - pg) / tau)[:, None], (1.0 / ne)[:, None], 1.0 / tn
    c = cs[:, None]
    d_e = gk * (t * ie * itn - c * e * ie * ie)
    d_t = (gk * (e * ie * itn - c * t * itn * itn)).sum(0)
    A = (e * t).abs().sum(-1) / (ne * tn * tau)                        # sum of |terms| of the exponent a_k, itself a D-term sum
    G = ((ps + pg) / tau + ps * A / tau)[:, None]                      # |gk| and, to first order, what the terms of a_k move it by (d ps = ps d a_k)
    terms = dict(kl=(pg * (b.abs() + lse_g.abs() + lse_s.abs() + A)).sum(), rg=rg, d_pred=d_pred.abs(),
                 d_e=G * ((t * ie * itn).abs() + (c * e * ie * ie).abs()), d_t=(G * ((e * ie * itn).abs() + (c * t * itn * itn).abs())).sum(0))
    return torch.stack([kl, rg]), d_e, d_t, d_pred, terms


def align_mutant(e, t, gi, pr, gp, mut):
    """one item in fp64, a subtly wrong problem, gradients by autograd"""
    K = e.shape[0]
    e, t, pr = e.clone().requires_grad_(True), t.clone().requires_grad_(True), pr.clone().requires_grad_(True)
    tau = 1.0 if mut == "tau_missing" else float(np.float32(TAU))
    cs = (e @ t) / (e.norm(dim=-1) * (1.0 if mut == "target_norm_missing" else t.norm()))
    ls, lg = torch.log_softmax(cs / tau, 0), torch.log_softmax(gi / tau, 0)
    kl = (ls.exp() * (ls - lg)).sum() if mut == "kl_direction_reversed" else (lg.exp() * (lg - ls)).sum()
    w = torch.ones_like(gp) if mut == "exp_weight_missing" else torch.exp(gp - 1.0)
    rg = ((pr - gp) ** 2 * w).mean() * 50.0
    d_e, d_t = torch.autograd.grad(kl, (e, t))
    (d_pred,) = torch.autograd.grad(rg, pr)
    if mut == "dpred_factor_missing":
        d_pred = d_pred * K / 50.0
    return torch.stack([kl, rg]).detach(), d_e, d_t, d_pred


def align_compute(case, inp, mut=None, emu=None):
    R, K, D = case.items, case.K, case.D
    tau = float(np.float32(TAU))
    outs, aux = {n: [] for n in ("out", "d_e", "d_t", "d_pred")}, {n: [] for n in ("out", "d_e", "d_t", "d_pred")}
    for r in range(R):
        e, t, gi, pr, gp = (_T(inp[k][r], emu) for k in ("e", "t", "gi", "pr", "gp"))
        if emu:
            o, d_e, d_t, d_p, _ = align_kernel_formula(e, t, gi, pr, gp, tau, emu)
        elif mut and mut != "last_column_chunk_zero":
            o, d_e, d_t, d_p = align_mutant(e, t, gi, pr, gp, mut)
        else:                                                            # the reference: the oracle's losses in fp64 and their autograd gradients
            er, tr, pp = e.clone().requires_grad_(True), t.clone().requires_grad_(True), pr.clone().requires_grad_(True)
            la, lr = olosses.softmax_align(er, tr[None], gi[:, None], tau), olosses.iop_regression(pp[:, None], gp[:, None])
            d_e, d_t = torch.autograd.grad(la, (er, tr))
            (d_p,) = torch.autograd.grad(lr, pp)
            o = torch.stack([la, lr]).detach()
            if mut == "last_column_chunk_zero":
                d_e, d_t = d_e.clone(), d_t.clone()
                d_e[:, (D - 1) // 64 * 64:], d_t[(D - 1) // 64 * 64:] = 0.0, 0.0
            else:
                tm = align_kernel_formula(e, t, gi, pr, gp, tau, None)[4]
                aux["out"].append(torch.stack([f32_bound(K + D + 3, tm["kl"]), f32_bound(K + 3, tm["rg"])]))
                aux["d_e"].append(f32_bound(D + 2, tm["d_e"], c=C_DE))
                aux["d_t"].append(f32_bound(K + D, tm["d_t"]))
                aux["d_pred"].append(f32_bound(2, tm["d_pred"], c=C_DPRED))
        for n, v in (("out", o), ("d_e", d_e), ("d_t", d_t), ("d_pred", d_p)):
            outs[n].append(v.to(F64))
    names = ("out", "d_e", "d_t", "d_pred") if case.grads else ("out",)
    return {n: torch.stack(outs[n]) for n in names}, ({f"bound:{n}": torch.stack(aux[n]) for n in names} if aux["out"] else {})


def align_mutants(case):
    m = ["exp_weight_missing"]
    if case.K > 1:                                     # one proposal: both softmaxes are 1, the KL and its gradients 0 whatever tau, the direction or the norm
        m += ["tau_missing", "kl_direction_reversed"]
    if case.grads:
        m.append("dpred_factor_missing")
        if case.K > 1:
            m += ["last_column_chunk_zero", "target_norm_missing"]      # the target norm cancels in the cosine's softmax only up to the gradient d_t
    return m


# ------------------------------------------------------------------------------------------------- rope_kv_append and decode_attn
HD, CAP = 128, 130


def decode_inputs(case):
    g = _g(case)
    N, D, pos = case.N, case.heads * HD, case.pos
    qkv = torch.randn(N, 3 * D, generator=g)
    qkv[:, :D] *= case.qscale                          # qscale 25: scores q . k / sqrt(128) of sigma 25 over 130 keys reach +/-60
    ang = torch.rand(CAP, HD // 2, generator=g) * 6.28
    kc, vc = torch.randn(N, CAP, D, generator=g), torch.randn(N, CAP, D, generator=g)
    kc[:, pos + 1:], vc[:, pos + 1:] = NAN, NAN        # beyond pos: NaN (never read); row pos holds a stale finite row
    return dict(qkv=qkv.to(BF), cos=ang.cos().float().contiguous(), sin=ang.sin().float().contiguous(), kc=kc.to(BF), vc=vc.to(BF), scale=HD ** -0.5)


def _rot(x, c, s, emu):
    """rotate-half of x [..., 128] (fp64 values of bf16 inputs) with cos / sin [64]; emulation: fmaf(a, c, -(b * s)) and fmaf(b, c, a * s)"""
    a, b = x[..., :HD // 2], x[..., HD // 2:]
    if emu:
        return torch.cat([(a * c - (b.float() * s.float()).double()).float().double(), (b * c + (a.float() * s.float()).double()).float().double()], -1)
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def decode_compute(case, inp, mut=None, emu=None):
    """-> out [N, D]; kc / vc: the caches after decode_attn (rope_kv_append must leave the same bits); qkv: rope_kv_append's in-place operand"""
    N, H, pos = case.N, case.heads, case.pos
    D = H * HD
    c, s = inp["cos"][pos].to(F64), inp["sin"][pos].to(F64)
    x = inp["qkv"].to(F64).view(N, 3, H, HD)
    q, kn = _rot(x[:, 0], c, s, emu), _rot(x[:, 1], c, s, emu)
    vn = _rot(x[:, 2], c, s, emu) if mut == "v_rotated" else x[:, 2]
    qb, kb, vb = (t.to(BF).to(F64) for t in (q, kn, vn))            # the op's own roundings: q is used, k and v are stored, as bf16
    kc, vc = inp["kc"].to(F64).clone(), inp["vc"].to(F64).clone()
    wpos = pos + 1 if mut == "k_written_at_pos_plus_1" else pos
    kc[:, wpos] = (kb if emu else kn).reshape(N, D)                 # the new k row takes the bf16 bound against the unrounded rotation
    vc[:, pos] = vb.reshape(N, D)
    K, V = kc.clone(), vc.clone()
    K[:, pos] = kb.reshape(N, D)                                   # the kernel attends to the bf16 row it stores (from LDS, not from the cache)
    if mut == "stale_cache_row_used_for_pos":
        K[:, pos], V[:, pos] = inp["kc"][:, pos].to(F64), inp["vc"][:, pos].to(F64)
    lo, hi = 0, pos + 1
    if mut == "key_pos_excluded":
        hi = pos
    elif mut == "key_pos_plus_1_included":
        hi = pos + 2
    elif mut == "last_split_dropped":
        sp = decode_splits(N, H, decode_scratch_floats(case))
        per = (cdiv(pos + 1, sp) + 15) // 16 * 16
        hi = pos // per * per
    K, V = K[:, lo:hi].reshape(N, hi - lo, H, HD).transpose(1, 2), V[:, lo:hi].reshape(N, hi - lo, H, HD).transpose(1, 2)
    scale = 1.0 if mut == "scale_missing" else float(np.float32(inp["scale"]))
    dt = F32 if emu else F64
    sc = (qb.to(dt)[:, :, None] * K.to(dt)).sum(-1) * scale                   # [N, H, keys]
    e = _exp(sc - sc.amax(-1, keepdim=True), emu) if hi > lo else sc
    o = (e[..., None] * V.to(dt)).sum(-2) / e.sum(-1, keepdim=True)
    qkv2 = inp["qkv"].to(F64).clone()
    qkv2[:, :D] = _rb(q.reshape(N, D), emu)
    exact = {"exact:kc": torch.ones_like(kc, dtype=torch.bool), "exact:vc": torch.ones_like(vc, dtype=torch.bool), "exact:qkv": torch.ones_like(qkv2, dtype=torch.bool)}
    exact["exact:kc"][:, pos] = False
    exact["exact:qkv"][:, :D] = False
    return {"out": _rb(o.reshape(N, D), emu), "kc": kc, "vc": vc, "qkv": qkv2}, exact


def decode_mutants(case):
    if case.qscale > 1:                                # scores of sigma 25: the softmax is all but one-hot on some other key, and what happens to key pos does not reach the output
        return ["v_rotated", "scale_missing"]
    m = ["key_pos_excluded", "stale_cache_row_used_for_pos", "v_rotated"]
    if case.pos > 0:                                   # one key: the softmax is 1 whatever the scale
        m.append("scale_missing")
    if case.pos + 1 < CAP:
        m += ["key_pos_plus_1_included", "k_written_at_pos_plus_1"]
    sp = decode_splits(case.N, case.heads, decode_scratch_floats(case))
    if sp > 1 and case.pos // ((cdiv(case.pos + 1, sp) + 15) // 16 * 16) >= 1:      # the last split that holds keys is not the first
        m.append("last_split_dropped")
    return m


# ----------------------------------------------------------------------------------------------------------------------- registry
OPS = {
    "norm": (norm_inputs, norm_compute, norm_mutants),
    "rope": (rope_inputs, rope_compute, rope_mutants),
    "act": (act_inputs, act_compute, act_mutants),
    "swiglu": (swiglu_inputs, swiglu_compute, swiglu_mutants),
    "add_rows": (addrows_inputs, addrows_compute, addrows_mutants),
    "stride": (stride_inputs, stride_compute, lambda c: ["beyond_first_sweep_unwritten"]),
    "patchify": (patchify_inputs, patchify_compute, patchify_mutants),
    "im2col3x3": (im2col_inputs, im2col_compute, lambda c: ["tap_order_transposed", "border_wraps"]),
    "embed_splice": (splice_inputs, splice_compute, splice_mutants),
    "gather_rows": (gather_inputs, gather_compute, gather_mutants),
    "cosine": (cosine_inputs, cosine_compute, cosine_mutants),
    "align": (align_inputs, align_compute, align_mutants),
    "decode": (decode_inputs, decode_compute, decode_mutants),
    "pullback": (pullback_inputs, pullback_compute, pullback_mutants),
    "dice": (dice_inputs, dice_compute, dice_mutants),
}
EXACT_OPS = ("patchify", "im2col3x3", "embed_splice", "gather_rows")          # bit for bit: the bound is zero


@functools.lru_cache(maxsize=4)
def inp_cached(case):
    return OPS[case.op][0](case)


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> (inputs, fp64 reference outputs, per-element bounds); built once per case"""
    inp = inp_cached(case)
    ref, aux = OPS[case.op][1](case, inp)
    bounds = {}
    for n, r in ref.items():
        if case.op in EXACT_OPS:
            b = torch.zeros(())
        elif f"bound:{n}" in aux:
            b = aux[f"bound:{n}"]
        elif f"sum:{n}" in aux:
            b = f32_bound(*aux[f"sum:{n}"])
        else:
            w = aux.get(f"width:{n}")
            core = r if w is None else r[..., :w]
            b = torch.where(core == 0, torch.zeros_like(core), torch.nan_to_num(bf16_bound(core), nan=0.0))      # structural zeros and sentinels: exact
            if w is not None:
                b = torch.cat([b, torch.zeros_like(r[..., w:])], -1)
            if f"extra:{n}" in aux:
                b = b + aux[f"extra:{n}"]
            if f"exact:{n}" in aux:
                b = torch.where(aux[f"exact:{n}"], torch.zeros_like(b), b)
        bounds[n] = b
    return inp, ref, bounds


def ratios(got, refs, bounds):
    return {n: ratio(got[n], refs[n], bounds[n]) for n in refs}


def emulation_ratios(case):
    inp, ref, bounds = reference(case)
    got, _ = OPS[case.op][1](case, inp, emu=True)
    return ratios(got, ref, bounds)


def mutant_names(case):
    return list(OPS[case.op][2](case))


def mutant_ratios(case):
    """mutant -> its worst tolerance ratio over the outputs against the fp64 reference"""
    inp, ref, bounds = reference(case)
    out = {}
    for name in mutant_names(case):
        got, _ = OPS[case.op][1](case, inp, mut=name)
        out[name] = max(ratios(got, ref, bounds).values())
    return out
