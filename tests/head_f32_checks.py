"""The fp32-activation kernels of the inference head (llmseg_amd/csrc/head_f32.hip: llmseg_linear_f32, llmseg_layernorm_f32, llmseg_attn_f32, llmseg_cosine_f32),
the composed head (`_mask_head_f32`) and the inference tail (`_inference_scores_f32`): a case table at the tile and stride edges, input builders, fp64
references, LOCAL per-element tolerances, fp32 emulations of what each kernel rounds, and mutants (fp64 results of subtly wrong problems) that the
tolerances must reject.

Everything here runs on the CPU (no import of the HIP library).  tests/test_head_f32_cpu.py proves that the tolerance passes the emulations with a 2x
margin and rejects every applicable mutant by at least 2x on every case; tests/test_head_f32_gpu.py holds the kernels to the same rule.  Case, ratio,
f32_bound and its constant C_SUM are those of tests/backward_kernel_checks.py.  Weights and biases are bf16, activations fp32 values; the reference
takes exactly those values in fp64.

Outputs are compared over the whole buffer the call is handed: the slack of a strided output holds NaN in the reference (a sentinel that must stay).
Tolerances, per element (n = chain length, t_i = the fp64 terms of that element, f32_bound(n, s) = C_SUM 2^-24 sqrt(n) s):
  linear      pre = alpha sum_k x w + bias: B = f32_bound(n, sum |t_i|), n = K + (bias) + (residual), the bias among the terms;
              y = act(pre) + residual: slope(act) B + 2^-24 |act(pre)| (one rounding of the activation's result) + f32_bound(n, |residual|).
              slope = the activation's largest slope: 1 (ReLU), 1/4 (sigmoid), 1.0999 (SiLU, QuickGELU), 1.1290 (GELU)
  layernorm   d(mean) = f32_bound(D, sum |x|) / D; the centred variance moves by d(var) = f32_bound(D, sum d_i^2) / D + 2 d(mean) mean |d_i|, rstd by
              rstd^3 d(var) / 2 + 2^-23 rstd (the square root and the reciprocal); y = d_i rstd w + b moves by |w| (rstd d(mean) + |d_i| d(rstd)) +
              f32_bound(3, |d_i rstd w| + |b|).  A one-pass fp32 variance E[x^2] - mean^2 misses this bound on the offset row (x = 1000 + N(0, 1)) by
              more than MUT_MIN: the bound holds the kernel to its two-pass form
  attention   o = sum_j p_j v_j: numerator and denominator are fp32 sums over the Nk keys, f32_bound(Nk, sum_j p_j |v_j|) and |o| f32_bound(Nk, 1).  A
              score moves by d(s_j) = f32_bound(hd + 1, scale sum_d |q_d k_jd|) + 2^-24 |s_j - max| (its dot product; the rounding of the exponent's
              argument) and its weight by p_j d(s_j): + sum_j p_j d(s_j) |v_j| + |o| sum_j p_j d(s_j)
  cosine      the form of tests/forward_kernel_checks.py: f32_bound(D, sum_d |t_d e_d| / (|t| |e|)) with its C_COS
  composed    per OUTPUT (pred_iou, embedding; pred_similarity for the tail), measured from the reference alone: HEAD_MARGIN = 4 x the max-norm deviation of the
  head, tail  oracle run in fp32 from the oracle run in fp64 on that case.  4 x: the kernels' summation order is an independent draw of the same rounding
              process; over ~3e4 elements the maxima of two such draws rarely differ by 2 x, and a wrong head is wrong by 1e-2
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cases as ocases
from oracle import mask_head as ohead
from tests.backward_kernel_checks import C_SUM, EMU_MAX, MUT_MIN, Case, cdiv, f32_bound, ratio      # noqa: F401  (re-exported)
from tests.forward_kernel_checks import C_COS

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
NAN = float("nan")
JUNK = 7.0                      # what the slack of a strided INPUT holds (finite: a kernel that reads it is wrong, not NaN)
EPS24 = 2.0 ** -24
HEAD_MARGIN = 4.0
ACTS = {"none": 0, "relu": 1, "gelu": 2, "quickgelu": 3, "silu": 4, "sigmoid": 5}      # LLMSEG_ACT_*
SLOPE = {"none": 1.0, "relu": 1.0, "gelu": 1.1290, "quickgelu": 1.0999, "silu": 1.0999, "sigmoid": 0.25}      # the largest |slope| of each activation
LT, LK = 64, 16                 # linear_f32_kernel: output tile, K step
QWG, KSTAGE = 128, 64           # attn_f32_kernel: queries per workgroup, keys per LDS stage
LN_EPS = 1e-5


def _g(case):
    return torch.Generator().manual_seed(case.seed)


def _T(t, emu):
    return t.to(F32 if emu else F64)


def _fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in fp64, the sum is rounded once more than fmaf does (2^-53: never visible)"""
    return (a.double() * b.double() + c.double()).float()


def _pad(t, ld):
    """t [r, c] inside a NaN buffer [r, ld]"""
    out = torch.full((t.shape[0], ld), NAN, dtype=F64)
    out[:, :t.shape[1]] = t.to(F64)
    return out


def _junk(rows, cols, width, body):
    """body [rows, cols] inside a buffer [rows, width] whose slack is finite and varied"""
    out = (JUNK + 0.25 * torch.arange(width, dtype=F32)).repeat(rows, 1)
    out[:, :cols] = body
    return out


def _wave_sum(v):
    """the xor butterfly of wave_sum over the last dimension (64 lanes), in the tensor's dtype"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _lanes(t):
    """[..., D] -> [..., trips, 64]: element i belongs to lane i % 64, trip i // 64 (zero beyond D: a lane that skips a trip adds nothing)"""
    D = t.shape[-1]
    n = cdiv(D, 64)
    return F.pad(t, (0, n * 64 - D)).reshape(*t.shape[:-1], n, 64)


def _lane_fma_sum(a, b):
    """sum_i a_i b_i as the row kernels take it in fp32: an fmaf chain per lane over its trips, then the butterfly"""
    a, b = _lanes(a), _lanes(b)
    acc = torch.zeros_like(a[..., 0, :])
    for i in range(a.shape[-2]):
        acc = _fma(a[..., i, :], b[..., i, :], acc)
    return _wave_sum(acc)


# ----------------------------------------------------------------------------------------------------------------- the case table
def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))

    def lin(name, M, N, K, kn=0, act="none", bias=1, res=0, alpha=1.0, ldx=0, wslice="", ldr=0, ldy=0, wide=0):
        add("linear", name, 1, M=M, N=N, K=K, kn=kn, act=act, bias=bias, res=res, alpha=alpha, ldx=ldx, wslice=wslice, ldr=ldr, ldy=ldy, wide=wide)
    # ---- linear_f32: 64 x 64 tile, 4 x 4 outputs per thread, K step 16, two W loaders.  M, N over 1, 63, 64, 65, 130; K over 1, 15, 16, 17, 50; both layouts
    for M, N, K, kn, bias, res in ((1, 1, 1, 0, 1, 0), (1, 63, 15, 1, 0, 0), (63, 64, 16, 0, 1, 0), (64, 65, 17, 1, 1, 0), (65, 130, 50, 0, 1, 1), (130, 1, 50, 1, 0, 0),
                                   (64, 64, 64, 0, 0, 0), (65, 50, 50, 1, 1, 0), (130, 63, 1, 0, 0, 1), (63, 130, 15, 1, 1, 0), (1, 64, 17, 0, 1, 1), (130, 65, 16, 1, 0, 1)):
        lin(f"{M}x{N}x{K}_{'kn' if kn else 'nk'}{'_bias' if bias else ''}{'_res' if res else ''}", M, N, K, kn=kn, bias=bias, res=res)
    # every activation at 33 x 65 x 17, pre-activations over about +/-12 (sigmoid and SiLU saturate, the GELU tail); a residual behind three of them
    for i, act in enumerate(ACTS):
        lin(f"33x65x17_{act}{'_kn' if i % 2 else ''}{'_res' if i % 2 == 0 else ''}", 33, 65, 17, kn=i % 2, act=act, res=int(i % 2 == 0), wide=1)
    lin("33x65x17_alpha_bias_res_relu", 33, 65, 17, act="relu", res=1, alpha=0.5, wide=1)
    lin("33x65x17_alpha_bias_res_kn", 33, 65, 17, kn=1, res=1, alpha=0.5)
    # leading dimensions: each alone, then all at once in each layout
    lin("33x65x17_ldx", 33, 65, 17, ldx=5)
    lin("33x65x17_ldr", 33, 65, 17, res=1, ldr=3)
    lin("33x65x17_ldy", 33, 65, 17, kn=1, ldy=3)
    for kn in (0, 1):
        for ws in ("row", "col"):
            lin(f"33x65x17_ldw_{ws}slice_{'kn' if kn else 'nk'}", 33, 65, 17, kn=kn, wslice=ws)
    lin("33x65x17_ld_all_nk", 33, 65, 17, res=1, ldx=5, wslice="col", ldr=3, ldy=3)
    lin("33x65x17_ld_all_kn", 33, 65, 17, kn=1, res=1, ldx=5, wslice="row", ldr=3, ldy=3)
    # the head's own chains at reduced M
    lin("head_text_fc_3x256x4096_relu", 3, 256, 4096, act="relu")
    lin("head_qkv_130x768x256", 130, 768, 256)
    lin("head_mlp1_130x2048x256_relu", 130, 2048, 256, act="relu")
    lin("head_mlp2_130x256x2048_res", 130, 256, 2048, res=1)
    lin("head_pool_20x256x4096_kn", 20, 256, 4096, kn=1, bias=0)
    # ---- layernorm_f32: one wave per row, four rows per workgroup
    for rows, D, bias, kind in ((1, 1, 1, ""), (3, 8, 0, ""), (4, 63, 1, ""), (5, 64, 0, ""), (130, 65, 1, ""), (3, 100, 1, ""), (5, 256, 1, ""), (1, 256, 0, ""),
                                (4, 100, 1, "const"), (5, 256, 0, "const"), (5, 256, 1, "offset")):
        add("layernorm", f"{rows}x{D}{'_bias' if bias else ''}{'_' + kind if kind else ''}", 1, rows=rows, D=D, bias=bias, kind=kind)
    # ---- attn_f32: 128 queries per workgroup, 64-key LDS stages, head_dim 32 and 64
    def att(name, B, H, Nq, Nk, hd, layout, scale=0.0, ldo=0, peak=""):
        add("attn", name, 1, B=B, H=H, Nq=Nq, Nk=Nk, hd=hd, layout=layout, scale=scale, ldo=ldo, peak=peak)
    att("B1_H1_q1_k1_hd32", 1, 1, 1, 1, 32, "kv")
    att("B2_H8_q1_k65_hd32_cross", 2, 8, 1, 65, 32, "kv")                  # the head's cross-attention: q [C, D], k | v packed in [C * K, 2 D]
    att("B3_H8_q130_k130_hd32_self", 3, 8, 130, 130, 32, "qkv")            # the head's self-attention: q | k | v in [C * K, 3 D]
    att("B1_H2_q127_k63_hd64", 1, 2, 127, 63, 64, "kv")
    att("B1_H2_q128_k64_hd64", 1, 2, 128, 64, 64, "kv")
    att("B2_H2_q129_k65_hd64", 2, 2, 129, 65, 64, "kv")
    att("B1_H8_q64_k130_hd32_scale_ldo", 1, 8, 64, 130, 32, "kv", scale=0.3, ldo=8)
    att("B1_H2_q5_k130_hd32_peak_last", 1, 2, 5, 130, 32, "kv", peak="last")      # logits over about +/-90: the running maximum moves at every key
    att("B1_H2_q5_k130_hd32_peak_first", 1, 2, 5, 130, 32, "kv", peak="first")    # ... and never after the first
    # ---- cosine_f32: one wave per row of e
    for K, D in ((1, 1), (3, 63), (4, 64), (5, 65), (130, 256)):
        add("cosine", f"K{K}_D{D}", 1, K=K, D=D)
    return out


# --------------------------------------------------------------------------------------------------------------------------- linear
def weight_view(case, inp):
    """the [rows, cols] view of the weight the kernel is handed, inside the buffer inp['wbuf'] (a row or a column slice of a wider weight, or all of it)"""
    r0, c0, R, Cc = inp["wsl"]
    return inp["wbuf"][r0:r0 + R, c0:c0 + Cc]


def linear_inputs(case):
    g = _g(case)
    M, N, K = case.M, case.N, case.K
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * (1.0 if case.wide else K ** -0.5)      # wide: pre-activations of sigma sqrt(17): about +/-12 over the 2145 outputs
    stored = (w.t() if case.kn else w).contiguous().to(BF)                       # [K, N] when w_kn, else [N, K]
    R, Cc = stored.shape
    if case.wslice:
        wbuf = (torch.randn(R + 2, Cc + 6, generator=g) * 3.0).to(BF)            # the rest of the wider weight: large, finite
        r0, c0 = (2, 0) if case.wslice == "row" else (0, 6)
        wbuf[r0:r0 + R, c0:c0 + Cc] = stored
    else:
        wbuf, r0, c0 = stored, 0, 0
    bias = torch.randn(N, generator=g).to(BF) if case.bias else None
    res = _junk(M, N, N + case.ldr, torch.randn(M, N, generator=g)) if case.res else None
    return dict(x=_junk(M, K, K + case.ldx, x), wbuf=wbuf, wsl=(r0, c0, R, Cc), bias=bias, res=res, ldy=N + case.ldy, alpha=case.alpha)


def act_apply(v, act, mut=None):
    """the activation in the dtype of v (fp32: every operation rounds once, exp and erf as accurate fp32 functions)"""
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-v))
    if act == "silu":
        return v / (1.0 + torch.exp(-v))
    if act == "quickgelu":
        c = 1.0 if mut == "quickgelu_constant_1" else (float(np.float32(1.702)) if v.dtype == F32 else 1.702)
        return v / (1.0 + torch.exp(-c * v))
    if act == "gelu":
        if mut == "tanh_gelu":
            return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))
        return 0.5 * v * (1.0 + torch.erf(v * (float(np.float32(0.70710678118654752)) if v.dtype == F32 else 0.7071067811865476)))
    return v


def linear_compute(case, inp, mut=None, emu=None):
    M, N, K = case.M, case.N, case.K
    xb = inp["x"]
    x = _T(xb.reshape(-1)[:M * K].view(M, K) if mut == "ldx_taken_as_K" else xb[:, :K], emu)
    w = _T(weight_view(case, inp), emu)
    wkn = w if case.kn else w.t()                                          # [K, N]
    if mut == "layout_swapped":
        wkn = wkn.t()
    Kk = K // LK * LK if mut == "k_tail_dropped" else K
    alpha = float(np.float32(inp["alpha"]))
    b = _T(inp["bias"], emu)[None, :] if inp["bias"] is not None else None
    if b is not None and mut == "bias_indexed_by_row":
        b = b[0][torch.arange(M) % N][:, None]
    if emu:                                                                # per K step of 16 one fmaf chain in ascending k, the steps' sums added in order, then fmaf(acc, alpha, bias)
        acc = torch.zeros(M, N, dtype=F32)
        for k0 in range(0, Kk, LK):
            part = torch.zeros(M, N, dtype=F32)
            for k in range(k0, min(k0 + LK, Kk)):
                part = _fma(x[:, k:k + 1], wkn[k:k + 1], part)
            acc = acc + part
        pre = _fma(acc, torch.tensor(alpha, dtype=F32), b if b is not None else torch.zeros((), dtype=F32))
    else:
        s = x[:, :Kk] @ wkn[:Kk]
        pre = alpha * (s + b) if (mut == "alpha_on_bias" and b is not None) else alpha * s + (b if b is not None else 0.0)
    r = None
    if inp["res"] is not None:
        rb = inp["res"]
        r = _T(rb.reshape(-1)[:M * N].view(M, N) if mut == "ldr_taken_as_N" else rb[:, :N], emu)
    if r is not None and mut == "residual_before_act":
        y = act_apply(pre + r, case.act, mut)
    else:
        y = act_apply(pre, case.act, mut)
        if r is not None:
            y = y + r
    out = _pad(y, inp["ldy"])
    if mut == "last_row_dropped":
        out[M - 1, :N] = NAN
    if mut == "last_col_dropped":
        out[:, N - 1] = NAN
    aux = {}
    if not emu and mut is None:
        n = K + int(b is not None) + int(r is not None)
        sabs = abs(alpha) * (x.abs() @ wkn.abs()) + (b.abs() if b is not None else 0.0)
        bound = SLOPE[case.act] * f32_bound(n, sabs)
        if case.act != "none":
            bound = bound + EPS24 * act_apply(pre, case.act).abs()
        if r is not None:
            bound = bound + f32_bound(n, r.abs())
        aux["bound:y"] = torch.cat([bound, torch.zeros(M, inp["ldy"] - N, dtype=F64)], 1)
    return {"y": out}, aux


def linear_mutants(case):
    m = ["last_row_dropped", "last_col_dropped"]
    if case.K % LK:
        m.append("k_tail_dropped")
    if case.bias and case.alpha != 1.0:
        m.append("alpha_on_bias")
    if case.res and case.act != "none":
        m.append("residual_before_act")
    if case.bias and case.M > 1:
        m.append("bias_indexed_by_row")
    if case.N == case.K and case.N > 1:
        m.append("layout_swapped")
    if case.ldx and case.M > 1:
        m.append("ldx_taken_as_K")
    if case.res and case.ldr and case.M > 1:
        m.append("ldr_taken_as_N")
    if case.act == "gelu":
        m.append("tanh_gelu")
    if case.act == "quickgelu":
        m.append("quickgelu_constant_1")
    return m


# ------------------------------------------------------------------------------------------------------------------------ layernorm
CONST_ROW, CONST_VALUE = 1, 0.75          # the constant row of a "const" case: every partial sum of 0.75 is exact in fp32, so mean = 0.75 and the variance is exactly 0


def layernorm_inputs(case):
    g = _g(case)
    r, D = case.rows, case.D
    z = torch.randn(r, D, generator=g)
    if case.kind == "offset":
        x = 1000.0 + z
    else:
        off = torch.randn(r, 1, generator=g)
        off = torch.sign(off) * (0.7 + 0.5 * off.abs())                   # a mean of the order of the row's sigma on every row
        x = 0.005 * (z + off)                                             # small x: eps = 1e-5 is ~40 % of the variance
    if case.kind == "const":
        x[CONST_ROW] = CONST_VALUE
    w = (1.0 + 0.5 * torch.randn(D, generator=g)).to(BF)
    b = (0.5 * torch.randn(D, generator=g)).to(BF) if case.bias else None
    return dict(x=x.contiguous(), w=w, b=b, eps=LN_EPS)


def layernorm_compute(case, inp, mut=None, emu=None):
    r, D = case.rows, case.D
    x, w = _T(inp["x"], emu), _T(inp["w"], emu)
    b = _T(inp["b"], emu) if (inp["b"] is not None and mut != "bias_dropped") else None
    eps = 0.0 if mut == "eps_dropped" else float(np.float32(inp["eps"]))
    Dk = D // 64 * 64 if mut == "last_lane_group_dropped" else D
    aux = {}
    if emu:                                    # two passes; per lane a chain over its trips, then the butterfly.  emu == "one_pass": E[x^2] - mean^2 (NOT the kernel)
        ones = torch.ones_like(x)
        mean = _lane_fma_sum(x, ones) / torch.tensor(float(D), dtype=F32)
        if emu == "one_pass":
            var = _lane_fma_sum(x, x) / torch.tensor(float(D), dtype=F32) - mean * mean
        else:
            d = x - mean[:, None]
            var = _lane_fma_sum(d, d) / torch.tensor(float(D), dtype=F32)
        rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
        u = (x - mean[:, None]) * rstd[:, None]
        y = _fma(u, w[None], b[None] if b is not None else torch.zeros((), dtype=F32))
    else:
        xs = x[:, :Dk]
        mean = xs.sum(-1, keepdim=True) / max(Dk, 1)
        d = x - mean
        var = (d[:, :Dk] ** 2).sum(-1, keepdim=True) / ((Dk - 1) if mut == "unbiased_variance" else max(Dk, 1)) if Dk else torch.full((r, 1), NAN, dtype=F64)
        rstd = (var + eps).rsqrt()
        y = d * rstd * w
        if b is not None:
            y = y + b
        if mut is None:
            d_mean = f32_bound(D, x.abs().sum(-1, keepdim=True)) / D
            d_var = f32_bound(D, (d * d).sum(-1, keepdim=True)) / D + 2.0 * d_mean * d.abs().mean(-1, keepdim=True)
            d_rstd = 0.5 * rstd ** 3 * d_var + 2.0 * EPS24 * rstd
            aux["bound:y"] = w.abs() * (rstd * d_mean + d.abs() * d_rstd) + f32_bound(3, (d * rstd * w).abs() + (b.abs() if b is not None else 0.0))
    y = y.to(F64).clone()
    if mut == "last_lane_group_dropped":
        y[:, Dk:] = NAN
    if mut == "last_row_dropped":
        y[r - 1] = NAN
    return {"y": y}, aux


def layernorm_mutants(case):
    m = ["last_row_dropped"]
    if case.kind != "offset":                  # x = 1000 + N(0, 1): eps = 1e-5 is 1e-5 of the variance, and the 0.2 % of D / (D - 1) on y <= 3 is what d(mean) =
        m += ["eps_dropped", "unbiased_variance"]      # f32_bound(256, 256000) / 256 = 2.9e-3 allows (0.66 of the bound); the one-pass emulation is what this row is for
    if case.D % 64:
        m.append("last_lane_group_dropped")
    if case.bias:
        m.append("bias_dropped")
    return m


# ------------------------------------------------------------------------------------------------------------------------ attention
PEAK = 90.0


def attn_scale(case):
    return float(np.float32(case.scale if case.scale else 1.0 / math.sqrt(case.hd)))


def attn_inputs(case):
    """q [B, H, Nq, hd], k and v [B, H, Nk, hd], fp32"""
    g = _g(case)
    B, H, Nq, Nk, hd = case.B, case.H, case.Nq, case.Nk, case.hd
    q = torch.randn(B, H, Nq, hd, generator=g)
    k = torch.randn(B, H, Nk, hd, generator=g)
    v = torch.randn(B, H, Nk, hd, generator=g)
    if case.peak:                              # scores f_i * ramp_j + noise: ramp over -90 .. 90 (ascending: the last key is the maximum), f_i over 0.96 .. 1
        u = torch.randn(B, H, 1, hd, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        ramp = torch.linspace(-PEAK, PEAK, Nk)
        if case.peak == "first":
            ramp = ramp.flip(0)
        q = u * (1.0 - 0.01 * torch.arange(Nq, dtype=F32))[None, None, :, None] + 0.02 * q
        k = u * (ramp / attn_scale(case))[None, None, :, None] + 0.5 * k
    return dict(q=q, k=k, v=v)


def attn_rows(t):
    """[B, H, n, hd] -> rows [B * n, H * hd]"""
    B, H, n, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * n, H * hd)


def attn_buffers(case, inp, device="cpu", out=None):
    """the operands as the head lays them out -> (q, k, v views, o view, the four (batch, head, row) stride triples).  layout "qkv": q | k | v packed in
    [B * N, 3 D]; "kv": q [B * Nq, D], k | v packed in [B * Nk, 2 D]; o [B * Nq, ldo] (`out`, or a fresh NaN buffer)"""
    B, H, Nq, Nk, hd = case.B, case.H, case.Nq, case.Nk, case.hd
    D = H * hd
    ldo = D + case.ldo
    qr, kr, vr = (attn_rows(inp[n]).to(device) for n in ("q", "k", "v"))
    if case.layout == "qkv":
        buf = torch.cat([qr, kr, vr], 1).contiguous()
        q, k, v = buf, buf[:, D:], buf[:, 2 * D:]
        qs = ks = vs = (Nq * 3 * D, hd, 3 * D)
    else:
        q = qr.contiguous()
        buf = torch.cat([kr, vr], 1).contiguous()
        k, v = buf, buf[:, D:]
        qs, ks = (Nq * D, hd, D), (Nk * 2 * D, hd, 2 * D)
        vs = ks
    o = torch.full((B * Nq, ldo), NAN, dtype=F32, device=device) if out is None else out
    return q, k, v, o, (qs, ks, vs, (Nq * ldo, hd, ldo))


def attn_compute(case, inp, mut=None, emu=None):
    B, H, Nq, Nk, hd = case.B, case.H, case.Nq, case.Nk, case.hd
    q, k, v = (_T(inp[n], emu) for n in ("q", "k", "v"))
    scale = 1.0 if mut == "scale_missing" else attn_scale(case)
    if mut == "batch_reads_batch0_keys":
        k, v = k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1)
    if mut == "heads_permuted":
        k, v = k.flip(1), v.flip(1)
    if mut == "v_read_from_k_columns":
        v = k
    if mut == "last_key_dropped":
        k, v = k[:, :, :Nk - 1], v[:, :, :Nk - 1]
    if mut == "last_stage_dropped":
        keep = (Nk - 1) // KSTAGE * KSTAGE
        k, v = k[:, :, :keep], v[:, :, :keep]
    if mut == "stage_padding_counted":
        pad = (0, 0, 0, cdiv(Nk, KSTAGE) * KSTAGE - Nk)
        k, v = F.pad(k, pad), F.pad(v, pad)
    nk = k.shape[2]
    aux = {}
    if emu:
        qs = q * torch.tensor(scale, dtype=F32)
        s = torch.zeros(B, H, Nq, nk, dtype=F32)
        for d in range(hd):                    # one fmaf chain over d per (query, key)
            s = _fma(qs[..., d:d + 1], k[..., d].unsqueeze(2), s)
        if emu == "no_max":                    # NOT the kernel: exp(s) without the running maximum
            p = torch.exp(s)
            o = (p @ v) / p.sum(-1, keepdim=True)
        else:                                  # online softmax, one key after the other
            mx = torch.full((B, H, Nq, 1), -float("inf"), dtype=F32)
            l = torch.zeros(B, H, Nq, 1, dtype=F32)
            acc = torch.zeros(B, H, Nq, hd, dtype=F32)
            for j in range(nk):
                sj = s[..., j:j + 1]
                mn = torch.maximum(mx, sj)
                corr, p = torch.exp(mx - mn), torch.exp(sj - mn)
                l = l * corr + p
                acc = _fma(acc, corr, p * v[:, :, j:j + 1])
                mx = mn
            o = acc * (1.0 / l)
    elif nk == 0:
        o = torch.full((B, H, Nq, hd), NAN, dtype=F64)
    else:
        s = (q @ k.transpose(-1, -2)) * scale
        m = s.amax(-1, keepdim=True)
        p = torch.softmax(s, -1)
        o = p @ v
        if mut is None:
            ds = f32_bound(hd + 1, (q.abs() @ k.abs().transpose(-1, -2)) * scale) + EPS24 * (s - m).abs()
            pd = p * ds
            aux["bound:o"] = f32_bound(Nk, p @ v.abs()) + pd @ v.abs() + o.abs() * (f32_bound(Nk, torch.ones(())) + pd.sum(-1, keepdim=True))
    D = H * hd
    out = {"o": _pad(attn_rows(o.to(F64)), D + case.ldo)}
    if "bound:o" in aux:
        aux["bound:o"] = torch.cat([attn_rows(aux["bound:o"]), torch.zeros(B * Nq, case.ldo, dtype=F64)], 1)
    return out, aux


def attn_mutants(case):
    m = ["v_read_from_k_columns"]
    if case.peak != "first":                   # the first key is the maximum: the last ones weigh e^-180
        m.append("last_key_dropped")
        if case.Nk > KSTAGE:
            m.append("last_stage_dropped")
    if case.Nk % KSTAGE and not case.peak:     # a maximum of 90: a key of score 0 weighs e^-90
        m.append("stage_padding_counted")
    if case.Nk > 1:                            # one key: the softmax is 1 whatever the scale
        m.append("scale_missing")
    if case.B > 1:
        m.append("batch_reads_batch0_keys")
    if case.H > 1:
        m.append("heads_permuted")
    return m


# --------------------------------------------------------------------------------------------------------------------------- cosine
def cosine_rows(case):
    """-> (row equal to t, row equal to -t, all-zero row) or None where K has no room"""
    K = case.K
    return (0 if K >= 3 else None, 1 if K >= 3 else None, 2 if K >= 4 else None)


def cosine_inputs(case):
    g = _g(case)
    t = torch.randn(case.D, generator=g) + 0.3
    e = torch.randn(case.K, case.D, generator=g) * (torch.rand(case.K, 1, generator=g) * 4 + 0.1) + 0.3
    same, opp, zero = cosine_rows(case)
    if same is not None:
        e[same], e[opp] = t, -t
    if zero is not None:
        e[zero] = 0.0
    return dict(t=t.contiguous(), e=e.contiguous())


def cosine_compute(case, inp, mut=None, emu=None):
    t, e = _T(inp["t"], emu), _T(inp["e"], emu)
    if mut == "last_lane_group_dropped":               # the columns beyond the last multiple of 64
        t, e = t[:case.D // 64 * 64], e[:, :case.D // 64 * 64]
    if emu:
        tb = t[None].expand_as(e)
        sim = _lane_fma_sum(tb, e) / (torch.sqrt(_lane_fma_sum(tb, tb)) * torch.sqrt(_lane_fma_sum(e, e)))
    else:
        dot, ne, nt = (e * t).sum(-1), (e * e).sum(-1).sqrt(), (t * t).sum().sqrt()
        sim = dot / (ne * (1.0 if mut == "target_norm_missing" else nt))      # an all-zero row: 0 / 0 = NaN, as the reference's x / x.norm() gives
    sim = sim.to(F64).clone()
    if mut == "last_row_dropped":
        sim[-1] = NAN
    aux = {"bound:sim": f32_bound(case.D, (e * t).abs().sum(-1) / (ne * nt), c=C_COS)} if not emu and mut is None else {}
    return {"sim": sim}, aux


def cosine_mutants(case):
    return ["target_norm_missing", "last_row_dropped"] + (["last_lane_group_dropped"] if case.D % 64 else [])      # D < 64: nothing is left, 0 / 0


# ----------------------------------------------------------------------------------------------------------------------- registry
OPS = {
    "linear": (linear_inputs, linear_compute, linear_mutants),
    "layernorm": (layernorm_inputs, layernorm_compute, layernorm_mutants),
    "attn": (attn_inputs, attn_compute, attn_mutants),
    "cosine": (cosine_inputs, cosine_compute, cosine_mutants),
}


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> (inputs, fp64 reference outputs, per-element bounds); built once per case"""
    inp = OPS[case.op][0](case)
    ref, aux = OPS[case.op][1](case, inp)
    return inp, ref, {n: aux[f"bound:{n}"] for n in ref}


def ratios(got, refs, bounds):
    return {n: ratio(got[n], refs[n], bounds[n]) for n in refs}


def emulation_ratios(case, emu=True):
    inp, ref, bounds = reference(case)
    got, _ = OPS[case.op][1](case, inp, emu=emu)
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


# --------------------------------------------------------------------------------------------------------------- the composed head
HEAD_CASES = ((1, 1), (1, 65), (3, 130), (2, 64))          # (conversations C, proposals K)
HEAD_MUTANTS = ("text_of_conversation_0", "last_proposal_missing_from_self_attention_keys", "post_attention_layernorm_skipped")
PFX = "model."


def head_weights(sd):
    """the head's tensors of a state dict, rounded to bf16 (as fp32 values)"""
    return {k: v.to(BF).float() for k, v in sd.items() if ".lisa_" in k and "dino_conv" not in k}


@functools.lru_cache(maxsize=None)
def head_inputs(C, K):
    """seeded head weights, pooled [K, D] and text [C, D], all rounded to bf16 (fp32 values)"""
    sd, pooled, text = ocases.head_case(C=C, K=K)
    return head_weights(sd), pooled.to(BF).float(), text.to(BF).float()


def head_oracle(sd, pooled, text, dtype, mut=None, restated=False):
    """oracle.mask_head.mask_head in `dtype` -> (pred_iou [C, K], embedding [C, K, D]); mut: one of HEAD_MUTANTS, a subtly wrong head, computed by a restatement
    of the oracle's wiring (restated = True without a mutant: that restatement itself, which must give the oracle's bits)"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    s, t = pooled.to(dtype), text.to(dtype)
    with torch.no_grad():
        if mut is None and not restated:
            iou, emb = ohead.mask_head(sd, PFX, s, t)
            return iou[..., 0], emb
        C = t.shape[0]
        if mut == "text_of_conversation_0":
            t = t[:1].expand(C, -1)
        t, s = t.unsqueeze(1), s.unsqueeze(0).expand(C, -1, -1)
        ln, att = ohead._ln, ohead.mh_attention
        for i in range(2):                                 # oracle.mask_head.two_way_block, with the two defects
            p = f"{PFX}lisa_attention_layers.{i}."
            keys = s[:, :-1] if mut == "last_proposal_missing_from_self_attention_keys" else s
            a = s + att(sd, p + "self_attn.", s, keys, keys)
            s = a if (mut == "post_attention_layernorm_skipped" and i == 0) else ln(sd, p + "norm1", a)
            s = ln(sd, p + "norm2", s + att(sd, p + "cross_attn_token_to_image.", s, t, t))
            s = ln(sd, p + "norm3", s + ohead._lin(sd, p + "mlp.lin2", F.relu(ohead._lin(sd, p + "mlp.lin1", s))))
            t = ln(sd, p + "norm4", t + att(sd, p + "cross_attn_image_to_token.", t, s, s))
        s = ln(sd, PFX + "lisa_norm_final_attn", s + att(sd, PFX + "lisa_final_attn.", s, t, t))
        iou = torch.sigmoid(ohead._lin(sd, PFX + "lisa_iou_head.2", F.relu(ohead._lin(sd, PFX + "lisa_iou_head.0", s))))
        emb = ohead._lin(sd, PFX + "lisa_embedding_head.2", F.relu(ohead._lin(sd, PFX + "lisa_embedding_head.0", s)))
        return iou[..., 0], emb


def head_mutant_names(C, K):
    return [m for m in HEAD_MUTANTS if not (m == "text_of_conversation_0" and C == 1) and not (m.startswith("last_proposal") and K == 1)]


def dev_bound(ref, f32):
    """per output: (the max-norm deviation of the fp32 oracle from the fp64 one, HEAD_MARGIN x that)"""
    dev = {n: float((f32[n].to(F64) - ref[n]).abs().max()) for n in ref}
    return dev, {n: HEAD_MARGIN * d for n, d in dev.items()}


@functools.lru_cache(maxsize=None)
def head_reference(C, K):
    """-> (fp64 reference {iou, emb}, fp32-oracle deviation per output, bound per output)"""
    sd, pooled, text = head_inputs(C, K)
    ref = dict(zip(("iou", "emb"), head_oracle(sd, pooled, text, F64)))
    f32 = dict(zip(("iou", "emb"), head_oracle(sd, pooled, text, F32)))
    dev, bound = dev_bound(ref, f32)
    return ref, dev, bound


def head_ratios(got, ref, bound):
    """per output: max |got - ref| / bound (NaN -> inf)"""
    out = {}
    for n in ref:
        d = (got[n].to(F64).reshape(ref[n].shape) - ref[n]).abs()
        out[n] = float("inf") if bool(torch.isnan(d).any()) else float(d.max()) / bound[n]
    return out


# --------------------------------------------------------------------------------------------------------------- the inference tail
TAIL_K, TAIL_ZERO = 67, 5       # proposals of the tail case (no multiple of 64) and the one that is all zero


def tail_batch(cfg):
    """one image of the tiny batch with its C = 2 conversations and TAIL_K seeded proposals, proposal TAIL_ZERO empty; floating-point inputs rounded to bf16"""
    b = ocases.tiny_lisa_batch(img_size=cfg.sam.img)
    segs = (ocases.seeded.uniform((TAIL_K, 256, 256), 91) > 0.4).float()
    segs[TAIL_ZERO] = 0.0
    r = lambda t: t.to(BF).float()
    return dict(images=r(b["images"][:1]), images_clip=r(b["images_clip"][:1]), input_ids=b["input_ids"][:2], labels=None, attention_masks=b["attention_masks"][:2],
                offset=torch.tensor([0, 2]), sam_segs_list=[segs])


def seg_rows(input_ids, T, seg_token):
    """flat indices into hidden [N * T, H] of the rows that predict a [SEG] token: the mask shifted by one and by the P - 1 extra image tokens"""
    N, L = input_ids.shape
    P = T - L + 1
    segm = torch.zeros((N, T), dtype=torch.bool)
    segm[:, P - 1:P - 1 + L - 1] = input_ids[:, 1:] == seg_token
    return segm.view(-1).nonzero().flatten()


def tail_oracle(sd, feats_cl, hidden, input_ids, segs, seg_token, dtype):
    """The inference tail of one image, restated from the two trunk outputs on: feats_cl [g * g, D] (channels-last rows) and hidden [N, T, H] as the trunk
    returned them (bf16 values), segs [K, S, S], sd the model's weights (bf16 values).  [SEG] rows -> text_hidden_fcs -> bilinear upsampling -> mask
    pooling with the + 1e-8 -> the oracle head -> cosine scores.  -> {pred_similarity [C, K], pred_iou [1, K], pooled [K, D], pred_embeddings [C, D]}"""
    w = lambda n: sd[n].to(dtype)
    N, T, H = hidden.shape
    with torch.no_grad():
        hs = hidden.reshape(N * T, H)[seg_rows(input_ids, T, seg_token)].to(dtype)
        hs = F.relu(F.linear(hs, w("model.text_hidden_fcs.0.0.weight"), w("model.text_hidden_fcs.0.0.bias")))
        pred = F.linear(hs, w("model.text_hidden_fcs.0.2.weight"), w("model.text_hidden_fcs.0.2.bias"))
        g = int(round(math.sqrt(feats_cl.shape[0])))
        S = segs.shape[-1]
        chw = feats_cl.to(dtype).t().reshape(1, -1, g, g)
        up = F.interpolate(chw, size=(S, S), mode="bilinear", align_corners=False)[0]
        pooled = ohead.mask_pooling(up, segs.to(dtype))
        iou, emb = head_oracle(head_weights(sd), pooled, pred, dtype)
        sim = torch.cat([ohead.cosine_scores(pred[c:c + 1], emb[0]) for c in range(pred.shape[0])], 0)
    return {"pred_similarity": sim, "pred_iou": iou[:1], "pooled": pooled, "pred_embeddings": pred}
