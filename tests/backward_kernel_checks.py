"""Backward, LoRA and optimizer kernels (llmseg_amd/csrc/backward.hip and lora.hip, the CE forward of head.hip) on every dispatch route: a case table,
input builders, fp64 references, LOCAL tolerances, fp32 / bf16 emulations of what the kernels round, and mutants (fp64 results of subtly
wrong problems) that the tolerances must reject.

Everything here runs on the CPU (no import of the HIP library).  tests/test_backward_kernels_cpu.py proves that the tolerance passes the
emulations with a 2x margin and rejects every applicable mutant by at least 2x on every case; tests/test_backward_kernels_gpu.py holds the
kernels to the same rule through llmseg_amd.ops.

A case names the entry point (`op`), its shapes (`p`), the workspace mode (`ws`: "full", "none" or a byte count that cuts the slice count)
and the number of library launches the call must make (`launches`, read off llmseg_launch_count() on the GPU; derived from the dispatch code
and cross-checked here against `route(case)`, a restatement of that dispatch).

Two tolerance forms, both per element:
  bf16 outputs:  |got - ref| <= C_BF16 * 2^-8 * (|ref| + sigma_row)           sigma_row = RMS of that row of the reference; a row whose reference
                                                                             is exactly zero must be exactly zero
  fp32 sums:     |got - ref| <= C_SUM * 2^-24 * sqrt(n) * sum_i |t_i|         n terms t_i (fp64) of that output element, the existing content of a
                                                                             `+=` output included (C_ELEM for AdamW's element-wise master / m / v)
Wherever the reference of a bf16 output is exactly zero (ignored CE rows, zero_cols, padding columns, masked and causal entries of P and dS) the bound is
zero: bit for bit.  So is every element of transpose_pad and lora_pack.  NaN in a reference marks sentinel rows that must stay NaN.
"""
import functools
import math

import numpy as np
import torch

from oracle import dropout as odrop

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
INF = float("inf")

C_BF16 = 2.0                  # half an ulp of bf16 is up to 2^-8 |ref|: a correctly rounded store of an exact value reaches 1 / C_BF16 where |ref| >> sigma_row
C_SUM = 3.0                   # fp32 sums (the reductions): smallest integer for which every emulation stays <= EMU_MAX (the worst, 0.42: lora_wgrads at 5 x 72,
                              # few terms, each carrying the dropout scale's and alpha's roundings)
C_ELEM = 7.0                  # AdamW's element-wise fp32 outputs (master, m, v), same form with n = 2 or 3: the worst emulation, 0.45, is the master weight where
                              # |w| << |lr * update| -- the update carries ~10 fp32 roundings (m, v, two divisions, a square root) and the table draws 6 M elements
EMU_MAX = 0.5                 # the emulations must stay at <= half the bound
MUT_MIN = 2.0                 # every applicable mutant must exceed the bound by >= 2x
REDUCE_WS_BYTES = 16 << 20    # llmseg_amd.ops.REDUCE_WS_BYTES (what ws = "full" hands over)
FILL = 0.375                  # what `+=` outputs are pre-filled with (exact in bf16 and fp32)
SEED, OFFSET, STREAM, P_DROP = 0x1234567, 11, 5, 0.05


class Case:
    def __init__(self, op, name, launches, ws="full", einval=None, **p):
        self.op, self.name, self.launches, self.ws, self.einval, self.p = op, f"{op}-{name}", launches, ws, einval, p

    def __repr__(self):
        return self.name

    def __eq__(self, o):
        return isinstance(o, Case) and self.name == o.name

    def __hash__(self):
        return hash(self.name)

    def __getattr__(self, k):
        try:
            return self.__dict__["p"][k]
        except KeyError:
            raise AttributeError(k)

    @property
    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) % 100003

    @property
    def ws_bytes(self):
        return REDUCE_WS_BYTES if self.ws == "full" else 0 if self.ws == "none" else int(self.ws)


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ the dispatch, restated (slices, launches)
def colsum_slices(M, N, ws):
    colwg = cdiv(N, 64)
    gy = min(64, max(1, min(cdiv(M, 32), cdiv(256, colwg))))
    return max(1, min(gy, ws // (N * 4)))


def norm_route(rows, cols, wgrad, ws):
    """-> (route, partial count, launches)"""
    cpl = cdiv(cols // 8, 64)
    if not wgrad and rows >= 64 and 2048 <= cols <= 8192:
        cpt = cdiv(cols // 8, 256)
        return f"wg_cpt{1 if cpt <= 1 else 2 if cpt <= 2 else 4}", 1, 1
    if not wgrad:
        return f"wave_cpl{1 if cpl <= 1 else 2 if cpl <= 2 else 4 if cpl <= 4 else 8 if cpl <= 8 else 0}", 1, 1
    wsf = ws // 4
    if cpl <= 2:
        G = min(min(max(1, cdiv(rows, 32)), 256), wsf // (2 * cols))
        G = G if G > 1 else 1
        return f"acc_cpl{1 if cpl <= 1 else 2}", G, 2 if G > 1 else 1
    if wsf < 2 * rows + 2 * cols:
        return "einval", 0, 0
    off = cdiv(2 * rows, 64) * 64
    gy = min(min(64, cdiv(rows, 256)), (wsf - off) // (2 * cols))
    gy = gy if gy > 1 else 1
    return "wide", gy, 3 if gy > 1 else 2


def norm_wide_ws(rows, cols, partials):
    return (cdiv(2 * rows, 64) * 64 + partials * 2 * cols) * 4


def lora_down_S(M, K, w_kr, scratch):
    """-> K slices of the MFMA kernel (0: the per-row kernel).  scratch: what llmseg_amd.ops.lora_down hands over by default (True) or none (False)"""
    if w_kr or K % 128:
        return 0
    tiles = cdiv(M, 16)
    sb = 32 * 2 * M * 16 * 4 if (scratch and tiles < 256 and K % 256 == 0) else 0
    S = 1
    while tiles * S < 256 and K % (256 * S) == 0 and sb and S * 2 * M * 64 <= sb and S < 32:
        S *= 2
    return S


def outer_slices(M, N, nz, ws):
    colwg = cdiv(N, 64)
    gy = max(max(1, 256 // (colwg * nz)), min(32, M // 512))
    return max(1, min(gy, ws // (nz * N * 8 * 4)))


def sumsq_groups(n, ws):
    return max(1, min(min(2048, cdiv(n, 2048)), ws // 4))


def route(case):
    """-> (slices / partials of the reduction (1 where none), launches) as the dispatch code of the library decides them"""
    p, op = case.p, case.op
    if op == "colsum":
        s = colsum_slices(p["M"], p["N"], case.ws_bytes)
        return s, 2 if s > 1 else 1
    if op == "norm_bwd":
        _, s, l = norm_route(p["rows"], p["cols"], p["dw"], case.ws_bytes)
        return s, l
    if op == "lora_down":
        S = lora_down_S(p["M"], p["K"], p.get("w_kr", False), p.get("scratch", True))
        if p.get("parts") and S > 1:
            return S, 3                     # the MFMA launch (no finish) + the K-sliced dX product + its ONE tail launch, which finishes the partials and writes y
        return max(S, 1), (2 if S > 1 else 1) + (1 if p.get("pack") and S <= 1 else 0)
    if op in ("lora_outer", "lora_wgrads"):
        s = outer_slices(p["M"], p["N"], 4 if op == "lora_wgrads" else p["nz"], case.ws_bytes)
        return s, 2 if s > 1 else 1
    if op == "sumsq":
        return sumsq_groups(p["n"], case.ws_bytes), 2
    if op == "ce":
        return 1, 3                         # ce_loss (rows + fold) and ce_bwd
    if op == "softmax_ds":
        return 1, 2                         # softmax_rows and attn_ds
    return 1, 1


# ----------------------------------------------------------------------------------------------------------------- the case table
def _ws2(op, **p):
    """workspace bytes that cut the reduction of this call to two slices / partials"""
    if op == "colsum":
        return 2 * p["N"] * 4
    if op == "norm_acc":
        return 2 * 2 * p["cols"] * 4
    if op == "norm_wide":
        return norm_wide_ws(p["rows"], p["cols"], 2)
    if op == "outer":
        return 2 * p["nz"] * p["N"] * 8 * 4
    raise KeyError(op)


EINVAL_WIDE = "norm_bwd: weight gradients of a wide norm need workspace >= (2 rows + 2 cols) floats (row statistics)"


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # ---- norm_bwd, frozen weight: rms and layer form, with and without dres
    for rows, cols, rt in ((638, 4096, "wg_cpt2"), (7656, 4096, "wg_cpt2"), (64, 2048, "wg_cpt1"), (63, 4096, "wave_cpl8"), (1, 4096, "wave_cpl8"),
                           (200, 2040, "wave_cpl4"), (70, 8192, "wg_cpt4"), (5, 8200, "wave_cpl0"), (3, 8, "wave_cpl1"), (333, 520, "wave_cpl2")):
        for k, (rms, dres) in enumerate(((1, 1), (0, 0), (1, 0), (0, 1))):
            if rows == 7656 and k >= 2:
                continue                    # the tall shape: rms + dres (the benchmark's call) and layer without
            add("norm_bwd", f"frozen_{rows}x{cols}_{'rms' if rms else 'ln'}{'_dres' if dres else ''}", 1, rows=rows, cols=cols, rms=rms, dres=dres, dw=0,
                db=0, route=rt)
    # ---- norm_bwd with dw / db (pre-filled: the contract is +=): every row class on each of the three routes
    acc_l = {1: 1, 3: 1, 31: 1, 33: 2, 200: 2, 638: 2, 7656: 2}
    wide_l = {1: 2, 3: 2, 31: 2, 33: 2, 200: 2, 638: 3, 7656: 3}
    for i, rows in enumerate((1, 3, 31, 33, 200, 638, 7656)):
        for cols, rt in ((256, "acc_cpl1"), ((520, 1024)[i % 2], "acc_cpl2"), ((1032, 4096)[i % 2], "wide")):
            rms = (i + cols // 8) % 2
            add("norm_bwd", f"wgrad_{rows}x{cols}_{'rms' if rms else 'ln'}{'_dres' if i % 2 else ''}", (wide_l if rt == "wide" else acc_l)[rows], rows=rows, cols=cols,
                rms=rms, dres=i % 2, dw=1, db=1, route=rt)
    for rows, cols, rt, l in ((200, 520, "acc_cpl2", 2), (638, 4096, "wide", 3)):
        add("norm_bwd", f"wgrad_{rows}x{cols}_rms_nodb", l, rows=rows, cols=cols, rms=1, dres=0, dw=1, db=0, route=rt)
    for rows, cols, rt, kind in ((200, 256, "acc_cpl1", "norm_acc"), (638, 1024, "acc_cpl2", "norm_acc"), (638, 4096, "wide", "norm_wide"), (7656, 1032, "wide", "norm_wide")):
        add("norm_bwd", f"wgrad_{rows}x{cols}_ln_ws2", 3 if rt == "wide" else 2, ws=_ws2(kind, rows=rows, cols=cols), rows=rows, cols=cols, rms=0, dres=1, dw=1, db=1, route=rt)
        if rt == "wide":
            add("norm_bwd", f"wgrad_{rows}x{cols}_ln_wsnone", 0, ws="none", einval=EINVAL_WIDE, rows=rows, cols=cols, rms=0, dres=1, dw=1, db=1, route="einval")
        else:
            add("norm_bwd", f"wgrad_{rows}x{cols}_ln_wsnone", 1, ws="none", rows=rows, cols=cols, rms=0, dres=1, dw=1, db=1, route=rt)
    # ---- colsum
    for M, N, ld in ((512, 256, 256), (512, 2048, 2048), (638, 4096, 4096), (7656, 4096, 4096), (200, 264, 264), (7, 1, 8), (31, 8, 8), (2049, 72, 136)):
        add("colsum", f"{M}x{N}_ld{ld}", 2 if M > 32 else 1, M=M, N=N, ld=ld)
    for M, N, ld in ((512, 2048, 2048), (2049, 72, 136)):
        add("colsum", f"{M}x{N}_ld{ld}_ws2", 2, ws=_ws2("colsum", N=N), M=M, N=N, ld=ld)
        add("colsum", f"{M}x{N}_ld{ld}_wsnone", 1, ws="none", M=M, N=N, ld=ld)
    # ---- ce_loss + ce_bwd on the same inputs
    for (N, T), (V, ld) in (((2, 319), (32004, 32004)), ((2, 9), (32004, 32064)), ((1, 2), (1000, 1000)), ((2, 9), (32003, 32008)), ((2, 9), (32772, 32776)),
                            ((2, 319), (37, 40)), ((1, 2), (32004, 32064)), ((2, 9), (1000, 1000))):
        add("ce", f"{N}x{T}_V{V}_ld{ld}", 3, N=N, T=T, V=V, ld=ld)
    # ---- scatter_add_rows
    for n, cols, pat in ((1, 64, "distinct"), (255, 72, "hot"), (256, 64, "firstlast"), (257, 72, "distinct"), (1023, 64, "hot"), (1024, 72, "firstlast"),
                         (1025, 64, "firstlast"), (2500, 72, "hot"), (2500, 64, "firstlast"), (7656, 4096, "hot"), (7656, 64, "firstlast"), (1025, 4096, "distinct")):
        add("scatter_add", f"n{n}_c{cols}_{pat}", 1, n=n, cols=cols, pat=pat)
    # ---- sumsq
    for dt in ("bf16", "f32"):
        for n in (1, 7, 1000, 4099, 2 ** 22 + 3):
            add("sumsq", f"{dt}_n{n}", 2, ws=8192, n=n, dt=dt, off=0)
    for n in (7, 4099, 2 ** 22 + 3):
        add("sumsq", f"f32_n{n}_offset1", 2, ws=8192, n=n, dt="f32", off=1)
    for ws in (4, 64):
        add("sumsq", f"f32_n{2 ** 22 + 3}_ws{ws}", 2, ws=ws, n=2 ** 22 + 3, dt="f32", off=0)
        add("sumsq", f"bf16_n4099_ws{ws}", 2, ws=ws, n=4099, dt="bf16", off=0)
    # ---- adamw
    for n in (1000, 3 * 2 ** 21 + 5):
        for k, (gdt, gs, wd, step) in enumerate((("bf16", 0, 0.01, 1), ("f32", 1, 0.0, 2), ("bf16", 1, 0.01, 1000), ("f32", 0, 0.01, 1), ("f32", 1, 0.01, 1), ("bf16", 0, 0.0, 2))):
            if n > 1000 and k >= 2:
                continue
            add("adamw", f"n{n}_{gdt}{'_gs' if gs else ''}_wd{wd}_step{step}", 1, n=n, gdt=gdt, gs=gs, wd=wd, step=step)
    # ---- lora_down: launches = MFMA (+ finish where K-sliced), + 1 where a pack rides without a finish launch
    D = dict(nb=2, same=1, zc=0, wide=0, drop=0, seg=0, w_kr=0, scratch=1, pack=0, parts=0)
    for name, l, kw in (("638x4096_S8", 2, dict(M=638, K=4096)), ("638x4096_S8_x2_zc48_wide", 2, dict(M=638, K=4096, same=0, zc=48, wide=1)),
                        ("638x4096_S8_drop", 2, dict(M=638, K=4096, drop=1)), ("638x4096_S8_drop_seg", 2, dict(M=638, K=4096, drop=1, seg=319)),
                        ("638x4096_S8_nb1_drop", 2, dict(M=638, K=4096, nb=1, drop=1)), ("638x4096_S8_pack", 2, dict(M=638, K=4096, pack=1, zc=48, wide=1)),
                        ("638x4096_S8_parts_gemm_tail", 3, dict(M=638, K=4096, same=0, zc=48, wide=1, parts=1)),
                        ("638x4096_S8_parts_gemm_tail_same", 3, dict(M=638, K=4096, zc=48, wide=1, parts=1)),
                        ("7656x4096_S1", 1, dict(M=7656, K=4096)), ("7656x4096_S1_x2_drop_seg", 1, dict(M=7656, K=4096, same=0, drop=1, seg=319, zc=48, wide=1)),
                        ("638x4096_noscratch", 1, dict(M=638, K=4096, scratch=0, zc=48, wide=1)), ("638x4096_noscratch_pack", 2, dict(M=638, K=4096, scratch=0, pack=1)),
                        ("50x256_S2", 2, dict(M=50, K=256)), ("50x256_S2_nb1_zc48", 2, dict(M=50, K=256, nb=1, zc=48, wide=1)),
                        ("37x136_rw1", 1, dict(M=37, K=136, same=0, zc=48, wide=1)), ("37x136_rw1_drop", 1, dict(M=37, K=136, drop=1)),
                        ("2100x264_rw4", 1, dict(M=2100, K=264, same=0)), ("2100x264_rw4_nb1_zc48_drop_seg", 1, dict(M=2100, K=264, nb=1, zc=48, wide=1, drop=1, seg=700)),
                        ("50x256_wkr", 1, dict(M=50, K=256, w_kr=1, zc=48, wide=1)), ("2100x264_wkr", 1, dict(M=2100, K=264, w_kr=1, drop=1)),
                        ("1x4096_S32", 2, dict(M=1, K=4096)), ("15x4096_S32", 2, dict(M=15, K=4096, same=0, drop=1)), ("16x4096_S32", 2, dict(M=16, K=4096, zc=48, wide=1)),
                        ("17x4096_S32", 2, dict(M=17, K=4096, nb=1)), ("17x384_S1", 1, dict(M=17, K=384, same=0)),
                        # parts=1 where the shape takes no K slices (per-row kernel; MFMA with S = 1; MFMA unsliced for want of scratch): S = 0 comes back, no
                        # partials, y complete after the one launch and the same bits as the plain call
                        ("37x136_rw1_parts_noslices", 1, dict(M=37, K=136, same=0, zc=48, wide=1, parts=1)), ("17x384_S1_parts_noslices", 1, dict(M=17, K=384, same=0, parts=1)),
                        ("50x256_noscratch_parts_noslices", 1, dict(M=50, K=256, scratch=0, parts=1))):
        add("lora_down", name, l, **{**D, **kw})
    # ---- lora_outer / lora_wgrads
    for M, N, l in ((638, 4096, 1), (7656, 4096, 2), (50, 256, 2), (37, 264, 2), (1, 8, 2), (5, 72, 2)):      # l: launches of lora_wgrads (nz = 4); lora_outer always slices here
        for k, (rn, nz, drop) in enumerate(((0, 1, 0), (1, 2, 1))):
            add("lora_outer", f"{M}x{N}_{'rn' if rn else 'nr'}_nz{nz}{'_drop' if drop else ''}", 2, M=M, N=N, rn=rn, nz=nz, drop=drop, seg=0)
        add("lora_wgrads", f"{M}x{N}{'_drop' if M != 50 else ''}{'_seg' if M in (638, 7656) else ''}", l, M=M, N=N, drop=int(M != 50),
            seg=319 if M in (638, 7656) else 0)
    for M, N in ((638, 4096), (37, 264)):
        add("lora_outer", f"{M}x{N}_rn_nz2_ws2", 2, ws=_ws2("outer", N=N, nz=2), M=M, N=N, rn=1, nz=2, drop=0, seg=0)
        add("lora_outer", f"{M}x{N}_nr_nz1_wsnone", 1, ws="none", M=M, N=N, rn=0, nz=1, drop=1, seg=0)
    for M, N in ((50, 256), (37, 264)):
        add("lora_wgrads", f"{M}x{N}_ws2", 2, ws=_ws2("outer", N=N, nz=4), M=M, N=N, drop=1, seg=0)
        add("lora_wgrads", f"{M}x{N}_wsnone", 1, ws="none", M=M, N=N, drop=0, seg=0)
    # ---- lora_apply, lora_pack
    for name, kw in (("50x256_nr_nb1", dict(M=50, N=256, rn=0, nb=1, drop=0, strided=1)), ("638x4096_rn_nb2_drop", dict(M=638, N=4096, rn=1, nb=2, drop=1, strided=0)),
                     ("37x264_nr_nb2_drop", dict(M=37, N=264, rn=0, nb=2, drop=1, strided=0)), ("5x72_rn_nb1_strided", dict(M=5, N=72, rn=1, nb=1, drop=0, strided=1)),
                     ("7656x4096_rn_nb2_strided", dict(M=7656, N=4096, rn=1, nb=2, drop=0, strided=1))):
        add("lora_apply", name, 1, **kw)
    for H in (8, 264, 4096):
        add("lora_pack", f"H{H}", 1, H=H)
    # ---- transpose_pad, swiglu_bwd, act_bwd
    for rows, cols, pad, ld_in, wide in ((200, 256, 256, 256, 0), (638, 4096, 640, 4096, 0), (7, 8, 8, 8, 0), (65, 72, 128, 72, 0), (65, 72, 72, 136, 1), (638, 4096, 640, 4104, 1)):
        add("transpose_pad", f"{rows}x{cols}_pad{pad}_ld{ld_in}{'_wide' if wide else ''}", 1, rows=rows, cols=cols, pad=pad, ld_in=ld_in, wide=wide)
    for rows, I in ((77, 512), (638, 11008)):
        add("swiglu_bwd", f"{rows}x{I}", 1, rows=rows, I=I)
    for act in ("relu", "sigmoid"):
        add("act_bwd", f"{act}_n1001", 1, act=act, n=1001)
    # ---- softmax_rows + attn_ds (the head_dim 80 fallback of the attention backward)
    for BH, T, ld, causal, mask in ((4, 196, 200, 0, 0), (4, 37, 40, 1, 0), (4, 64, 64, 0, 1), (4, 64, 64, 1, 1)):
        add("softmax_ds", f"{BH}x{T}_ld{ld}{'_causal' if causal else ''}{'_mask' if mask else ''}", 2, BH=BH, T=T, ld=ld, causal=causal, mask=mask, heads=2)
    return out


# --------------------------------------------------------------------------------------------------------------------- tolerance
def bf16_bound(ref):
    ref = ref.to(F64)
    return C_BF16 * 2.0 ** -8 * (ref.abs() + ref.pow(2).mean(-1, keepdim=True).sqrt())


def f32_bound(n, sabs, c=None):
    return (C_SUM if c is None else c) * 2.0 ** -24 * math.sqrt(n) * sabs.to(F64)


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; equal elements count 0 (also where the bound is 0), NaN -> inf"""
    got, ref = got.to(F64), ref.to(F64)
    d = (got - ref).abs()
    r = torch.nan_to_num(torch.where(d == 0, torch.zeros_like(d), d / bound.expand_as(d)), nan=INF, posinf=INF)
    r = torch.where(torch.isnan(got) | torch.isnan(ref), torch.full_like(r, INF), r)
    r = torch.where(torch.isnan(got) & torch.isnan(ref), torch.zeros_like(r), r)          # a sentinel that stayed
    return float(r.max()) if r.numel() else 0.0


def ratios(got, refs, bounds):
    return {n: ratio(got[n], refs[n], bounds[n]) for n in refs}


# --------------------------------------------------------------------------------------------------------------------- helpers
def _g(case):
    return torch.Generator().manual_seed(case.seed)


def _T(t, emu):
    return t.to(F32 if emu else F64)


def _rb(t, emu):
    """the bf16 store of the kernels (emulation only)"""
    return t.to(BF).to(F64) if emu else t


def _sum0(t, emu, slices=1, per=None):
    """sum over dim 0.  fp64 reference; emulation 'seq': fp32, one term after the other; 'sliced': fp32 slices of `per` rows folded in order"""
    if not emu:
        return t.sum(0)
    if emu == "seq" or slices <= 1:
        return torch.cumsum(t, 0)[-1]
    per = cdiv(t.shape[0], slices) if per is None else per
    acc = None
    for s in range(slices):
        c = t[s * per:(s + 1) * per]
        if c.shape[0]:
            v = c.sum(0)
            acc = v if acc is None else acc + v
    return acc


def keep(case, rows, cols, stream_add=0):
    """dropout keep mask * scale (fp64) of a dense [rows, cols] activation, or None"""
    if not case.p.get("drop"):
        return None
    return odrop.keep_mask(rows, cols, SEED, OFFSET, STREAM + stream_add, P_DROP, case.p.get("seg", 0)).to(F64) * odrop.drop_scale(P_DROP)


# ------------------------------------------------------------------------------------------------------------------------ norm_bwd
def norm_inputs(case):
    g = _g(case)
    r, c = case.rows, case.cols
    z = torch.randn(r, c, generator=g)
    x = (z * 0.005 + 0.002).to(BF)                                      # small x: eps = 1e-5 is ~30 % of the variance
    dy = ((torch.randn(r, c, generator=g) + 0.5 + 0.7 * z) * 0.01).to(BF)      # biased and correlated with x: c1 (layer form) and c2 carry weight on every row
    w = (1.5 + 0.5 * torch.randn(c, generator=g)).to(BF)                # mean != 1: the weight inside c2 matters on a single row too
    dres = torch.randn(r, c, generator=g).to(BF) if case.dres else None
    return dict(x=x, dy=dy, w=w, dres=dres, eps=1e-5)


def norm_compute(case, inp, mut=None, emu=None):
    """-> (outputs, aux): dx (bf16 form), dw / db (fp32 sums on top of FILL; aux = (n, sum |t|))"""
    x, dy, w = (_T(inp[k], emu) for k in ("x", "dy", "w"))
    cols, rms = case.cols, case.rms
    eps = 0.0 if mut == "eps_dropped" else float(np.float32(inp["eps"]))
    div = cdiv(cols, 512) * 512 if mut == "stats_over_padded_width" else cols
    mean = torch.zeros_like(x[:, :1]) if rms else x.sum(-1, keepdim=True) / div
    xc = x - mean
    rstd = ((xc * xc).sum(-1, keepdim=True) / div + eps).rsqrt()
    if mut == "stats_over_padded_width" and not rms:                     # the zero padding of the chunk enters the centred sum too
        rstd = (((xc * xc).sum(-1, keepdim=True) + (div - cols) * mean * mean) / div + eps).rsqrt()
    xh = xc * rstd
    gg = dy * w
    c1 = torch.zeros_like(mean) if (rms or mut == "c1_dropped") else gg.sum(-1, keepdim=True) / cols
    c2 = ((dy if mut == "c2_without_weight" else gg) * xh).sum(-1, keepdim=True) / cols
    dx = rstd * (gg - c1 - xh * c2)
    if inp["dres"] is not None and mut != "dres_dropped":
        dx = dx + _T(inp["dres"], emu)
    out, aux = {"dx": _rb(dx, emu).to(F64)}, {}
    if case.dw or case.db:
        _, G, _ = norm_route(case.rows, cols, True, case.ws_bytes)
        rows = torch.arange(case.rows)
        sel = torch.ones(case.rows, dtype=torch.bool)
        acc = case.route.startswith("acc")
        if mut == "last_row_dropped":
            sel[-1] = False
        elif mut == "last_partial_dropped":
            sel = ((rows // 4) % G != G - 1) if acc else (rows < cdiv(case.rows, G) * (G - 1))
        for name, on, t in (("dw", case.dw, dy * xh), ("db", case.db, dy)):
            if not on:
                continue
            tt = t[sel]
            if mut == "first_row_twice":
                tt = torch.cat([t[:1], tt])
            if mut == "last_column_chunk_zero":
                tt = tt.clone()
                tt[:, (cols - 1) // 64 * 64:] = 0
            if emu == "sliced" and acc:                                   # workgroup b walks rows 4 b + wave, + 4 G, ...
                order = torch.argsort((rows // 4) % G, stable=True)
                s = _sum0(tt[order], emu, G, None) if G > 1 else _sum0(tt, "seq")
            else:
                s = _sum0(tt, emu, G) if tt.shape[0] else torch.zeros(cols, dtype=tt.dtype)
            fill = 0.0 if mut == "existing_content_ignored" else FILL
            out[name] = ((torch.full_like(s, fill) + s) if emu else (s + fill)).to(F64)
            if not emu and mut is None:
                aux[name] = (case.rows + 1, t.abs().sum(0) + FILL)
    return out, aux


def norm_mutants(case):
    m = ["c2_without_weight", "eps_dropped"]
    if not case.rms:
        m.append("c1_dropped")
    if case.dres:
        m.append("dres_dropped")
    if cdiv(case.cols, 512) * 512 >= 1.25 * case.cols:                    # a smaller change of the divisor is below what a bf16 dx resolves
        m.append("stats_over_padded_width")
    if case.dw or case.db:
        m += ["last_row_dropped", "first_row_twice", "existing_content_ignored"]
        if case.cols % 64:
            m.append("last_column_chunk_zero")
        _, G, _ = norm_route(case.rows, case.cols, True, case.ws_bytes)
        if G > 1 and (case.route.startswith("acc") or cdiv(case.rows, G) * (G - 1) < case.rows):
            m.append("last_partial_dropped")
    return m


# -------------------------------------------------------------------------------------------------------------------------- colsum
COLSUM_FILL = 16.0        # the existing content of `out`: large enough to show under the bound of a 7656-term column (FILL would sit at 1.7 x)


def colsum_inputs(case):
    g = _g(case)
    return dict(x=((torch.randn(case.M, case.ld, generator=g) + 0.25).to(BF)))       # a column view [:, :N] of a matrix ld wide


def colsum_compute(case, inp, mut=None, emu=None):
    t = _T(inp["x"][:, :case.N], emu)
    gy = colsum_slices(case.M, case.N, case.ws_bytes)
    full = t
    if mut == "last_row_dropped":
        t = t[:-1]
    elif mut == "last_partial_dropped":
        t = t[:cdiv(case.M, gy) * (gy - 1)]
    elif mut == "first_row_twice":
        t = torch.cat([t[:1], t])
    elif mut == "last_column_chunk_zero":
        t = t.clone()
        t[:, (case.N - 1) // 64 * 64:] = 0
    s = _sum0(t, emu, gy) if t.shape[0] else torch.zeros(case.N, dtype=t.dtype)
    fill = 0.0 if mut == "existing_content_ignored" else COLSUM_FILL
    out = {"out": ((torch.full_like(s, fill) + s) if emu else s + fill).to(F64)}
    return out, ({"out": (case.M + 1, full.abs().sum(0) + COLSUM_FILL)} if not emu and mut is None else {})


def colsum_mutants(case):
    m = ["first_row_twice", "existing_content_ignored", "last_row_dropped"]
    if case.N % 64:
        m.append("last_column_chunk_zero")
    gy = colsum_slices(case.M, case.N, case.ws_bytes)
    if gy > 1 and cdiv(case.M, gy) * (gy - 1) < case.M:                   # the last slice holds rows
        m.append("last_partial_dropped")
    return m


# ------------------------------------------------------------------------------------------------------------------------------ CE
PAD_LOGIT = 12.0        # what the columns V .. ld of the logits hold: a softmax over ld instead of V is dominated by them
COEF = 0.37


def ce_inputs(case):
    g = _g(case)
    N, T, V, ld = case.N, case.T, case.V, case.ld
    lg = torch.full((N, T, ld), PAD_LOGIT)
    lg[..., :V] = torch.randn(N, T, V, generator=g) * 2.0
    lab = torch.randint(0, V, (N, T), generator=g)
    if T >= 9:
        lab[0, :3] = -100                    # a leading run of ignored labels
        lab[0, 4] = V                        # out of range: treated as ignored
        lab[0, 5], lab[0, 6] = 0, V - 1      # the first and the last column
        lab[N - 1, :] = -100                 # one sequence entirely ignored
    else:
        lab[0, 1] = V - 1
    return dict(logits=lg.to(BF), labels=lab, coef=torch.tensor([COEF]))


def ce_compute(case, inp, mut=None, emu=None):
    """-> loss fp32[2] = (sum nll, count) and dlogits [N, T, V] (bf16 form; rows of ignored positions and of t = T - 1 exactly zero)"""
    N, T, V = case.N, case.T, case.V
    width = case.ld if mut == "softmax_over_ld" else V
    x = _T(inp["logits"][..., :width], emu)
    lab = inp["labels"]
    tgt = torch.full((N, T), -100, dtype=torch.int64)
    if mut == "label_unshifted":
        tgt[:] = lab
    else:
        tgt[:, :-1] = lab[:, 1:]
        if mut == "last_position_scored":
            tgt[:, -1] = lab[:, 0]
    valid = (tgt >= 0) & (tgt < V)
    if mut == "last_position_scored":
        valid[:, -1] = True
        tgt[:, -1] = tgt[:, -1].clamp(0, V - 1)
    mx = x.amax(-1, keepdim=True)
    e = torch.exp(x - mx)
    s = e.sum(-1, keepdim=True)
    sm = (e / s)[..., :V]
    oh = torch.zeros_like(sm)
    if mut != "onehot_missing":
        oh.scatter_(-1, tgt.clamp(0, V - 1)[..., None], 1.0)
    c = 1.0 if mut == "coef_not_applied" else float(np.float32(COEF))
    dl = c * (sm - oh)
    if mut == "ignored_row_nonzero":
        dl = torch.where(valid[..., None] | (torch.arange(T) == T - 1)[None, :, None], dl, c * sm)
        dl = torch.where((valid | (tgt < 0) | (tgt >= V))[..., None] & ~(torch.arange(T) == T - 1)[None, :, None], dl, torch.zeros_like(dl))
    else:
        dl = torch.where(valid[..., None], dl, torch.zeros_like(dl))
    xl = x.gather(-1, tgt.clamp(0, V - 1)[..., None])
    terms = torch.stack([mx, torch.log(s), -xl], 0).squeeze(-1) * valid                          # nll = mx + log s - x[label]
    nll = terms.sum(0)
    if emu:
        loss = torch.stack([torch.cumsum(nll.reshape(-1), 0)[-1], valid.sum().to(nll.dtype)])
    else:
        loss = torch.stack([nll.sum(), valid.sum().to(F64)])
    if mut == "count_includes_ignored":
        loss[1] = N * (T - 1)
    out = {"dlogits": _rb(dl, emu).to(F64), "loss": loss.to(F64)}
    aux = {}
    if not emu and mut is None:
        aux["loss"] = (3 * max(1, int(valid.sum())), torch.stack([terms.abs().sum(), torch.zeros((), dtype=F64)]))      # the count is exact
    return out, aux


def ce_mutants(case):
    m = ["label_unshifted", "last_position_scored", "coef_not_applied", "onehot_missing"]
    if case.ld > case.V:
        m.append("softmax_over_ld")
    if case.T >= 9:
        m += ["ignored_row_nonzero", "count_includes_ignored"]
    return m


# --------------------------------------------------------------------------------------------------------------------- scatter_add
N_DST = 8000


def scatter_inputs(case):
    g = _g(case)
    n, cols, pat = case.n, case.cols, case.pat
    src = (torch.randn(n, cols, generator=g) + 0.25).to(BF)
    if pat == "distinct":
        idx = torch.randperm(N_DST, generator=g)[:n]
    elif pat == "hot":
        idx = torch.randint(0, 10, (n,), generator=g) * 777 + 3            # ~10 destinations hit n / 10 times each
    else:
        idx = torch.randperm(N_DST, generator=g)[:n]
        idx[-1] = idx[0] = 4242 if n > 1 else idx[0]                       # one destination hit by the first and the last source row
        if n > 2:
            idx[n // 2] = 4242
    if n >= 16:
        idx[1], idx[n // 3], idx[n - 2] = -1, -1, -1
    if pat == "hot" or (pat == "distinct" and n > 1):
        idx[0] = -1                                                        # a skipped row in position 0
    return dict(src=src, idx=idx.to(torch.int64))


def scatter_compute(case, inp, mut=None, emu=None):
    src, idx = _T(inp["src"], emu), inp["idx"].clone()
    n = case.n
    sel = idx >= 0
    if mut == "minus_one_to_row0":
        idx = idx.clamp(min=0)
        sel = torch.ones(n, dtype=torch.bool)
    seen, first = {}, {}
    if mut in ("second_hit_dropped", "hits_beyond_1024_dropped"):
        for i, d in enumerate(idx.tolist()):
            if d < 0:
                continue
            first.setdefault(d, i)
            seen[d] = seen.get(d, 0) + 1
            if (mut == "second_hit_dropped" and seen[d] == 2) or (mut == "hits_beyond_1024_dropped" and i - first[d] >= 1024):
                sel[i] = False
    if mut == "last_row_dropped":
        sel[int(torch.nonzero(idx >= 0).flatten()[-1])] = False
    dst = torch.full((N_DST, case.cols), 0.0 if mut == "existing_content_ignored" else FILL, dtype=src.dtype)
    ii = torch.nonzero(sel).flatten()
    if emu:                                                                # the owner adds a chunk's hits in source order, then += into dst
        for i in ii.tolist():
            dst[idx[i]] += src[i]
    else:
        dst.index_add_(0, idx[ii], src[ii])
    aux = {}
    if not emu and mut is None:
        sab = torch.full((N_DST, case.cols), FILL, dtype=F64).index_add_(0, idx[ii], src[ii].abs())
        cnt = torch.ones(N_DST, dtype=F64).index_add_(0, idx[ii], torch.ones(len(ii), dtype=F64))
        aux["dst"] = (1, sab * cnt.sqrt()[:, None])                        # sqrt(n) per destination row, folded into sum |t|
    return {"dst": dst.to(F64)}, aux


def scatter_mutants(case):
    idx = inp_cached(case)["idx"]
    v = idx[idx >= 0]
    m = ["last_row_dropped", "existing_content_ignored"]
    if len(v) != len(v.unique()):
        m.append("second_hit_dropped")
    if bool((idx < 0).any()):
        m.append("minus_one_to_row0")
    first = {}
    for i, d in enumerate(idx.tolist()):
        if d >= 0 and i - first.setdefault(d, i) >= 1024:
            m.append("hits_beyond_1024_dropped")
            break
    return m


# --------------------------------------------------------------------------------------------------------------------------- sumsq
def sumsq_inputs(case):
    g = _g(case)
    n = case.n
    buf = torch.randn(n + 1, generator=g) * 3.0
    big = max(3.0, float(round(0.9 * math.sqrt(n))))                         # a tenth of the total each: one dropped element, tail or workgroup share shows in a sum of 4 M terms
    for i in (0, n - 1, (sumsq_groups(n, case.ws_bytes) - 1) * 256):
        if i < n:
            buf[case.off + i] = big
    buf = buf.to(BF) if case.dt == "bf16" else buf
    return dict(buf=buf)                                                   # x = buf[off : off + n]


def sumsq_compute(case, inp, mut=None, emu=None):
    x = _T(inp["buf"][case.off:case.off + case.n], emu)
    n = case.n
    if mut == "tail_dropped":
        x = x[:n // 4 * 4]
    elif mut == "last_partial_dropped":                                    # the grid-stride share of the last workgroup
        G = sumsq_groups(n, case.ws_bytes)
        i = torch.arange(x.numel())
        x = x[(i // 256) % G != G - 1]
    elif mut == "first_row_twice":
        x = torch.cat([x[:1], x])
    elif mut == "last_row_dropped":
        x = x[:-1]
    t = x * x
    if emu == "sliced":
        G = sumsq_groups(n, case.ws_bytes)
        pad = torch.zeros(cdiv(t.numel(), 256 * G) * 256 * G, dtype=t.dtype)
        pad[:t.numel()] = t
        s = torch.cumsum(pad.view(-1, G, 256).sum(0).sum(-1), 0)[-1]      # per thread, per workgroup, then the fold
    elif emu:
        s = torch.cumsum(t, 0)[-1] if t.numel() else torch.zeros((), dtype=t.dtype)
    else:
        s = t.sum()
    fill = 0.0 if mut == "existing_content_ignored" else float(n)         # `out` is pre-filled with n (about a ninth of the sum)
    out = {"out": ((torch.full_like(s, fill) + s) if emu else s + fill).to(F64).reshape(1)}
    return out, ({"out": (n + 1, (t.sum() + float(n)).reshape(1))} if not emu and mut is None else {})


def sumsq_mutants(case):
    m = ["existing_content_ignored", "first_row_twice", "last_row_dropped"]
    if case.n % 4 and case.dt == "f32" and case.off == 0:
        m.append("tail_dropped")
    if sumsq_groups(case.n, case.ws_bytes) > 1:
        m.append("last_partial_dropped")
    return m


# --------------------------------------------------------------------------------------------------------------------------- adamw
LR, B1, B2, AEPS, GSCALE = 3e-4, 0.9, 0.95, 1e-8, 0.5


def adamw_inputs(case):
    g = _g(case)
    n = case.n
    master = torch.randn(n, generator=g) * 0.02
    grad = torch.randn(n, generator=g) * 1e-3
    grad = grad.to(BF) if case.gdt == "bf16" else grad
    m = torch.randn(n, generator=g).abs() * 5e-4 * torch.sign(grad.float())      # same sign as the gradient: m does not cancel (its error would reach master amplified)
    v = (torch.randn(n, generator=g) * 1e-3).pow(2) + 1e-8
    return dict(master=master, grad=grad, m=m, v=v)


def adamw_bc(step, exact=False):
    """bias corrections: as the host code computes them (powf in fp32), or exactly"""
    if exact:
        return 1.0 - float(np.float32(B1)) ** step, 1.0 - float(np.float32(B2)) ** step
    f = np.float32
    return float(f(1) - np.power(f(B1), f(step), dtype=f)), float(f(1) - np.power(f(B2), f(step), dtype=f))


def adamw_compute(case, inp, mut=None, emu=None, exact_bc=False):
    f = lambda v: float(np.float32(v))
    lr, b1, b2, eps, wd = f(LR), f(B1), f(B2), f(AEPS), f(case.wd)
    c1, c2 = f(np.float32(1) - np.float32(B1)), f(np.float32(1) - np.float32(B2))
    bc1, bc2 = (1.0, 1.0) if mut == "bias_correction_missing" else adamw_bc(case.step, exact_bc)
    gs = f(GSCALE) if (case.gs and mut != "grad_scale_ignored") else 1.0
    w, m0, v0 = (_T(inp[k], emu) for k in ("master", "m", "v"))
    g_raw = _T(inp["grad"], emu)
    g = gs * g_raw
    if mut == "wd_as_l2":
        g = g + wd * w
    gv = g_raw if mut == "m_v_from_unscaled_grad" else g
    m = b1 * m0 + c1 * gv
    v = b2 * v0 + c2 * gv * gv
    den = (v / bc2 + eps).sqrt() if mut == "eps_inside_sqrt" else (v / bc2).sqrt() + eps
    upd = (m / bc1) / den + (0.0 if mut == "wd_as_l2" else wd) * w
    w1 = w - lr * upd
    out = {"master": w1.to(F64), "m": m.to(F64), "v": v.to(F64), "p": _rb(w1, emu).to(F64)}
    aux = {}
    if not emu and mut is None:
        aux = {"master": (3, w.abs() + (lr * (m / bc1) / den).abs() + (lr * wd * w).abs()), "m": (2, (b1 * m0).abs() + (c1 * g).abs()), "v": (2, b2 * v0 + c2 * g * g)}
    return out, aux


def adamw_mutants(case):
    m = ["eps_inside_sqrt"]
    if case.step <= 2:
        m.append("bias_correction_missing")            # at step 1000 both corrections round to 1
    if case.wd:
        m.append("wd_as_l2")
    if case.gs:
        m += ["grad_scale_ignored", "m_v_from_unscaled_grad"]      # the same numbers in plain AdamW (g enters through m and v only); both names of the issue are kept
    return m


# ----------------------------------------------------------------------------------------------------------------------- lora_down
ALPHA = 0.25
PAD_ROWS = 16            # rows allocated beyond M in lora_down's out


def lora_down_inputs(case):
    g = _g(case)
    M, K = case.M, case.K
    x = torch.randn(M, K, generator=g).to(BF)
    x2 = x if case.same else torch.randn(M, K, generator=g).to(BF)
    w = [(torch.randn(8, K, generator=g) * K ** -0.5 + 0.3 * K ** -0.5).to(BF) for _ in range(2)]
    inp = dict(x=x, x2=x2, w0=w[0], w1=w[1])
    if case.p.get("parts") and route(case)[0] > 1:      # the dX product whose norm-backward tail finishes the K-slice partials: d [M, 3K] . wt [K, 3K]^T, pre-norm input nx, weight nw, LoRA A matrices
        Kg = 3 * K
        inp.update(d=(torch.randn(M, Kg, generator=g) * 0.3).to(BF), wt=(torch.randn(K, Kg, generator=g) * Kg ** -0.5).to(BF), nx=torch.randn(M, K, generator=g).to(BF),
                   nw=torch.randn(K, generator=g).to(BF), a0=(torch.randn(8, K, generator=g) * 0.1).to(BF), a1=(torch.randn(8, K, generator=g) * 0.1).to(BF))
    if case.pack:
        inp.update(pack_inputs(case, 264))
    return inp


def lora_down_compute(case, inp, mut=None, emu=None):
    M, K, nb = case.M, case.K, case.nb
    S, _ = route(case)
    ys = []
    for b in range(nb):
        xb = inp["x"] if (b == 0 or mut == "second_branch_reads_x") else inp["x2"]
        k = keep(case, M, K, 0 if mut == "v_uses_q_stream" else b)
        if k is not None and mut == "segment_offset_not_advanced":
            k = odrop.keep_mask(M, K, SEED, OFFSET, STREAM + b, P_DROP, 0)[:case.seg].repeat(cdiv(M, case.seg), 1)[:M].to(F64) * odrop.drop_scale(P_DROP)
        a = float(np.float32(ALPHA))
        if k is not None:                                                   # the mask zeroes elements of x (exact); the scale joins alpha
            xb = xb.to(F64) * (k != 0)
            a = a * (1.0 if mut == "dropout_scale_missing" else float(np.float32(odrop.drop_scale(P_DROP))))
        if mut == "alpha_missing":
            a = a / float(np.float32(ALPHA))
        xx, ww = _T(xb, emu), _T(inp[f"w{b}"], emu)
        if mut == "last_k_slice_dropped":
            xx = xx[:, :K - K // S]
            ww = ww[:, :K - K // S]
        if emu == "sliced" and S > 1:
            kq = K // S
            y = None
            for s in range(S):
                v = xx[:, s * kq:(s + 1) * kq] @ ww[:, s * kq:(s + 1) * kq].T
                y = v if y is None else y + v
        else:
            y = xx @ ww.T
        ys.append(y * a)
    y = _rb(torch.cat(ys + [torch.zeros(M, case.zc, dtype=ys[0].dtype)], 1), emu).to(F64)
    if mut == "zero_cols_hold_1e-4":
        y[:, 8 * nb:] = 1e-4
    y = torch.cat([y, torch.full((PAD_ROWS, y.shape[1]), float("nan"), dtype=F64)], 0)           # the rows >= M of an over-allocated out keep their NaN
    if mut == "row_m1_written_to_unused_tile_rows":
        y[M:cdiv(M, 16) * 16] = y[M - 1]
    out = {"y": y}
    if case.pack:
        out.update(pack_compute(case, inp)[0])
    return out, {}


def lora_down_mutants(case):
    m = ["alpha_missing"]
    if case.zc:
        m.append("zero_cols_hold_1e-4")
    if case.M % 16:
        m.append("row_m1_written_to_unused_tile_rows")
    if route(case)[0] > 1:
        m.append("last_k_slice_dropped")
    if case.nb == 2 and not case.same:
        m.append("second_branch_reads_x")
    if case.drop:
        m.append("dropout_scale_missing")
        if case.nb == 2 and case.same:
            m.append("v_uses_q_stream")
        if case.seg and case.M > case.seg:
            m.append("segment_offset_not_advanced")
    return m


# ---------------------------------------------------------------------------------------------------------- lora_outer / lora_wgrads
def outer_inputs(case):
    g = _g(case)
    M, N = case.M, case.N
    mk = lambda *s: (torch.randn(*s, generator=g) + 0.2).to(BF)
    if case.op == "lora_outer":
        return dict(a=[mk(M, N) for _ in range(case.nz)], b=mk(M, 64))        # b_z = b[:, 8 z : 8 z + 8] (row pitch 64)
    return dict(d=mk(M, 3 * N), x=mk(M, N), xa=mk(M, 64), t=mk(M, 16))


def _outer_products(case, inp):
    """[(name, a [M, N], b [M, 8], out_rn, alpha, dropout stream or None)]"""
    if case.op == "lora_outer":
        return [(f"out{z}", inp["a"][z], inp["b"][:, 8 * z:8 * z + 8], case.rn, ALPHA, z if case.drop else None) for z in range(case.nz)]
    N, d = case.N, inp["d"]
    return [("gbq", d[:, :N], inp["xa"][:, :8], 0, ALPHA, None), ("gbv", d[:, 2 * N:], inp["xa"][:, 8:16], 0, ALPHA, None),
            ("gaq", inp["x"], inp["t"][:, :8], 1, 1.0, 0 if case.drop else None), ("gav", inp["x"], inp["t"][:, 8:16], 1, 1.0, 1 if case.drop else None)]


def outer_compute(case, inp, mut=None, emu=None):
    M, N = case.M, case.N
    gy, _ = route(case)
    per = cdiv(M, gy * 4) * 4
    out, aux = {}, {}
    for name, a, b, rn, alpha, st in _outer_products(case, inp):
        a, b = _T(a, emu), _T(b, emu)
        if st is not None:
            k = keep(case, M, N, 0 if mut == "v_uses_q_stream" else st)
            if mut == "segment_offset_not_advanced":
                k = odrop.keep_mask(M, N, SEED, OFFSET, STREAM + st, P_DROP, 0)[:case.seg].repeat(cdiv(M, case.seg), 1)[:M].to(F64) * odrop.drop_scale(P_DROP)
            if mut == "dropout_scale_missing":
                k = (k != 0).to(F64)
            a = a * k.to(a.dtype)
        fa, fb = a, b
        if mut == "last_row_dropped":
            a, b = a[:-1], b[:-1]
        elif mut == "last_partial_dropped":
            a, b = a[:per * (gy - 1)], b[:per * (gy - 1)]
        elif mut == "first_row_twice":
            a, b = torch.cat([a[:1], a]), torch.cat([b[:1], b])
        elif mut == "last_column_chunk_zero":
            a = a.clone()
            a[:, (N - 1) // 64 * 64:] = 0
        if emu == "sliced" and gy > 1:
            s = None
            for i in range(gy):
                v = a[i * per:(i + 1) * per].T @ b[i * per:(i + 1) * per]
                s = v if s is None else s + v
        elif emu:                                                          # fp32, rows in order
            s = torch.zeros(N, 8, dtype=a.dtype)
            for r0 in range(0, a.shape[0], 8):
                s = s + a[r0:r0 + 8].T @ b[r0:r0 + 8]
        else:
            s = a.T @ b
        s = s * float(np.float32(alpha))
        fill = 0.0 if mut == "existing_content_ignored" else FILL
        s = (torch.full_like(s, fill) + s) if emu else s + fill
        out[name] = (s.T if rn else s).contiguous().to(F64)
        if not emu and mut is None:
            sab = (fa.abs().T @ fb.abs()) * abs(alpha) + FILL
            aux[name] = (M + 1, (sab.T if rn else sab).contiguous())
    return out, aux


def outer_mutants(case):
    m = ["last_row_dropped", "first_row_twice", "existing_content_ignored"]
    gy, _ = route(case)
    if gy > 1 and cdiv(case.M, gy * 4) * 4 * (gy - 1) < case.M:
        m.append("last_partial_dropped")
    if case.N % 64:
        m.append("last_column_chunk_zero")
    if case.drop:
        m.append("dropout_scale_missing")
        if case.op == "lora_wgrads" or case.nz == 2:
            m.append("v_uses_q_stream")
        if case.seg and case.M > case.seg:
            m.append("segment_offset_not_advanced")
    return m


# ------------------------------------------------------------------------------------------------------------ lora_apply / lora_pack
def apply_inputs(case):
    g = _g(case)
    M, N = case.M, case.N
    ld = N + 72 if case.strided else N
    w = [(torch.randn(*((8, N) if case.rn else (N, 8)), generator=g) + 0.2).to(BF) for _ in range(2)]
    return dict(y=torch.randn(M, ld, generator=g).to(BF), xa=(torch.randn(M, 64, generator=g) + 0.2).to(BF), w0=w[0], w1=w[1])


def apply_compute(case, inp, mut=None, emu=None):
    M, N = case.M, case.N
    y = _T(inp["y"][:, :N], emu)
    for b in range(case.nb):
        w = _T(inp[f"w{b}"], emu)
        dv = _T(inp["xa"][:, 8 * b:8 * b + 8], emu) @ (w if case.rn else w.T)
        k = keep(case, M, N, 0 if mut == "v_uses_q_stream" else b)
        if k is not None:
            dv = dv * ((k != 0).to(dv.dtype) if mut == "dropout_scale_missing" else k.to(dv.dtype))
        y = y + (1.0 if mut == "alpha_missing" else float(np.float32(ALPHA))) * dv
    return {"y": _rb(y, emu).to(F64)}, {}


def apply_mutants(case):
    m = ["alpha_missing"]
    if case.drop:
        m.append("dropout_scale_missing")
        if case.nb == 2:
            m.append("v_uses_q_stream")
    return m


PACK_S = 0.3


def pack_inputs(case, H=None):
    g = torch.Generator().manual_seed(case.seed + 1)
    H = case.p.get("H", H)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF)
    return dict(aq=mk(8, H), av=mk(8, H), bq=mk(H, 8), bv=mk(H, 8))


def pack_compute(case, inp, mut=None, emu=None):
    """the layout formula of include/llmseg_hip.h, bit for bit: the only rounding is s * B to bf16"""
    aq, av, bq, bv = (inp[k] for k in ("aq", "av", "bq", "bv"))
    H = aq.shape[1]
    sb = lambda b: (b.float() * np.float32(PACK_S)).to(BF)
    w2b = torch.zeros(3 * H, 64, dtype=BF)
    w2b[:H, :8] = sb(bq)
    w2b[2 * H:, 8:16] = sb(bv)
    w2a = torch.zeros(H, 64, dtype=BF)
    w2a[:, :8], w2a[:, 8:16] = aq.T, av.T
    bt = torch.cat([bq.T, bv.T], 0)
    if mut == "bv_into_q_block":
        w2b[:H, :8] = sb(bv)
    if mut == "scale_missing":
        w2b[:H, :8], w2b[2 * H:, 8:16] = bq, bv
    out = {"w2b": w2b.to(F64), "w2a": w2a.to(F64), "bt": bt.contiguous().to(F64)}
    return out, {}


def pack_mutants(case):
    return ["bv_into_q_block", "scale_missing"]


# ----------------------------------------------------------------------------------------------- transpose_pad, swiglu_bwd, act_bwd
def tp_inputs(case):
    return dict(x=torch.randn(case.rows, case.ld_in, generator=_g(case)).to(BF))


def tp_compute(case, inp, mut=None, emu=None):
    out = torch.zeros(case.cols, case.pad, dtype=F64)
    out[:, :case.rows] = inp["x"][:, :case.cols].to(F64).T
    if mut == "last_row_dropped":
        out[:, case.rows - 1] = 0
    return {"out": out}, {}


def swiglu_inputs(case):
    g = _g(case)
    return dict(gu=(torch.randn(case.rows, 2 * case.I, generator=g) * 1.5).to(BF), dout=torch.randn(case.rows, case.I, generator=g).to(BF))


def swiglu_compute(case, inp, mut=None, emu=None):
    I = case.I
    gu, d = _T(inp["gu"], emu), _T(inp["dout"], emu)
    gt, up = (gu[:, I:], gu[:, :I]) if mut == "gate_up_swapped" else (gu[:, :I], gu[:, I:])
    sg = torch.sigmoid(gt)
    dsilu = sg if mut == "silu_derivative_term_missing" else sg * (1 + gt * (1 - sg))
    dg, du = d * up * dsilu, d * gt * sg
    out = torch.cat([du, dg], 1) if mut == "gate_up_swapped" else torch.cat([dg, du], 1)
    return {"dgu": _rb(out, emu).to(F64)}, {}


def act_inputs(case):
    g = _g(case)
    pre = torch.randn(case.n, generator=g) * 2.0
    y = (torch.relu(pre) if case.act == "relu" else torch.sigmoid(pre)).to(BF)
    return dict(dy=torch.randn(case.n, generator=g).to(BF), y=y, pre=pre.to(BF))


def act_compute(case, inp, mut=None, emu=None):
    dy = _T(inp["dy"], emu)
    y = _T(inp["pre"] if mut == "derivative_from_preactivation" else inp["y"], emu)
    out = dy * ((y >= 0) if mut == "relu_passes_at_zero" else (y > 0)) if case.act == "relu" else dy * y * (1 - y)
    return {"out": _rb(out, emu).to(F64)}, {}


# -------------------------------------------------------------------------------------------------------- softmax_rows + attn_ds
def sd_inputs(case):
    g = _g(case)
    BH, T, ld = case.BH, case.T, case.ld
    km = None
    if case.mask:
        km = torch.ones(BH // case.heads, T, dtype=torch.uint8)
        km[0, T // 2:] = 0
        km[1, :] = 0                                                       # one batch entry fully masked
    return dict(S=torch.randn(BH, T, ld, generator=g) * 8.0, dP=torch.randn(BH, T, ld, generator=g), km=km, scale=0.25)


def sd_compute(case, inp, mut=None, emu=None):
    """P = softmax_rows(S) (bf16 form, padding and fully masked rows exactly zero); dS = attn_ds(bf16 P of the reference, dP)"""
    BH, T, ld = case.BH, case.T, case.ld
    sc = float(np.float32(inp["scale"]))
    s = _T(inp["S"][..., :T], emu) * sc
    ok = torch.ones(BH, T, T, dtype=torch.bool)
    if case.causal:
        kk, qq = torch.arange(T)[None, :], torch.arange(T)[:, None]
        ok &= ((kk < qq) if mut == "causal_k_lt_q" else (kk <= qq))[None]
    if inp["km"] is not None:
        km = torch.roll(inp["km"], 1, 0) if mut == "mask_of_b_on_b+1" else inp["km"]
        ok &= (km != 0).repeat_interleave(case.heads, 0)[:, None, :]
    sm = s.masked_fill(~ok, -INF)
    mx = sm.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(sm - mx)
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / l, torch.zeros_like(e))
    P = torch.zeros(BH, T, ld, dtype=p.dtype)
    P[..., :T] = p
    # attn_ds is handed the reference's P rounded to bf16 (the GPU test does the same), so its check does not inherit the softmax's error
    pb = sd_reference_P(case).to(BF)
    pp, dp = _T(pb[..., :T], emu), _T(inp["dP"][..., :T], emu)
    dl = torch.zeros_like(pp[..., :1]) if mut == "delta_dropped" else (pp * dp).sum(-1, keepdim=True)
    dS = torch.zeros(BH, T, ld, dtype=pp.dtype)
    dS[..., :T] = (1.0 if mut == "scale_missing" else sc) * pp * (dp - dl)
    P, dS = _rb(P, emu).to(F64), _rb(dS, emu).to(F64)
    if mut == "padding_holds_1e-4":
        P[..., T:], dS[..., T:] = 1e-4, 1e-4
    if mut == "masked_entries_hold_1e-4":
        P[..., :T][~ok], dS[..., :T][~ok] = 1e-4, 1e-4
    return {"P": P, "dS": dS}, {}


@functools.lru_cache(maxsize=None)
def sd_reference_P(case):
    inp = inp_cached(case)
    T = case.T
    s = inp["S"][..., :T].to(F64) * float(np.float32(inp["scale"]))
    ok = torch.ones(case.BH, T, T, dtype=torch.bool)
    if case.causal:
        ok &= (torch.arange(T)[None, :] <= torch.arange(T)[:, None])[None]
    if inp["km"] is not None:
        ok &= (inp["km"] != 0).repeat_interleave(case.heads, 0)[:, None, :]
    p = torch.nan_to_num(torch.softmax(s.masked_fill(~ok, -INF), -1), nan=0.0)
    P = torch.zeros(case.BH, T, case.ld, dtype=F64)
    P[..., :T] = p
    return P


def sd_mutants(case):
    m = ["delta_dropped", "scale_missing"]
    if case.ld > case.T:
        m.append("padding_holds_1e-4")
    if case.causal or case.mask:
        m.append("masked_entries_hold_1e-4")
    if case.causal:
        m.append("causal_k_lt_q")
    if case.mask:
        m.append("mask_of_b_on_b+1")
    return m


# ----------------------------------------------------------------------------------------------------------------------- registry
OPS = {
    "norm_bwd": (norm_inputs, norm_compute, norm_mutants),
    "colsum": (colsum_inputs, colsum_compute, colsum_mutants),
    "ce": (ce_inputs, ce_compute, ce_mutants),
    "scatter_add": (scatter_inputs, scatter_compute, scatter_mutants),
    "sumsq": (sumsq_inputs, sumsq_compute, sumsq_mutants),
    "adamw": (adamw_inputs, adamw_compute, adamw_mutants),
    "lora_down": (lora_down_inputs, lora_down_compute, lora_down_mutants),
    "lora_outer": (outer_inputs, outer_compute, outer_mutants),
    "lora_wgrads": (outer_inputs, outer_compute, outer_mutants),
    "lora_apply": (apply_inputs, apply_compute, apply_mutants),
    "lora_pack": (pack_inputs, pack_compute, pack_mutants),
    "transpose_pad": (tp_inputs, tp_compute, lambda c: ["last_row_dropped"]),
    "swiglu_bwd": (swiglu_inputs, swiglu_compute, lambda c: ["gate_up_swapped", "silu_derivative_term_missing"]),
    "act_bwd": (act_inputs, act_compute, lambda c: ["relu_passes_at_zero"] if c.act == "relu" else ["derivative_from_preactivation"]),
    "softmax_ds": (sd_inputs, sd_compute, sd_mutants),
}
EXACT_OPS = ("transpose_pad", "lora_pack")          # bit for bit: the bound is zero


@functools.lru_cache(maxsize=4)
def inp_cached(case):
    return OPS[case.op][0](case)


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> (inputs, fp64 reference outputs, per-element bounds); built once per case (the 7656 x 4096 references are not rebuilt per mutant)"""
    inp = inp_cached(case)
    ref, aux = OPS[case.op][1](case, inp)
    bounds = {}
    for n, r in ref.items():
        if case.op in EXACT_OPS or (case.op == "lora_down" and n in ("w2b", "w2a", "bt")):
            bounds[n] = torch.zeros(())
        elif n in aux:
            bounds[n] = f32_bound(*aux[n], c=C_ELEM if case.op == "adamw" else None)
        else:
            bounds[n] = torch.where(r == 0, torch.zeros_like(r), torch.nan_to_num(bf16_bound(r), nan=0.0))       # structural zeros and sentinels: exact
    return inp, ref, bounds


def emulation_ratios(case):
    """worst tolerance ratio per output of the two emulations (fp32 terms, summed one after the other / as the kernel's slices folded in order)"""
    inp, ref, bounds = reference(case)
    out = {}
    for order in ("seq", "sliced"):
        got, _ = OPS[case.op][1](case, inp, emu=order)
        for n, r in ratios(got, ref, bounds).items():
            out[n] = max(out.get(n, 0.0), r)
    return out


def mutant_names(case):
    return [] if case.einval else list(OPS[case.op][2](case))


def mutant_ratios(case):
    """mutant -> its worst tolerance ratio over the outputs against the fp64 reference"""
    inp, ref, bounds = reference(case)
    out = {}
    for name in mutant_names(case):
        got, _ = OPS[case.op][1](case, inp, mut=name)
        out[name] = max(ratios(got, ref, bounds).values())
    return out
