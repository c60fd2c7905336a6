"""The GEMM kernels (llmseg_amd/csrc/gemm.hip behind gemm_plan.h) at their tile, K-slice, stride and epilogue edges: a case table, input builders, fp64
references, PER-ELEMENT bounds, fp32 / bf16 emulations of what the kernels round, and mutants (fp64 results of slightly wrong problems) the bounds must reject.

Everything here runs on the CPU (no import of the HIP library).  tests/test_gemm_kernels_cpu.py proves on every case that the emulations stay at <= EMU_MAX of
the bound and that every applicable mutant exceeds it by >= MUT_MIN, and feeds each case's GemmQuery line (`query_line`, the format of tests/gemm_plan_checks.py)
to the real gemm_plan.h: the route, kernel, slice count, extension mode, reduce kernel, fused epilogue and launch count a case DECLARES must be the plan's.
tests/test_gemm_kernels_gpu.py holds the kernels to the same bounds through llmseg_amd.ops.

The bound of one output element, with T the fp64 sum of the absolute values of its n terms,
    T = |gamma| (|alpha| (sum_k |a_k w_k| + sum |a2 w2|) + |bias|) + |residual| + |old C|            (the last with `accumulate`)
  fp32 outputs:  |got - ref| <= C_SUM 2^-24 sqrt(n) T
  bf16 outputs:  |got - ref| <= C_BF16 2^-8 |ref| + C_SUM 2^-24 sqrt(n) T
Where a route rounds an INTERMEDIATE to bf16 (the first launch of EXT_SECOND; the product under a fused tail: RoPE, SwiGLU, SwiGLU backward, the norm_out and
delta reduces, the norm-backward reduce) the reference stays the exact fp64 function of the exact product and the bound gains C_MID 2^-8 S, S = sum_i |d out / d x_i| |x_i| over the
rounded intermediates x_i (for EXT_SECOND simply |intermediate|).
The skinny kernel's A-row transforms round A' to bf16 from fp32 arithmetic, and the reference restates those roundings in fp64 with no allowance in the
bound.  A rounding is discontinuous at a tie, so the INPUTS are built to stay clear of ties: `inputs` zeroes the few elements whose pre-rounding value lies
within TIE_MARGIN (relative) of the midpoint of two bf16 neighbours (see `_clear_of_ties`)."""
import functools
import math

import torch

from tests import gemm_plan_checks as gp
from tests.backward_kernel_checks import C_BF16, C_SUM, EMU_MAX, FILL, MUT_MIN, Case, cdiv, ratio  # noqa: F401  (re-exported to the two test files)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
EPS = 1e-6
C_MID = 1.9                   # weight of a bf16-rounded intermediate (half an ulp is 2^-8 |x|).  With 1 the emulations of EXT_SECOND reach 0.87, of the fused RoPE 0.78,
                              # of SwiGLU (backward) 0.63, of norm_out 0.54: a correctly rounded intermediate alone uses up all of a 1 x 2^-8 |x| term.  The smallest
                              # value for which every emulation stays <= EMU_MAX is 1.862 (EXT_SECOND on the 128 x 128 DMA kernel, M = 257), rounded up to one decimal
TIE_MARGIN = 2.0 ** -16       # input conditioning of the A-row transforms, not part of any bound: about 0.4 % of the elements are zeroed
ACTS = ("none", "relu", "gelu", "quickgelu", "silu", "sigmoid")          # index = LLMSEG_ACT_*
KERNELS = {0: "reg", 2: "glds", 8: "pp256", 9: "pp128", 10: "t160"}      # llmseg_gemm_set_variant's low bits -> the plan's kernel name
ROWS = {0: 128, 2: 128, 8: 256, 9: 128, 10: 160}
FX = {"rope": gp.FX_ROPE, "swiglu": gp.FX_SWIGLU, "swiglu_bwd": gp.FX_SWIGLU_BWD}

DEFAULTS = dict(v=5, S=0, ta=0, tw=0, f32=0, acc=0, bias=0, gamma=0, res=0, act=0, alpha=1.0, ext=None, lda2=64, lda_pad=0, ldw_pad=0, ldc_pad=0, ldr_pad=0,
                off_c=0, off_r=0, off_b=0, off_g=0, b1=1, b2=1, w_bcast=0, sc_gap=0, a_norm=0, a_swiglu=0, tail=None, fx_cols=0, T=0, dres=0,
                slices=1, ext_mode="none", reduce="none", fx=0, rows=0, ksplit=0, cpt=0)


def r8(x):
    return (x + 7) // 8 * 8


def G(group, name, M, N, K, route, kernel, launches=None, **kw):
    """One case: the call (shape + DEFAULTS' keys) and the plan it was written for (route, kernel, slices, ext_mode, reduce, fx, launches; rows / ksplit / cpt)"""
    assert not set(kw) - set(DEFAULTS), set(kw) - set(DEFAULTS)
    p = dict(DEFAULTS, **kw)
    if launches is None:
        launches = 2 if p["slices"] > 1 else 1
    return Case("gemm", f"{group}-{name}", launches, group=group, M=M, N=N, K=K, route=route, kernel=kernel, **p)


def _o(i, **cycle):
    """the i-th choice of each keyword's list (pairwise coverage by walking lists of coprime lengths)"""
    return {k: v[i % len(v)] for k, v in cycle.items()}


# ------------------------------------------------------------------------------------------------------------------------------ the table
def _group_a():
    cs = []
    Ns = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 320)
    for v in (0, 2, 8, 9):
        bm = ROWS[v]
        Ms = (1, 9, 31, 32, 33, bm - 1, bm, bm + 1, bm + 33, 2 * bm + 1)
        route = {0: "reg", 2: "glds", 8: "pp", 9: "pp"}[v]
        for j, N in enumerate(Ns):
            M, K, f32 = Ms[(j * 3 + v) % 10], (128, 192)[j % 2], (j // 2 + v) % 2
            cs.append(G("A", f"{KERNELS[v]}-{M}x{N}x{K}-{'f32' if f32 else 'bf16'}", M, N, K, route, KERNELS[v], v=v, f32=f32))
    for j, N in enumerate((1, 65, 128, 258)):
        cs.append(G("A", f"glds-k64-{(33, 127, 129, 257)[j]}x{N}x64", (33, 127, 129, 257)[j], N, 64, "glds", "glds", v=2, f32=j % 2))
    Ms = (1, 9, 31, 32, 33, 159, 160, 161, 193, 321)          # the 160 x 256 tile: K-slices only, so N % 4 == 0
    for j, M in enumerate(Ms):
        N = (4, 64, 128, 256, 320, 260, 68, 132, 252, 324)[j]
        cs.append(G("A", f"t160-{M}x{N}x256-{'f32' if j % 2 else 'bf16'}", M, N, 256, "pp_sliced", "t160", v=10, S=2, slices=2, reduce="plain", f32=j % 2))
    # N % 4 != 0 where the cost model would slice K (129 x 256 x 4096 runs as 16 slices): the one-slice fallback
    cs.append(G("A", "auto-n_not_4-129x258x4096", 129, 258, 4096, "pp", "pp128"))
    cs.append(G("A", "auto-129x256x4096", 129, 256, 4096, "pp_sliced", "pp128", slices=16, reduce="plain"))
    return cs


def _group_b():
    cs = []
    for j, K in enumerate((8, 24, 56, 64, 72, 120, 136, 200)):
        cs.append(G("B", f"reg-k{K}", 130, 70, K, "reg", "reg", v=0 if K % 64 == 0 else 5, f32=j % 2))
    for K in (20, 67):                                        # ld = roundup8(K), the padding zeroed
        cs.append(G("B", f"reg-kpad{K}", 130, 70, K, "reg", "reg", f32=int(K == 67)))
    for ta, tw in ((0, 1), (1, 0), (1, 1)):
        for j, K in enumerate((1, 3, 4, 5, 63, 65, 300)):
            cs.append(G("B", f"reg-t{ta}{tw}-k{K}", 67, 45, K, "reg", "reg", ta=ta, tw=tw, f32=(j + ta) % 2))
    for ta, tw, M, N, K in ((1, 0, 65, 45, 65), (0, 1, 67, 63, 63), (1, 1, 72, 72, 72)):      # square stored operands: a transposed read must differ from a plain one
        cs.append(G("B", f"reg-t{ta}{tw}-square-{M}x{N}x{K}", M, N, K, "reg", "reg", ta=ta, tw=tw))
    # register staging as K-slices: 32 K-tiles as 16 slices of 2 (the pinned head dW shape); 35 K-tiles as 12 slices of 3 with 2 in the last; K % 64 != 0
    cs.append(G("B", "reg_sliced-136x72x2048", 136, 72, 2048, "reg_sliced", "reg", ta=1, tw=1, f32=1, slices=16, reduce="plain"))
    cs.append(G("B", "reg_sliced-short_last-136x72x2240", 136, 72, 2240, "reg_sliced", "reg", ta=1, tw=1, f32=1, slices=12, reduce="plain"))
    cs.append(G("B", "reg_sliced-k_not_64-136x72x2000", 136, 72, 2000, "reg_sliced", "reg", tw=1, slices=16, reduce="plain"))
    for v in (8, 9):
        for K in (128, 320):
            cs.append(G("B", f"{KERNELS[v]}-k{K}", 257, 260, K, "pp", KERNELS[v], v=v))
        cs.append(G("B", f"{KERNELS[v]}-k64-ext", 257, 260, 64, "pp", KERNELS[v], v=v, ext="dense", ext_mode="ktile"))
    for v in (8, 9, 10):
        # 21 K-tiles in 4 slices: 6, 6, 6, 3;  5 in 2: 3 + 2;  20 in 10 slices of 2: one more slice would leave the last one empty (split_ok's limit)
        for K, S in ((1344, 4), (320, 2), (1280, 10)):
            cs.append(G("B", f"{KERNELS[v]}-s{S}-k{K}", 161, 260, K, "pp_sliced", KERNELS[v], v=v, S=S, slices=S, reduce="plain", f32=int(K == 320)))
    return cs


SKINNY_N = (1, 3, 4, 5, 15, 16, 17, 37)
SKINNY_K = (8, 16, 504, 512, 520, 1016, 1024, 1032, 2040, 2048, 2056, 4104)


def _skinny_rows(M):
    return 1 if M == 1 else 2 if M == 2 else 4 if M <= 4 else 8


def _group_c():
    cs = []
    i = 0
    for Ms in ((1,), (2,), (3, 4), (5, 6, 7, 8)):
        for j, K in enumerate(SKINNY_K):
            M, N = Ms[j % len(Ms)], SKINNY_N[(j + i) % 8]
            epi = (dict(), dict(bias=1, act=2 + j % 4, gamma=1, res=1, alpha=0.5), dict(f32=1, acc=1, bias=1), dict(lda_pad=24, res=1, ldr_pad=3))[(j + i) % 4]
            cs.append(G("C", f"m{M}-n{N}-k{K}-e{(j + i) % 4}", M, N, K, "skinny", "skinny", rows=_skinny_rows(M), ksplit=int(K >= 2048), **epi))
            i += 1
        for j, K in enumerate((2040, 2048, 2056, 4104)):      # more than 8192 columns: the plain kernel at long K
            M = Ms[-1 - j % len(Ms)]
            cs.append(G("C", f"m{M}-n8196-k{K}", M, 8196, K, "skinny", "skinny", rows=_skinny_rows(M), ksplit=0, f32=j % 2, bias=j // 2))
    j = 0
    for Ms in ((1,), (2,), (3, 4), (5, 6, 7, 8)):             # every row template of both A-row transforms, plain and K-split
        for sk in (0, 1):
            Kn, Ks = ((520, 16, 504, 1032), (2056, 4104, 2048, 2056))[sk][j % 4], ((512, 24, 1016, 520), (2048, 2056, 4104, 2048))[sk][j % 4]
            M, M2, N = Ms[j % len(Ms)], Ms[-1 - j % len(Ms)], SKINNY_N[(j + 3) % 8]
            # fp32 output: nothing hides the transform's own error (a rstd over K - 8 columns moves a long row's bf16 elements by less than an ulp)
            cs.append(G("C", f"a_norm-m{M}-n{N}-k{Kn}", M, N, Kn, "skinny", "skinny", rows=_skinny_rows(M), ksplit=sk, a_norm=1, f32=1, lda_pad=8 * (j % 2)))
            cs.append(G("C", f"a_swiglu-m{M2}-n{N}-k{Ks}", M2, N, Ks, "skinny", "skinny", rows=_skinny_rows(M2), ksplit=sk, a_swiglu=1, res=j % 2, lda_pad=8 + 8 * (j % 3)))
            j += 1
    return cs


def _on(v, **kw):
    """route / kernel / forced split of `the kernel v` for the stride, epilogue and batch groups; v = "red" is the plain reduce behind two slices of 128 x 256"""
    if v == "red":
        return dict(route="pp_sliced", kernel="pp128", v=9, S=2, slices=2, reduce="plain", **kw)
    return dict(route={0: "reg", 2: "glds", 8: "pp", 9: "pp"}[v], kernel=KERNELS[v], v=v, **kw)


def _group_d():
    cs = []
    for v in (0, 2, 9, "red"):
        K = 320 if v == "red" else 128
        tag = "red" if v == "red" else KERNELS[v]
        pads = (4, 8) if v == "red" else (1, 2, 4, 8)        # the K-sliced route needs ldc % 4 == 0
        var = [("views", dict(lda_pad=8, ldw_pad=16, f32=1))]
        var += [(f"ldc+{p}", dict(ldc_pad=p, f32=i % 2, res=1, ldr_pad=0)) for i, p in enumerate(pads)]
        var += [("off_c", dict(off_c=1, bias=1)), ("off_c-f32", dict(off_c=1, f32=1, acc=1)), ("off_r", dict(off_r=1, res=1)), ("off_b", dict(off_b=1, bias=1, gamma=1)),
                ("off_g", dict(off_g=1, gamma=1, bias=1, res=1)), ("ldr+8", dict(res=1, ldr_pad=8, ldc_pad=4))]
        if v != "red":
            var.append(("ldr_odd", dict(res=1, ldr_pad=3, ldc_pad=4)))
        for name, kw in var:
            cs.append(G("D", f"{tag}-{name}", 130, 132, K, **_on(v, **kw)))
    # what makes can_split false on a shape the cost model slices: the one-slice plan it falls back to
    cs.append(G("D", "auto-ldc_not_4", 129, 256, 4096, "pp", "pp128", ldc_pad=2))
    cs.append(G("D", "auto-ldr_not_4", 129, 256, 4096, "pp", "pp128", res=1, ldr_pad=3))
    return cs


def _group_e():
    cs = []
    forms = (("interior", 9, 256, 256, 128), ("edge", 9, 300, 520, 256), ("edge-glds", 2, 300, 520, 64), ("edge-reg", 0, 300, 520, 200), ("skinny", 5, 5, 520, 256),
             ("reduce", "red", 300, 520, 256), ("reduce-interior", "red", 256, 256, 256))
    for fi, (form, v, M, N, K) in enumerate(forms):
        on = dict(route="skinny", kernel="skinny", rows=8) if form == "skinny" else dict(route="reg", kernel="reg") if form == "edge-reg" else _on(v)
        for a in range(6):
            # four epilogue operands, pairwise over the six activations: each operand on in half the cases, each pair in every combination
            o = _o(a + fi, bias=(1, 0, 1, 0, 1, 1), gamma=(0, 1, 1, 0, 0, 1), res=(1, 1, 0, 0, 1, 0), alpha=(0.5, 1.0, 1.0, 0.5, 1.0, 0.5))
            cs.append(G("E", f"{form}-{ACTS[a]}-b{o['bias']}g{o['gamma']}r{o['res']}a{o['alpha']}", M, N, K, act=a, **o, **on))
        # fp32 and fp32 `+=` output: ReLU is exact in fp32; the other activations' approximations (__expf, rcp, the A&S erf) are covered by bf16 rounding only
        cs.append(G("E", f"{form}-f32-relu-full", M, N, K, act=1, f32=1, bias=1, gamma=1, res=1, alpha=0.5, **on))
        cs.append(G("E", f"{form}-f32acc-full", M, N, K, f32=1, acc=1, bias=1, gamma=1, res=1, alpha=0.5, **on))
        cs.append(G("E", f"{form}-f32acc-plain", M, N, K, f32=1, acc=1, **on))
    return cs


def _group_f():
    cs = []
    for v in (0, 2, 8):
        tag = KERNELS[v]
        cs.append(G("F", f"{tag}-3x1-f32", 70, 132, 128, b1=3, f32=1, **_on(v)))
        cs.append(G("F", f"{tag}-2x3-bf16-gap", 70, 132, 128, b1=2, b2=3, sc_gap=256, **_on(v)))
        cs.append(G("F", f"{tag}-2x3-f32-w_bcast-sc_not_4", 129, 65, 192, b1=2, b2=3, f32=1, w_bcast=1, sc_gap=2, **_on(v)))
        cs.append(G("F", f"{tag}-3x1-bf16-w_bcast-ldc", 257, 130, 128, b1=3, w_bcast=1, ldc_pad=2, sc_gap=6, **_on(v)))
    cs.append(G("F", "reg_sliced-2x1", 128, 128, 2048, "reg_sliced", "reg", tw=1, b1=2, f32=1, sc_gap=128, slices=16, reduce="plain"))
    cs.append(G("F", "reg_sliced-3x1-bf16", 70, 132, 1024, "reg_sliced", "reg", ta=1, b1=3, slices=8, reduce="plain"))
    return cs


def _group_g():
    cs = []
    for j, M in enumerate((127, 128, 129, 257)):
        e = dict(ext=("dense", "16")[j % 2], lda2=(64, 72)[(j // 2) % 2])
        cs.append(G("G", f"ktile-pp128-m{M}", M, 260, 128, "pp", "pp128", v=9, ext_mode="ktile", res=j % 2, **e))
        cs.append(G("G", f"ktile-pp256-m{M}", M, 260, 192, "pp", "pp256", v=8, ext_mode="ktile", bias=1, act=4 * (j % 2), lda2=e["lda2"], ext=("16", "dense")[j % 2]))
        cs.append(G("G", f"slab-pp128-m{M}", M, 260, 320, "pp_sliced", "pp128", 3, v=9, S=2, slices=2, reduce="plain", ext_mode="slab", bias=j % 2, **e))
        cs.append(G("G", f"second-glds-m{M}", M, 260, 128, "glds", "glds", 2, v=2, ext_mode="second", bias=1, res=1, alpha=(1.0, 0.5)[j % 2], **e))
    cs.append(G("G", "slab-t160-m161", 161, 260, 320, "pp_sliced", "t160", 3, v=10, S=2, slices=2, reduce="plain", ext_mode="slab", ext="dense", lda2=72))
    cs.append(G("G", "second-reg-m200", 200, 264, 200, "reg", "reg", 2, ext_mode="second", ext="16", res=1))
    return cs


def _group_h():
    cs = []
    on = dict(route="pp", kernel="pp128", v=9, fx=1)
    for M, N, cols, T in ((1, 256, 128, 1), (127, 256, 256, 7), (129, 256, 256, 129), (127, 512, 128, 127), (129, 512, 512, 7), (1, 512, 256, 7), (129, 512, 256, 129)):
        cs.append(G("H", f"rope-{M}x{N}-cols{cols}-T{T}", M, N, 128, tail="rope", fx_cols=cols, T=T, ext="16", ext_mode="ktile", **on))
    for M in (127, 129):
        cs.append(G("H", f"swiglu-{M}x512", M, 512, 128, tail="swiglu", **on))
    for j, N in enumerate((64, 192, 320, 256)):              # N % 256 != 0: the last column tile of d(out) is ragged
        cs.append(G("H", f"swiglu_bwd-{(129, 127, 130, 129)[j]}x{N}", (129, 127, 130, 129)[j], N, 128, tail="swiglu_bwd", **on))
    red = dict(route="pp_sliced", kernel="pp128", v=9, S=2, slices=2)
    for M in (64, 65):
        for N, cpt in ((2048, 1), (4096, 2), (8192, 4)):
            cs.append(G("H", f"norm-{M}x{N}", M, N, 256, tail="norm", res=int(N != 4096), reduce="norm", cpt=cpt, **red))
            cs.append(G("H", f"nb-{M}x{N}", M, N, 256, tail="nb", dres=int(N != 2048), reduce="nb", **red))
            T = {64: (16, 64, 8), 65: (13, 5, 65)}[M][cpt >> 1]
            cs.append(G("H", f"dl-{M}x{N}-T{T}", M, N, 256, tail="dl", T=T, reduce="dl", cpt=cpt, alpha=(1.0, 0.5)[M & 1], **red))
    return cs


@functools.lru_cache(maxsize=1)
def cases():
    out = _group_a() + _group_b() + _group_c() + _group_d() + _group_e() + _group_f() + _group_g() + _group_h()
    # A bf16 output of a handful of elements need not show one missing term of K (see mutant_names): each such call runs once more with fp32 output, which does
    out += [G(c.group, c.name[len(f"gemm-{c.group}-"):] + "-f32twin", c.M, c.N, c.K, c.route, c.kernel, c.launches, **dict({k: c.p[k] for k in DEFAULTS}, f32=1))
            for c in out if not c.f32 and c.M * c.N < 64]
    assert len({c.name for c in out}) == len(out), "duplicate case name"
    return out


# ------------------------------------------------------------------------------------------------------------------------- the query line
def dims(case):
    """ldc, ldr, sC (elements between batch entries of C), batch count, the C row count the call may write and its column count"""
    wide = 2 * case.N if case.tail == "swiglu_bwd" else case.N
    ldc = wide + case.ldc_pad
    ldr = case.N + case.ldr_pad if case.res else 0
    B = case.b1 * case.b2
    sC = case.M * ldc + case.sc_gap if B > 1 else 0
    return ldc, ldr, sC, B, wide


def query_line(case):
    """what llmseg_amd.ops.gemm / gemm_batched hand to gemm_dispatch for this case, as a line of tests/gemm_plan_main.cpp's input"""
    ldc, ldr, sC, B, _ = dims(case)
    kw = dict(batch1=case.b1, batch2=case.b2, trans_a=case.ta, trans_w=case.tw, out_f32=case.f32, bias=case.bias, gamma=case.gamma, residual=case.res, act=case.act,
              alpha_one=int(case.alpha == 1.0), ext=int(case.ext is not None), a_norm=case.a_norm, a_swiglu=case.a_swiglu, ldc=ldc, ldr=ldr, stride_c=sC,
              ws=int(case.K >= 256 and case.b2 <= 1), variant=case.v, split=case.S, norm_ptrs_aligned=int(case.tail == "norm"))
    if case.tail == "norm":
        kw["tail"] = gp.TAIL_NORM
    elif case.tail == "dl":
        kw["tail"] = gp.TAIL_DL
    elif case.tail == "nb":
        kw["tail"] = gp.TAIL_NB
    elif case.tail:
        kw["fx"] = FX[case.tail]
    return gp.query(case.name, case.M, case.N, case.K, **kw)


def declared(case):
    """the plan fields a case declares, as the plan program prints them"""
    d = dict(route=case.route, kernel=case.kernel, slices=case.slices, ext=case.ext_mode, reduce=case.reduce, fx=case.fx, launches=case.launches)
    if case.route == "skinny":
        d.update(rows=case.rows, ksplit=case.ksplit)
    if case.reduce in ("norm", "dl"):
        d["cpt"] = case.cpt
    return {k: str(v) for k, v in d.items()}


def skinny_template(case):
    return (1 if case.a_norm else 2 if case.a_swiglu else 0, case.ksplit, case.rows)


# ---------------------------------------------------------------------------------------------------------------------------------- inputs
def inputs(case):
    """the operands as they lie in memory (bf16 unless said), padding and the elements between rows included"""
    g = torch.Generator().manual_seed(case.seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF)
    M, N, K = case.M, case.N, case.K
    ldc, ldr, sC, B, wide = dims(case)
    inp = {}
    rows_a, cols_a = (K, M) if case.ta else (M + 1, 2 * K if case.a_swiglu else K)        # one more row than the call knows of (the skinny kernel clamps rows)
    a = rn(B, rows_a, r8(cols_a) + case.lda_pad)
    rows_w, cols_w = (K, N) if case.tw else (N, K)
    w = rn(1 if case.w_bcast else B, rows_w, r8(cols_w) + case.ldw_pad, scale=K ** -0.5)
    if not case.ta:
        a[..., cols_a:r8(cols_a)] = 0           # K % 8 != 0: the dispatch asks for zeros up to the next multiple of 8; anything may follow
    if not case.tw:
        w[..., cols_w:r8(cols_w)] = 0
    if case.a_norm or case.a_swiglu:
        inp["zeroed"] = torch.tensor(_clear_of_ties(case, a))
    inp["a"], inp["w"] = a, w
    if case.bias:
        inp["bias"] = rn(N + 1)
    if case.gamma:
        inp["gamma"] = (1.0 + 0.25 * torch.randn(N + 1, generator=g)).to(BF)
    if case.res:
        inp["res"] = rn(M * max(ldr, ldc) + N + 8)
    if case.ext:
        a2, w2 = rn(M, case.lda2, scale=0.5), rn(N, 64, scale=0.125)
        if case.ext == "16":
            a2[:, 16:64] = 0
        inp["a2"], inp["w2"] = a2, w2
    if case.a_norm:
        inp["anw"] = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF)
    if case.tail == "norm":
        inp["nw"] = (1.0 + 0.1 * torch.randn(N, generator=g)).to(BF)
    elif case.tail == "dl":
        inp["o"] = rn(M, N, scale=0.5)
    elif case.tail == "nb":
        inp["nx"], inp["nbw"] = rn(M, N), (1.0 + 0.1 * torch.randn(N, generator=g)).to(BF)
        if case.dres:
            inp["dres"] = rn(M, N, scale=0.2)
    elif case.tail == "rope":
        th = torch.rand(case.T, 64, generator=g, dtype=F64) * (2 * math.pi)
        inp["cos"], inp["sin"] = th.cos().to(F32), th.sin().to(F32)
    elif case.tail == "swiglu_bwd":
        inp["gu"] = rn(M, 2 * N)
    return inp


def _clear_of_ties(case, a):
    """Zeroes, in place, the elements of the rows the call reads whose transformed value would be rounded to bf16 within TIE_MARGIN of a tie: x where x * rstd
    is (a_norm; rstd moves with them, hence the loop), `up` where silu(gate) * up is (a_swiglu).  fp32 arithmetic may round such an element the other way than
    fp64 does, and one bf16 ulp of one A' element is far beyond the fp32 bound.  A zero transforms to an exact zero.  -> the number of elements zeroed"""
    M, K, n = case.M, case.K, 0
    for _ in range(20):
        x = a[0, :M].to(F64)
        y = x[:, :K] * torch.rsqrt(x[:, :K].pow(2).mean(-1, keepdim=True) + EPS) if case.a_norm else x[:, :K] * torch.sigmoid(x[:, :K]) * x[:, K:2 * K]
        tie = _near_tie(y)
        if not tie.any():
            return n
        n += int(tie.sum())
        (a[0, :M, :K] if case.a_norm else a[0, :M, K:2 * K])[tie] = 0
    raise AssertionError(f"{case.name}: the inputs do not settle clear of bf16 ties")


def residual_view(case, inp, ld=None):
    ldc, ldr, _, _, _ = dims(case)
    return inp["res"].as_strided((case.M, case.N), (ldr if ld is None else ld, 1), case.off_r)


# ------------------------------------------------------------------------------------------------------------- activations and roundings
def act_ref(v, a):
    if a == 1:
        return v.clamp(min=0)
    if a == 2:
        return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    if a == 3:
        return v * torch.sigmoid(1.702 * v)
    if a == 4:
        return v * torch.sigmoid(v)
    if a == 5:
        return torch.sigmoid(v)
    return v


def act_emu(v, a):
    """apply_act's formulas (llmseg_amd/csrc/common.h) in fp32"""
    one = torch.ones((), dtype=F32)
    if a == 1:
        return v.clamp(min=0)
    if a == 2:
        z = v.abs() * 0.70710678118654752
        t = one / (0.3275911 * z + 1)
        poly = t * (t * (t * (t * (t * 1.061405429 - 1.453152027) + 1.421413741) - 0.284496736) + 0.254829592)
        erfa = 1 - poly * torch.exp(-z * z)
        return 0.5 * v * (1 + torch.copysign(erfa, v))
    if a == 3:
        return v * (one / (1 + torch.exp(-1.702 * v)))
    if a == 4:
        return v * (one / (1 + torch.exp(-v)))
    if a == 5:
        return one / (1 + torch.exp(-v))
    return v


def _rb(t, emu):
    """a bf16 store of the kernels (emulation only: the reference keeps the exact value and the bound carries the rounding)"""
    return t.to(BF).to(t.dtype) if emu else t


def _silu(g, emu):
    return g / (1 + torch.exp(-g)) if emu else g * torch.sigmoid(g)


def _near_tie(y):
    """elements of y (fp64) within TIE_MARGIN (relative) of the midpoint of two bf16 neighbours"""
    a = y.abs()
    u = torch.exp2(torch.floor(torch.log2(a.clamp(min=1e-300))) - 7)          # a bf16 ulp at |y|
    f = a / u
    return ((f - torch.floor(f) - 0.5).abs() < TIE_MARGIN * f) & (a > 0)


# ------------------------------------------------------------------------------------------------------------------------------- compute
def _slice_tiles(case):
    """(K columns per accumulation tile, tiles per slice) of the route the case declares"""
    if case.route == "skinny":
        return 512, None
    nt = cdiv(case.K, 64)
    return 64, (cdiv(nt, case.slices) if case.slices > 1 else None)


def _product(case, A, W, emu):
    """A [B, M, K] x W [B | 1, N, K]^T.  Reference: fp64.  Emulation: fp32 per K-tile, the tiles of a slice one after the other, the slabs in slice order."""
    if not emu:
        return A @ W.transpose(-1, -2)
    tile, q = _slice_tiles(case)
    A, W = A.to(F32), W.to(F32)
    nt = cdiv(A.shape[-1], tile)
    q = q or nt
    total = None
    for s in range(0, nt, q):
        acc = None
        for t in range(s, min(s + q, nt)):
            part = A[..., t * tile:(t + 1) * tile] @ W[..., t * tile:(t + 1) * tile].transpose(-1, -2)
            acc = part if acc is None else acc + part
        total = acc if total is None else total + acc
    return total


def compute(case, inp, mut=None, emu=False):
    """-> (outputs, aux).  outputs: c [B, M, columns] and the tail's second output; aux (reference run only): T, n, S of the bound.
    Reference (fp64) by default; `mut` = the fp64 result of that wrong problem; `emu` = fp32 arithmetic in the kernel's order with its bf16 roundings."""
    M, N, K = case.M, case.N, case.K
    ldc, ldr, sC, B, wide = dims(case)
    D = F32 if emu else F64
    a, w = inp["a"].to(F64), inp["w"].to(F64)
    untr = mut == "transposed_read_untransposed"          # a square operand only
    A = (a[:, :, :M] if untr and M == K else a[:, :, :M].transpose(1, 2)) if case.ta else a[:, :M, :]
    W = (w[:, :, :N] if untr and N == K else w[:, :, :N].transpose(1, 2)) if case.tw else w[:, :, :K]
    if mut == "skinny_row_plus_1":
        A = a[:, 1:M + 1, :]
    if case.a_norm:                                   # A := bf16(gain * bf16(x * rstd)), llmseg_norm's two roundings
        x = A[..., :K].to(D)
        ss = (x[..., :K - 8] if mut == "a_norm_rstd_over_K-8" else x).pow(2).sum(-1, keepdim=True)
        y = x * torch.rsqrt(ss / K + EPS)
        A = (inp["anw"].to(D) * y.to(BF).to(D)).to(BF).to(F64)
    elif case.a_swiglu:                               # A := bf16(silu(gate) * up) of rows [gate | up]
        gate = A[..., :K].to(D)
        up = (A[..., K - 8:2 * K - 8] if mut == "a_swiglu_up_at_K-8" else A[..., K:2 * K]).to(D)
        y = _silu(gate, emu) * up
        A = y.to(BF).to(F64)
    else:
        A = A[..., :K]
    A = A.clone()
    if mut == "last_row_from_M-2":
        A[:, M - 1] = A[:, M - 2]
    if mut == "last_k8_dropped":
        A[..., max(K - 8, 0):] = 0
    if mut == "k_at_tile_boundary_dropped":
        A[..., 64 if K > 64 else 63] = 0
    if mut == "last_tile_of_last_slice_dropped":
        A[..., (cdiv(K, 64) - 1) * 64:] = 0
    if mut == "batch_uses_W0":
        W = W[:1]
    P = _product(case, A, W, emu)
    absP = A.abs() @ W.abs().transpose(-1, -2) if not (emu or mut) else None
    if mut == "slice1_first_tile_twice":
        q = _slice_tiles(case)[1] * 64
        P = P + A[..., q:q + 64] @ W[..., q:q + 64].transpose(-1, -2)
    alpha = case.alpha
    P2 = None
    if case.ext and mut != "ext_dropped":
        A2 = inp["a2"][:, :64].to(F64)
        if mut == "ext_from_row_m-1":
            A2 = A2.roll(1, 0)
        W2 = inp["w2"].to(F64)
        P2 = (A2.to(D) @ W2.to(D).t())[None]
        if absP is not None:
            absP = absP + (A2.abs() @ W2.abs().t())[None]
    second = case.ext_mode == "second"
    if P2 is not None and not second:
        P = P + P2                                    # one more K-tile / one more slab
    P = P.to(D)
    bias = inp["bias"][case.off_b:case.off_b + N].to(D) if case.bias else None
    gamma = inp["gamma"][case.off_g:case.off_g + N].to(D) if case.gamma else None
    if mut == "bias_shifted_one_column":
        bias = bias.roll(1)
    if mut == "gamma_shifted_one_column":
        gamma = gamma.roll(1)
    res = residual_view(case, inp, ldc if mut == "residual_read_with_ldc" else None).to(D)[None] if case.res else None
    old = FILL if case.acc else 0.0
    v = (P + bias) * alpha if mut == "alpha_after_bias" else P * alpha + bias if bias is not None else P * alpha
    if mut == "gamma_before_act":
        v = (act_emu if emu else act_ref)(v * gamma, case.act)
    else:
        v = (act_emu if emu else act_ref)(v, case.act)
        if gamma is not None:
            v = v * gamma
    if res is not None:
        v = v + res
    inter = None
    if second:                                        # the first launch stored bf16(v); the second adds alpha * A2 W2^T with C as its residual
        inter = v
        v = _rb(v, emu) + (P2.to(D) * alpha if P2 is not None else 0)
    if case.acc and mut != "accumulate_ignored":
        v = v + (2 * old if mut == "accumulate_twice" else old)
    fill = FILL if case.acc else NAN
    outs, aux = {}, {}
    if not (emu or mut):
        T = absP * abs(alpha)
        if bias is not None:
            T = T + bias.abs()
        if gamma is not None:
            T = T * gamma.abs()
        if res is not None:
            T = T + res.abs()
        T = T + abs(old)
        n = K + (64 if case.ext else 0) + case.bias + case.res + case.acc + (N if case.tail == "nb" else 0)
        aux = dict(T=T, n=n, S={}, fbw={})
        if inter is not None:
            aux["S"]["c"] = inter.abs()
    c = v
    # ---- the fused tails: exact functions of the exact product in the reference; the emulation rounds the product to bf16 first, as the kernels do
    if case.tail == "rope":
        cos, sin = inp["cos"].to(D), inp["sin"].to(D)
        pos = torch.arange(M) % case.T
        cm, sm = cos[pos][None, :, None, :], sin[pos][None, :, None, :]            # [1, M, 1, 64]
        x = _rb(c, emu)[..., :case.fx_cols].reshape(1, M, -1, 2, 64)
        lo, hi = x[..., 0, :], x[..., 1, :]
        rot = torch.stack((lo * cm - hi * sm, hi * cm + lo * sm), -2).reshape(1, M, case.fx_cols)
        c = torch.cat((rot, c[..., case.fx_cols:]), -1)
        if aux:
            Tx = aux["T"][..., :case.fx_cols].reshape(1, M, -1, 2, 64)
            ca, sa = cm.abs(), sm.abs()
            sens = lambda z: torch.stack((z[..., 0, :].abs() * ca + z[..., 1, :].abs() * sa, z[..., 1, :].abs() * ca + z[..., 0, :].abs() * sa), -2).reshape(1, M, case.fx_cols)
            aux["S"]["c"] = torch.cat((sens(x), torch.zeros_like(c[..., case.fx_cols:])), -1)
            aux["T"] = torch.cat((sens(Tx), aux["T"][..., case.fx_cols:]), -1)
    elif case.tail == "swiglu":
        x = _rb(c, emu)
        gt, up = x[..., :N // 2], x[..., N // 2:]
        outs["h"] = _silu(gt, emu) * up
        if aux:
            sg = torch.sigmoid(gt)
            dg = (sg * (1 + gt * (1 - sg)) * up).abs()
            aux["S"]["h"] = dg * gt.abs() + outs["h"].abs()
            aux["fbw"]["h"] = dg * aux["T"][..., :N // 2] + _silu(gt, emu).abs() * aux["T"][..., N // 2:]
    elif case.tail == "swiglu_bwd":
        gu = inp["gu"].to(D)[None]
        gt, up, d = gu[..., :N], gu[..., N:], _rb(c, emu)
        sg = 1 / (1 + torch.exp(-gt))
        c = torch.cat((d * up * sg * (1 + gt * (1 - sg)), d * gt * sg), -1)
        if aux:                                       # linear in d: the sensitivity to d's rounding is |out| itself
            k = torch.cat((up * sg * (1 + gt * (1 - sg)), gt * sg), -1).abs()
            aux["S"]["c"] = c.abs()
            aux["T"] = k * torch.cat((aux["T"], aux["T"]), -1)
    elif case.tail == "norm":
        x = _rb(c, emu)
        rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
        outs["h"] = inp["nw"].to(D) * _rb(x * rstd, emu)
        if aux:                                       # three roundings upstream of the store: x, the row statistic of the rounded x (bounded by 2^-8 as well), x * rstd
            aux["S"]["h"] = 3 * outs["h"].abs()
            aux["fbw"]["h"] = inp["nw"].to(D).abs() * rstd * aux["T"]
    elif case.tail == "nb":                           # C = rms_norm_bwd(dy = the product, x, w) + dres: with g = dy w and s = rsqrt(mean(x^2) + eps), s g - x s^3 mean(g x)
        x, nw, dy = inp["nx"].to(D)[None], inp["nbw"].to(D), _rb(c, emu)
        s_ = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
        c = s_ * dy * nw - x * s_ ** 3 * (dy * nw * x).mean(-1, keepdim=True)
        if "dres" in inp:
            c = c + inp["dres"].to(D)[None]
        if aux:
            sens = lambda z: s_ * nw.abs() * z + x.abs() * s_ ** 3 * (nw.abs() * x.abs() * z).mean(-1, keepdim=True)
            aux["S"]["c"] = sens(dy.abs())
            aux["T"] = sens(aux["T"]) + (inp["dres"].to(D)[None].abs() if "dres" in inp else 0.0)
    elif case.tail == "dl":
        H, T_ = N // 128, case.T
        x, o = _rb(c, emu), inp["o"].to(D)[None]
        prod = (x * o).reshape(M // T_, T_, H, 128)
        outs["delta"] = prod.sum(-1).permute(0, 2, 1)
        if aux:
            sabs = prod.abs().sum(-1).permute(0, 2, 1)
            aux["S"]["delta"] = sabs
            aux["fbw"]["delta"] = (aux["T"] * o.abs()).reshape(M // T_, T_, H, 128).sum(-1).permute(0, 2, 1)
            aux["dl_sabs"] = sabs
    c = c if case.f32 else _rb(c, emu)
    if "h" in outs:
        outs["h"] = _rb(outs["h"], emu)
    if mut == "last_columns_keep_fill":
        c = c.clone()
        c[..., N - N % 4:] = fill
    if mut == "batch_writes_at_C0":
        c = torch.cat((c[-1:], torch.full_like(c[1:], fill)), 0)
    outs["c"] = c.to(F64)
    return {k: t.to(F64) for k, t in outs.items()}, aux


# ------------------------------------------------------------------------------------------------------------------------------- mutants
def mutant_names(case):
    M, N, K = case.M, case.N, case.K
    # A bf16 output shows one missing term of K only on an element whose |ref| is small beside it (the bound is relative, 2^-7 |ref|, and a term is ~ K^-1/2
    # of |ref|'s scale): that takes a few dozen elements to be certain, so the outputs of a handful of elements carry these two mutants in fp32 only (their -f32twin cases, see cases()).
    m = ["last_k8_dropped"] if case.f32 or M * N >= 8 else []
    if K >= 64 and (case.f32 or M * N >= 64):
        m.append("k_at_tile_boundary_dropped")
    if case.slices > 1:
        m += ["last_tile_of_last_slice_dropped", "slice1_first_tile_twice"]
    if case.ext:
        m.append("ext_dropped")
        if M >= 2:
            m.append("ext_from_row_m-1")
    if M >= 2:
        m.append("last_row_from_M-2")
    if N % 4:
        m.append("last_columns_keep_fill")
    if case.bias and N >= 2:
        m.append("bias_shifted_one_column")
    if case.gamma and N >= 2:
        m.append("gamma_shifted_one_column")
    if case.res and dims(case)[0] != dims(case)[1] and case.tail != "swiglu_bwd":
        m.append("residual_read_with_ldc")
    if case.bias and case.alpha != 1.0:
        m.append("alpha_after_bias")
    if case.gamma and case.act >= 2:                  # (ReLU commutes with a positive gain)
        m.append("gamma_before_act")
    if case.acc:
        m += ["accumulate_ignored", "accumulate_twice"]
    if case.b1 * case.b2 > 1:
        m.append("batch_writes_at_C0")
        if not case.w_bcast:
            m.append("batch_uses_W0")
    if (case.ta and M == K) or (case.tw and N == K):
        m.append("transposed_read_untransposed")
    if case.route == "skinny":
        m.append("skinny_row_plus_1")
    if case.a_norm and K > 8:
        m.append("a_norm_rstd_over_K-8")
    if case.a_swiglu:
        m.append("a_swiglu_up_at_K-8")
    return m


# --------------------------------------------------------------------------------------------------------------------- reference and bounds
@functools.lru_cache(maxsize=4)
def inp_cached(case):
    return inputs(case)


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> (inputs, fp64 reference outputs, per-element bounds)"""
    inp = inp_cached(case)
    ref, aux = compute(case, inp)
    fb = C_SUM * 2.0 ** -24 * math.sqrt(aux["n"])
    bounds = {}
    for n, r in ref.items():
        if n == "c":
            b = fb * aux["T"]
            if not case.f32:
                b = b + C_BF16 * 2.0 ** -8 * r.abs()
        elif n == "delta":            # fp32: 128 products of the stored bf16 dO and O, summed in another order
            b = C_SUM * 2.0 ** -24 * math.sqrt(128) * aux["dl_sabs"] + fb * aux["fbw"][n]
        else:
            b = C_BF16 * 2.0 ** -8 * r.abs() + fb * aux["fbw"][n]
        if n in aux["S"]:
            b = b + C_MID * 2.0 ** -8 * aux["S"][n]
        bounds[n] = b
    return inp, ref, bounds


def ratios(got, ref, bounds):
    return {n: ratio(got[n], ref[n], bounds[n]) for n in ref}


def emulation_ratios(case):
    inp, ref, bounds = reference(case)
    got, _ = compute(case, inp, emu=True)
    return ratios(got, ref, bounds)


def mutant_ratios(case):
    """mutant -> its worst ratio over the outputs"""
    inp, ref, bounds = reference(case)
    return {name: max(ratios(compute(case, inp, mut=name)[0], ref, bounds).values()) for name in mutant_names(case)}
