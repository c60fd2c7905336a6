"""The GEMM dispatch queries whose plans are pinned in tests/golden/gemm_plans.txt, and the text format tests/gemm_plan_main.cpp reads.

A query line is `label` followed by the integers of QUERY_FIELDS (a GemmQuery of llmseg_amd/csrc/gemm_plan.h) and of KNOB_FIELDS (a GemmKnobs).
A plan line is `label` followed by the plan's fields as key=value, or `label refused`.  The golden file was written by the decision statements of
gemm_dispatch as they stood before gemm_plan.h existed (copied into a scratch program, launches replaced by records), not by gemm_plan: a change of
the dispatch shows as a diff of that file."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_plans.txt")
PLAN_HEADER_DIR = os.path.join(os.path.dirname(HERE), "llmseg_amd", "csrc")
MAIN_CPP = os.path.join(HERE, "gemm_plan_main.cpp")

QUERY_FIELDS = ("M", "N", "K", "batch1", "batch2", "trans_a", "trans_w", "out_f32", "bias", "gamma", "residual", "act", "alpha_one", "ext", "a_norm",
                "a_swiglu", "ldc", "ldr", "ldn", "stride_c", "ws", "ws_aligned", "ws_bytes", "norm_ptrs_aligned", "tail", "fx", "ncu")
KNOB_FIELDS = ("variant", "skew", "split", "no_t160", "no_rsplit", "group_m", "skinny_sk", "norm_wg_max", "no_fx", "no_nb", "no_dl", "no_norm_fuse")
KNOB_DEFAULTS = dict(variant=5, skew=13, split=0, no_t160=0, no_rsplit=0, group_m=0, skinny_sk=1, norm_wg_max=2048, no_fx=0, no_nb=0, no_dl=0, no_norm_fuse=0)
TAIL_NONE, TAIL_NORM, TAIL_NB, TAIL_DL, TAIL_FX = range(5)
FX_ROPE, FX_SWIGLU, FX_SWIGLU_BWD = 1, 2, 3
WS_BYTES = 192 << 20          # llmseg_amd.ops.WS_BYTES: the scratch ops.gemm hands over when K >= 256
NCU = 256


def query(label, M, N, K, **kw):
    """One query line.  Defaults are what llmseg_amd.ops.gemm passes for dense 2-D operands: ldc = N, the workspace when K >= 256."""
    fx = kw.get("fx", 0)
    res = kw.get("residual", 0)
    ldc = kw.pop("ldc", 2 * N if fx == FX_SWIGLU_BWD else N)
    tail = kw.pop("tail", TAIL_FX if fx else TAIL_NONE)
    ws = kw.pop("ws", 1 if (K >= 256 or tail == TAIL_NB) else 0)
    ws_bytes = kw.pop("ws_bytes", (WS_BYTES - (M * N * 2 + 255) // 256 * 256 if tail == TAIL_NB else WS_BYTES) if ws else 0)
    q = dict(M=M, N=N, K=K, batch1=1, batch2=1, trans_a=0, trans_w=0, out_f32=0, bias=0, gamma=0, residual=0, act=0, alpha_one=1, ext=0, a_norm=0, a_swiglu=0,
             ldc=ldc, ldr=kw.pop("ldr", ldc if res else 0), ldn=N, stride_c=0, ws=ws, ws_aligned=1, ws_bytes=ws_bytes, norm_ptrs_aligned=1, tail=tail, fx=0, ncu=NCU)
    q.update(KNOB_DEFAULTS)
    for k, v in kw.items():
        assert k in q, k
        q[k] = int(v)
    assert " " not in label
    return label + " " + " ".join(str(q[f]) for f in QUERY_FIELDS + KNOB_FIELDS)


def _llama(M):
    H, I, V = 4096, 11008, 32004
    Vp, Mp = (V + 63) // 64 * 64, (M + 63) // 64 * 64
    t = f"llama{M}:"
    return [
        query(t + "qkv", M, 3 * H, H, ext=1, fx=FX_ROPE),
        query(t + "o_proj", M, H, H, residual=1, tail=TAIL_NORM),
        query(t + "down", M, H, I, residual=1, tail=TAIL_NORM),
        query(t + "gate_up", M, 2 * I, H, fx=FX_SWIGLU),
        query(t + "dx_down", M, I, H, fx=FX_SWIGLU_BWD),
        query(t + "dx_o", M, H, H, tail=TAIL_DL),
        query(t + "dx_qkv", M, H, 3 * H, ext=1, tail=TAIL_NB),
        query(t + "dx_gate_up", M, H, 2 * I, tail=TAIL_NB),
        query(t + "lm_head", M, V, H),
        query(t + "lm_head_dx", M, H, Vp),
        query(t + "lm_head_dw", V, H, Mp, out_f32=1),
    ]


# every forced variant (llmseg_gemm_set_variant's low bits), 5 = the cost model
VARIANTS = (0, 2, 3, 5, 8, 9, 10)         # 3: a value that names no kernel


def queries():
    qs = []
    for M in (638, 6380, 7656):
        qs += _llama(M)
    # SAM ViT-H at 2 images: global blocks see 2 x 4096 rows, windowed blocks the real 8192 or the 2 x 25 x 196 rows of the padded windows
    for M in (8192, 9800):
        for N in (1280, 3840, 5120):
            for K in (1280, 5120):
                qs.append(query(f"sam:{M}x{N}x{K}", M, N, K, bias=1, act=2 if N == 5120 else 0, residual=1 if N == 1280 else 0))
    # CLIP-L at 2 images: 2 x 257 rows
    for N, K, kw in ((3072, 1024, dict(bias=1)), (1024, 1024, dict(bias=1, residual=1)), (4096, 1024, dict(bias=1, act=3)), (1024, 4096, dict(bias=1, residual=1))):
        qs.append(query(f"clip:514x{N}x{K}", 514, N, K, **kw))
    # the head's small Linears: forward, dX through the stored transpose (trans_w), and the transposed dW form into the fp32 arena
    for M, N, K in ((2048, 136, 72), (2048, 72, 136), (2048, 256, 256), (2048, 8, 256), (512, 256, 2048)):
        qs.append(query(f"head:fwd:{M}x{N}x{K}", M, N, K, bias=1, act=1))
        qs.append(query(f"head:dx:{M}x{K}x{N}", M, K, N, trans_w=1, ws=1, ws_bytes=WS_BYTES))
        qs.append(query(f"head:dw:{N}x{K}x{M}", N, K, M, trans_a=1, trans_w=1, out_f32=1))
        qs.append(query(f"head:dw_nows:{N}x{K}x{M}", N, K, M, trans_a=1, trans_w=1, out_f32=1, ws=0))
    # skinny rows
    for M in (1, 2, 4, 5, 8):
        for K in (1024, 2048):
            for N in (4096, 8192, 8200, 32004):
                qs.append(query(f"skinny:{M}x{N}x{K}", M, N, K))
        qs.append(query(f"skinny:{M}:a_norm", M, 4096, 4096, a_norm=1))
        qs.append(query(f"skinny:{M}:a_swiglu", M, 4096, 11008, a_swiglu=1, residual=1))
        qs.append(query(f"skinny:{M}:f32", M, 32004, 4096, out_f32=1))
        qs.append(query(f"skinny:{M}:forced9", M, 4096, 4096, variant=9))
        qs.append(query(f"skinny:{M}:forced9:a_norm", M, 4096, 4096, variant=9, a_norm=1))
        qs.append(query(f"skinny:{M}:sk2", M, 32004, 4096, skinny_sk=2))
        qs.append(query(f"skinny:{M}:sk0", M, 4096, 4096, skinny_sk=0))
        qs.append(query(f"skinny:{M}:ext", M, 4096, 4096, ext=1))
    # edges
    for K in (64, 128, 192):
        for ext in (0, 1):
            for M, N in ((300, 520), (638, 4096), (4096, 4096)):
                qs.append(query(f"edge:kt:{M}x{N}x{K}:ext{ext}", M, N, K, ext=ext, ws=1, ws_bytes=WS_BYTES))
    qs.append(query("edge:short_last_slice", 64, 256, 1344))
    for K in (100, 200, 1000, 4100):
        qs.append(query(f"edge:k_not_64:{K}", 300, 520, K))
        qs.append(query(f"edge:k_not_64:{K}:ext", 300, 520, K, ext=1))
    for ta, tw in ((0, 1), (1, 0), (1, 1)):
        for M, N, K in ((136, 72, 2048), (512, 256, 2048), (4096, 4096, 640), (300, 520, 64)):
            qs.append(query(f"edge:trans{ta}{tw}:{M}x{N}x{K}", M, N, K, trans_a=ta, trans_w=tw))
    for b1, b2 in ((16, 1), (4, 8), (2, 1)):
        for M, N, K in ((4096, 128, 80), (196, 32, 80), (128, 128, 2048), (638, 4096, 4096)):
            qs.append(query(f"edge:batch{b1}x{b2}:{M}x{N}x{K}", M, N, K, batch1=b1, batch2=b2, out_f32=1, stride_c=M * N, ws=int(K >= 256 and b2 == 1)))
        qs.append(query(f"edge:batch{b1}x{b2}:trans_w", 128, 128, 2048, batch1=b1, batch2=b2, trans_w=1, stride_c=128 * 128 + 2, ws=1, ws_bytes=WS_BYTES))
    for M, N, K in ((638, 4096, 4096), (129, 256, 4096), (136, 72, 2048)):
        slab = M * N * 4
        qs.append(query(f"edge:no_ws:{M}x{N}x{K}", M, N, K, ws=0))
        qs.append(query(f"edge:ws_unaligned:{M}x{N}x{K}", M, N, K, ws_aligned=0))
        qs.append(query(f"edge:ws_2_slabs:{M}x{N}x{K}", M, N, K, ws_bytes=2 * slab))
        qs.append(query(f"edge:ws_2_slabs:{M}x{N}x{K}:ext", M, N, K, ws_bytes=2 * slab, ext=1))
        qs.append(query(f"edge:ws_3_slabs:{M}x{N}x{K}:ext", M, N, K, ws_bytes=3 * slab, ext=1))
        qs.append(query(f"edge:ws_under_2_slabs:{M}x{N}x{K}", M, N, K, ws_bytes=2 * slab - 1))
        qs.append(query(f"edge:ws_2_slabs:{M}x{N}x{K}:trans_w", M, N, K, ws_bytes=2 * slab, trans_w=1))
        qs.append(query(f"edge:ws_under_2_slabs:{M}x{N}x{K}:trans_w", M, N, K, ws_bytes=2 * slab - 1, trans_w=1))
        # a forced 2-slice plan fits at exactly 2 slabs (3 with the extension's own) and is refused one byte below
        for ext in (0, 1):
            qs.append(query(f"edge:forced_s2:ws_exact:{M}x{N}x{K}:ext{ext}", M, N, K, variant=9, split=2, ext=ext, ws_bytes=(2 + ext) * slab))
            qs.append(query(f"edge:forced_s2:ws_1_short:{M}x{N}x{K}:ext{ext}", M, N, K, variant=9, split=2, ext=ext, ws_bytes=(2 + ext) * slab - 1))
    qs.append(query("edge:ldc_not_4", 638, 4096, 4096, ldc=4098))
    qs.append(query("edge:ldc_4_not_8:norm", 638, 4096, 4096, ldc=4100, residual=1, tail=TAIL_NORM))
    qs.append(query("edge:ldr_not_4", 638, 4096, 4096, residual=1, ldr=4098))
    qs.append(query("edge:n_not_4", 638, 4094, 4096))
    qs.append(query("edge:n_not_4:trans_w", 136, 70, 2048, trans_w=1))
    # fused tails: where the row kernels apply and where they do not
    for M, N, K in ((128, 2048, 2048), (128, 520, 2048), (63, 2048, 4096), (128, 8192, 2048), (128, 8320, 2048), (2048, 4096, 4096), (638, 4096, 4096)):
        qs.append(query(f"tail:norm:{M}x{N}x{K}", M, N, K, residual=1, tail=TAIL_NORM))
        qs.append(query(f"tail:nb:{M}x{N}x{K}", M, N, K, tail=TAIL_NB))
        if N % 128 == 0:
            qs.append(query(f"tail:dl:{M}x{N}x{K}", M, N, K, tail=TAIL_DL))
        qs.append(query(f"tail:none:{M}x{N}x{K}", M, N, K))
    qs.append(query("tail:norm:bias", 128, 2048, 2048, bias=1, tail=TAIL_NORM))
    qs.append(query("tail:norm:ptrs_unaligned", 128, 2048, 2048, tail=TAIL_NORM, norm_ptrs_aligned=0))
    qs.append(query("tail:norm:wg_max", 638, 4096, 4096, residual=1, tail=TAIL_NORM, norm_wg_max=512))
    qs.append(query("tail:dl:alpha", 128, 2048, 2048, tail=TAIL_DL, alpha_one=0))
    for fx, N in ((FX_ROPE, 12288), (FX_ROPE, 12416), (FX_SWIGLU, 22016), (FX_SWIGLU, 22032), (FX_SWIGLU_BWD, 11008), (FX_SWIGLU_BWD, 11016)):
        qs.append(query(f"tail:fx{fx}:638x{N}", 638, N, 4096, fx=fx, ext=int(fx == FX_ROPE)))
    qs.append(query("tail:fx1:no_ext", 638, 12288, 4096, fx=FX_ROPE))
    # every forced variant with and without a forced split, the refusals among them
    for v in VARIANTS:
        for S in (0, 1, 2, 4, 7, 31):
            for M, N, K, kw in ((638, 4096, 4096, {}), (638, 4096, 12288, dict(ext=1)), (300, 520, 128, dict(ws=1, ws_bytes=WS_BYTES)), (300, 520, 64, dict(ext=1)),
                                (200, 264, 200, dict(ext=1)), (638, 4096, 4096, dict(ws=0)), (638, 4096, 4096, dict(trans_w=1)), (5, 520, 2048, {}),
                                (638, 4096, 4096, dict(ext=1, act=2)), (128, 2048, 2048, dict(tail=TAIL_DL))):
                tag = "".join(f":{k}{x}" for k, x in kw.items())
                qs.append(query(f"forced:v{v}:s{S}:{M}x{N}x{K}{tag}", M, N, K, variant=v, split=S, **kw))
    # each A/B switch on one shape it changes
    qs.append(query("knob:no_t160", 638, 4096, 4096, no_t160=1))
    qs.append(query("knob:no_rsplit", 136, 72, 2048, trans_a=1, trans_w=1, out_f32=1, no_rsplit=1))
    qs.append(query("knob:group_m", 6380, 12288, 4096, group_m=2))
    qs.append(query("knob:skinny_sk", 5, 520, 2048, skinny_sk=0))
    qs.append(query("knob:norm_wg_max", 638, 4096, 4096, residual=1, tail=TAIL_NORM, norm_wg_max=600))
    qs.append(query("knob:no_fx", 638, 22016, 4096, fx=FX_SWIGLU, no_fx=1))
    qs.append(query("knob:no_nb", 638, 4096, 22016, tail=TAIL_NB, no_nb=1))
    qs.append(query("knob:no_dl", 638, 4096, 4096, tail=TAIL_DL, no_dl=1))
    qs.append(query("knob:no_norm_fuse", 638, 4096, 4096, residual=1, tail=TAIL_NORM, no_norm_fuse=1))
    qs.append(query("knob:skew", 638, 4096, 4096, skew=3))
    # the calls tests/test_gemm_plan_gpu.py runs: their launch counts are read from the golden file
    qs += gpu_queries()
    labels = [q.split()[0] for q in qs]
    assert len(set(labels)) == len(labels), "duplicate label"
    return qs


def gpu_queries():
    return [
        query("gpu:glds", 300, 520, 64, bias=1, act=1),
        query("gpu:pp128", 300, 520, 128, bias=1, act=1),
        query("gpu:pp128_s7", 64, 256, 1344, bias=1, act=1),
        query("gpu:pp128_s16", 129, 256, 4096),
        query("gpu:tail_fuses:norm", 128, 2048, 2048, residual=1, tail=TAIL_NORM),
        query("gpu:tail_fuses:nb", 128, 2048, 2048, tail=TAIL_NB),
        query("gpu:tail_fuses:dl", 128, 2048, 2048, tail=TAIL_DL),
        query("gpu:tail_fuses:none", 128, 2048, 2048),
        query("gpu:tail_separate:norm", 128, 520, 2048, residual=1, tail=TAIL_NORM),
        query("gpu:tail_separate:none", 128, 520, 2048, residual=1),
        query("gpu:ext_slab", 638, 512, 4096, ext=1),
        query("gpu:ext_ktile", 300, 520, 64, ext=1),
        query("gpu:ext_second", 200, 264, 200, ext=1),
        query("gpu:t160", 638, 4096, 4096),
        query("gpu:pp256", 4096, 4096, 2048),
        query("gpu:dw_sliced", 136, 72, 2048, trans_a=1, trans_w=1, out_f32=1),
        query("gpu:dw_single", 136, 72, 2048, trans_a=1, trans_w=1, out_f32=1, ws=0),
        query("gpu:skinny_ksplit", 5, 520, 2048),
        query("gpu:skinny", 5, 520, 256),
    ]


def build_plan_program(tmp_dir):
    """tests/gemm_plan_main.cpp as a stand-alone host program under AddressSanitizer and UBSan -> its path"""
    assert shutil.which("g++"), "the plan program needs g++"
    exe = os.path.join(str(tmp_dir), "gemm_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I", PLAN_HEADER_DIR, MAIN_CPP, "-o", exe])
    return exe


def run_plan_program(exe, query_lines):
    """one plan line per query line"""
    r = subprocess.run([exe], input="\n".join(query_lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def parse_plan(line):
    """label, {field: value} of one plan line (None: refused)"""
    parts = line.split()
    return parts[0], (None if parts[1:] == ["refused"] else dict(kv.split("=", 1) for kv in parts[1:]))


def golden_plans():
    """label -> {field: value} of the golden file; a refused call maps to None."""
    plans = {}
    with open(GOLDEN) as f:
        for line in f:
            parts = line.split()
            plans[parts[0]] = None if parts[1:] == ["refused"] else dict(kv.split("=", 1) for kv in parts[1:])
    return plans
