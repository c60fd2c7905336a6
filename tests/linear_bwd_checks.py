"""The one-launch backward of a small trainable Linear (`llmseg_linear_bwd`, llmseg_amd/csrc/backward.hip): case table, inputs, fp64 reference,
an fp32 emulation of the kernel's summation order, and mutants.  CPU only (no import of the HIP library); the tolerance forms, their constants
(`C_BF16`, `C_SUM`) and the margins (`EMU_MAX`, `MUT_MIN`) are those of tests/backward_kernel_checks.py.

The op:  y = act(x w^T + b), act in {none, relu, sigmoid};  dpre = bf16(dy * act'(y)) -- `llmseg_act_bwd`'s arithmetic (fp32: (dy * y) * (1 - y), or dy where
y > 0) and its bf16 store, which tests/backward_kernel_checks.py holds to fp64 on its own;  then, in fp64 from that dpre,
    dx [M, K] = dpre w  (bf16 form),    dW [N, K] (+)= dpre^T x,    db [N] (+)= column sums of dpre   (fp32 sums).
arena = 1: dW / db are `+=` on existing content (FILL); arena = 0: they overwrite (the buffers hold NaN before the call).

Summation order of the kernel, restated by the emulation: the contraction (m for dW / db, n for dx) runs in chunks of 256; wave w of the workgroup owns
[64 w, 64 w + 64) of every chunk and adds its terms in ascending order over all chunks, the four waves are then added in wave order (and the existing
content last).  db: thread j of a row's eight owns [32 j, 32 j + 32) of every chunk, then a fixed tree (j ^ 4, j ^ 2, j ^ 1)."""
import torch

from tests import backward_kernel_checks as bk

BF, F32, F64 = bk.BF, bk.F32, bk.F64
FILL = bk.FILL
MAX_M, MAX_NK = 2048, 1 << 22           # beyond: LLMSEG_NOT_TAKEN, nothing launched

# Every distinct (M, N, K, act, bias, arena) that one eager micro-step of the benchmark (bench.py --batch 2, 256 candidate masks, fp32 arena) hands to
# LinearFn.backward's small branch, read off an instrumented step.  taken = 0: the library answers "not taken" and today's route runs.
BENCH = [
    # M, N, K, act, bias, arena, taken                calls per micro-step
    (2, 256, 256, "none", 1, 1, 1),                   # 10: the single-key cross attentions' v / out projections, q_proj, out_proj of image -> token
    (2, 256, 4096, "none", 1, 1, 1),                  # 1: text_hidden_fcs.0.2
    (2, 4096, 4096, "relu", 1, 1, 0),                 # 1: text_hidden_fcs.0.0 -- 16 M weights: not taken, the separate launches run
    (512, 1, 128, "sigmoid", 1, 1, 1),                # 1: lisa_iou_head.2
    (512, 128, 256, "relu", 1, 1, 1),                 # 1: lisa_iou_head.0
    (512, 256, 256, "none", 1, 1, 1),                 # 2: self_attn.out_proj
    (512, 256, 2048, "none", 1, 1, 1),                # 3: mlp.lin2, lisa_embedding_head.2
    (512, 512, 256, "none", 1, 1, 1),                 # 2: k | v of image -> token
    (512, 768, 256, "none", 1, 1, 1),                 # 2: q | k | v of the self attention (the first layer's without dx)
    (512, 2048, 256, "relu", 1, 1, 1),                # 3: mlp.lin1, lisa_embedding_head.0
]

# edge shapes: M = 1, 15, 17, 638; N = 1, 4, 32; K = 64 +- 8; 256 and 512 proposals per image (M = 512 / 1024 rows at two images)
EDGE = [
    (1, 32, 64, "none", 1, 1, 1), (1, 1, 56, "sigmoid", 1, 1, 1), (15, 4, 56, "relu", 1, 1, 1), (15, 32, 72, "none", 1, 0, 1),
    (17, 1, 72, "sigmoid", 1, 1, 1), (17, 4, 64, "none", 0, 0, 1), (638, 32, 72, "relu", 1, 1, 1), (638, 1, 256, "sigmoid", 1, 0, 1),
    (638, 4, 56, "none", 0, 1, 1), (256, 256, 256, "relu", 1, 1, 1), (512, 264, 72, "none", 1, 1, 1), (1024, 256, 256, "none", 1, 1, 1),
    (1024, 2048, 256, "relu", 1, 1, 1), (1024, 256, 2048, "none", 1, 1, 1), (1024, 1, 256, "sigmoid", 1, 1, 1),
    (4, 4096, 4096, "relu", 1, 1, 0), (2049, 8, 8, "none", 1, 1, 0),
]


def cases():
    out, seen = [], set()
    for M, N, K, act, bias, arena, taken in BENCH + EDGE:
        name = f"{M}x{N}x{K}_{act}{'_b' if bias else ''}{'_arena' if arena else '_plain'}"
        if name in seen:
            continue
        seen.add(name)
        out.append(bk.Case("linear_bwd", name, 1 if taken else 0, M=M, N=N, K=K, act=act, bias=bias, arena=arena, taken=taken))
    return out


def taken(M, N, K):
    """the library's coverage rule, restated"""
    return M <= MAX_M and N * K <= MAX_NK


def inputs(case):
    g = bk._g(case)
    M, N, K = case.M, case.N, case.K
    pre = torch.randn(M, N, generator=g) * 2.0
    y = (torch.relu(pre) if case.act == "relu" else torch.sigmoid(pre) if case.act == "sigmoid" else pre).to(BF)
    dy = (torch.randn(M, N, generator=g) + 0.25).to(BF)
    x = (torch.randn(M, K, generator=g) + 0.25).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.25 + 0.05).to(BF)
    return dict(dy=dy, y=y, x=x, w=w)


def dpre_of(case, inp, masked=True):
    """bf16(dy * act'(y)) with the kernel's fp32 arithmetic (every step below is one IEEE fp32 operation, as in act_bwd_kernel)"""
    dy, y = inp["dy"].to(F32), inp["y"].to(F32)
    if case.act == "none" or not masked:
        return inp["dy"]
    if case.act == "relu":
        return torch.where(y > 0, dy, torch.zeros_like(dy)).to(BF)
    return ((dy * y) * (1.0 - y)).to(BF)


def _order_sum(t, emu, groups, per):
    """sum over dim 0 of t [C, ...].  emulation: fp32; chunk position p = c % 256; group p // per (`groups` of them) adds its terms in ascending c -> [groups, ...]"""
    C = t.shape[0]
    c = torch.arange(C)
    parts = []
    for gidx in range(groups):
        sel = ((c % 256) // per) == gidx
        tt = t[sel]
        parts.append(torch.cumsum(tt, 0)[-1] if tt.shape[0] else torch.zeros(t.shape[1:], dtype=t.dtype))
    return parts


def _wave_sum(a, b, emu):
    """sum_c a[c][i] b[c][k] -> [I, K].  emulation: fp32 rank-1 updates in ascending c into the accumulator of the wave that owns c, waves added in order"""
    if not emu:
        return a.t() @ b
    acc = [torch.zeros(a.shape[1], b.shape[1], dtype=a.dtype) for _ in range(4)]
    for c in range(a.shape[0]):
        acc[(c % 256) // 64] += a[c][:, None] * b[c][None, :]
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def _db_sum(t, emu):
    if not emu:
        return t.sum(0)
    p = _order_sum(t, emu, 8, 32)
    p = [p[j] + p[j ^ 4] for j in range(8)]
    p = [p[j] + p[j ^ 2] for j in range(8)]
    return p[0] + p[1]


def compute(case, inp, mut=None, emu=None):
    """-> (outputs, aux): dx (bf16 form), dw / db (fp32 sums; aux[name] = (n, sum |t|) of the fp64 reference)"""
    M, N, K = case.M, case.N, case.K
    T = lambda t: t.to(F32 if emu else F64)
    d = T(dpre_of(case, inp, masked=mut != "act_mask_dropped"))
    x, w = T(inp["x"]), T(inp["w"])
    rows = torch.ones(M, dtype=torch.bool)
    if mut == "last_partial_m_tile_skipped":
        rows[(M // 16) * 16:] = False
    elif mut == "last_row_dropped":
        rows[-1] = False
    # dx[m][k] = sum_n d[m][n] w[n][k]
    dx = bk._rb(_wave_sum(d.t().contiguous(), w, emu), emu).to(F64)
    if not rows.all():
        dx = dx.clone()
        dx[~rows] = float("nan")                                             # rows the mutant never writes keep the buffer's NaN
    out, aux = {"dx": dx}, {}
    fill = FILL if case.arena and mut != "existing_content_ignored" else 0.0
    sw = _wave_sum(d[rows], x[rows], emu)                                    # dW[n][k] = sum_m d[m][n] x[m][k]
    out["dw"] = ((torch.full_like(sw, fill) + sw) if emu else sw + fill).to(F64)
    if case.bias:
        sb = _db_sum(d[rows], emu) if rows.any() else torch.zeros(N, dtype=d.dtype)
        if mut == "db_skipped":
            sb = torch.zeros_like(sb)
            if not case.arena:
                sb = sb + float("nan")                                       # an overwritten output that is never written keeps its NaN
        out["db"] = ((torch.full_like(sb, fill) + sb) if emu else sb + fill).to(F64)
    if not emu and mut is None:
        na = 1 if case.arena else 0
        aux["dw"] = (M + na, (d.abs().t() @ x.abs()) + na * FILL)
        if case.bias:
            aux["db"] = (M + na, d.abs().sum(0) + na * FILL)
    return out, aux


def mutant_names(case):
    m = ["last_row_dropped"]
    if case.bias:
        m.append("db_skipped")
    if case.act != "none":
        m.append("act_mask_dropped")
    if case.M % 16:
        m.append("last_partial_m_tile_skipped")
    if case.arena:
        m.append("existing_content_ignored")
    return m


def reference(case):
    """-> (inputs, reference outputs, bounds)"""
    inp = inputs(case)
    ref, aux = compute(case, inp)
    bounds = {"dx": bk.bf16_bound(ref["dx"])}
    for n, (cnt, sabs) in aux.items():
        bounds[n] = bk.f32_bound(cnt, sabs)
    return inp, ref, bounds


def emulation_ratios(case):
    inp, ref, bounds = reference(case)
    got, _ = compute(case, inp, emu="order")
    return bk.ratios(got, ref, bounds)


def mutant_ratios(case):
    """-> mutant -> the LARGEST ratio over the outputs (a mutant is caught when any output leaves its bound)"""
    inp, ref, bounds = reference(case)
    out = {}
    for m in mutant_names(case):
        got, _ = compute(case, inp, mut=m)
        out[m] = max(bk.ratios(got, ref, bounds).values())
    return out
