"""GPU: the backward, LoRA and optimizer kernels (llmseg_amd/csrc/backward.hip and lora.hip, the CE forward of head.hip) on every dispatch route against fp64
references, under the local tolerances that tests/test_backward_kernels_cpu.py validates against emulations and mutants.  Every case also asserts
the number of library launches its call makes (the proof that it still reaches the route it was written for), that the guard region around every
output it hands over is untouched, and -- for the reductions -- that the same call twice gives the same bits."""
import time

import pytest
import torch

from tests import _lines
from tests import backward_kernel_checks as bk

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
CASES = bk.cases()
GUARD = 128                    # elements in front of and behind every output buffer
NAN = float("nan")
TWICE = ("norm_bwd", "colsum", "ce", "scatter_add", "sumsq", "lora_down", "lora_outer", "lora_wgrads")       # run twice: the same bits


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    t0 = time.time()
    yield
    print(f"\ntests/test_backward_kernels_gpu.py: {time.time() - t0:.1f} s")


def _d(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32 if t.dtype == F32 else t.dtype)


class Out:
    """an output buffer larger than needed: GUARD elements either side of [alloc_rows, ld], pre-filled; .w = the part the call may write"""

    def __init__(self, rows, cols, dtype, fill, ld=None, alloc_rows=None):
        ld, alloc_rows = ld or cols, alloc_rows or rows
        self.buf = torch.full((2 * GUARD + alloc_rows * ld,), fill, dtype=dtype, device=DEV)
        self.full = self.buf[GUARD:GUARD + alloc_rows * ld].view(alloc_rows, ld)
        self.w = self.full[:rows, :cols]
        self.before = self.buf.clone()

    def guard_untouched(self):
        a, b = self.buf.clone(), self.before.clone()
        for t in (a, b):
            t[GUARD:GUARD + self.full.numel()].view_as(self.full)[:self.w.shape[0], :self.w.shape[1]] = 0
        return torch.equal(_bits(a), _bits(b))


def _ws(case):
    """the workspace= keyword of this case: the library default, None, or a uint8 buffer of the case's byte count"""
    if case.ws == "full":
        return {}
    return {"workspace": None if case.ws == "none" else torch.zeros(int(case.ws), dtype=torch.uint8, device=DEV)}


def _rng():
    return torch.tensor([bk.SEED, bk.OFFSET], dtype=torch.int64, device=DEV)


def _drop(case):
    return (_rng(), bk.STREAM, bk.P_DROP, case.p.get("seg", 0)) if case.p.get("drop") else None


def _c(what, rc):
    from llmseg_amd import _lib
    _lib.check(rc, what)


# every runner -> (call, outs, guarded): call() issues the library call(s); outs: name -> getter of the output; guarded: the Out buffers.  Where the ops wrapper
# allocates the output itself (dx, dgu, act_bwd's out, P, dS) the entry point is called on an Out buffer directly, with the wrapper's own argument helpers.
def run_norm_bwd(case, inp, ops):
    from llmseg_amd import _lib
    x, dy, w, dres = (_d(inp[k]) for k in ("x", "dy", "w", "dres"))
    o = {n: Out(1, case.cols, F32, bk.FILL) for n in ("dw", "db") if case.p[n]}
    o["dx"] = Out(case.rows, case.cols, BF, NAN)
    ws = _ws(case)
    p = ops._ptr

    def call():
        wp, wb = ops._ws_arg(ws.get("workspace", ops._DEFAULT_WS), x.device)
        _c("norm_bwd", _lib.load().llmseg_norm_bwd_add(p(dy), p(x), p(w), p(dres), p(o["dx"].w), p(o["dw"].w) if "dw" in o else None, p(o["db"].w) if "db" in o else None,
                                                       case.rows, case.cols, inp["eps"], int(case.rms), wp, wb, ops._stream()))
    return call, {n: (lambda b=b, n=n: b.w if n == "dx" else b.w[0]) for n, b in o.items()}, list(o.values())


def run_colsum(case, inp, ops):
    x = _d(inp["x"])[:, :case.N]
    o = Out(1, case.N, F32, bk.COLSUM_FILL)
    return (lambda: ops.colsum(x, out=o.w[0], **_ws(case))), {"out": lambda: o.w[0]}, [o]


def run_ce(case, inp, ops):
    N, T, V, ld = case.N, case.T, case.V, case.ld
    lg, lab, coef = _d(inp["logits"])[..., :V], _d(inp["labels"]), _d(inp["coef"])
    o = Out(N * T, V, BF, NAN, ld=ld)
    res = {}

    def call():
        res["loss"] = ops.ce_loss(lg, lab)
        ops.ce_bwd(lg, lab, coef, out=o.full.view(N, T, ld)[..., :V])
    return call, {"loss": lambda: res["loss"], "dlogits": lambda: o.w.reshape(N, T, V)}, [o]


def run_scatter_add(case, inp, ops):
    src, idx = _d(inp["src"]), _d(inp["idx"])
    o = Out(bk.N_DST, case.cols, F32, bk.FILL)
    return (lambda: ops.scatter_add_rows(src, idx, o.w)), {"dst": lambda: o.w}, [o]


def run_sumsq(case, inp, ops):
    x = _d(inp["buf"])[case.off:case.off + case.n]
    o = Out(1, 1, F32, float(case.n))
    return (lambda: ops.sumsq(x, o.w[0], **_ws(case))), {"out": lambda: o.w[0]}, [o]


def run_adamw(case, inp, ops):
    n = case.n
    o = {k: Out(1, n, F32, 0.0) for k in ("master", "m", "v")}
    o["p"] = Out(1, n, BF, NAN)
    for k in ("master", "m", "v"):
        o[k].w[0].copy_(_d(inp[k]))
        o[k].before = o[k].buf.clone()
    grad = _d(inp["grad"])
    gs = torch.tensor([bk.GSCALE], device=DEV) if case.gs else None
    call = lambda: ops.adamw_(o["p"].w[0], o["master"].w[0], grad, o["m"].w[0], o["v"].w[0], bk.LR, bk.B1, bk.B2, bk.AEPS, case.wd, case.step, grad_scale=gs)
    return call, {k: (lambda b=b: b.w[0]) for k, b in o.items()}, list(o.values())


def _pack_outs(H):
    return {"w2b": Out(3 * H, 64, BF, NAN), "w2a": Out(H, 64, BF, NAN), "bt": Out(16, H, BF, NAN)}


def run_lora_down(case, inp, ops):
    M, nb, zc = case.M, case.nb, case.zc
    x, x2, w0, w1 = (_d(inp[k]) for k in ("x", "x2", "w0", "w1"))
    o = {"y": Out(M, 8 * nb + zc, BF, NAN, ld=64 if case.wide else 8 * nb + zc, alloc_rows=M + bk.PAD_ROWS)}       # rows >= M and columns beyond 8 nb + zc keep their NaN
    kw = dict(alpha=bk.ALPHA, out=o["y"].full[:M, :(64 if case.wide else 8 * nb + zc)] if case.wide else o["y"].w, zero_cols=zc, drop=_drop(case),
              w_kr=bool(case.w_kr), scratch=bool(case.scratch))
    if nb == 2:
        kw.update(x2=x if case.same else x2, w2=w1.t().contiguous() if case.w_kr else w1)
    if case.pack:
        po = _pack_outs(264)
        o.update(po)
        kw["pack"] = tuple(_d(inp[k]) for k in ("aq", "bq", "av", "bv")) + (bk.PACK_S, po["w2b"].w, po["w2a"].w, po["bt"].w)
    wk = w0.t().contiguous() if case.w_kr else w0
    outs = {k: (lambda b=b: b.w) for k, b in o.items()}
    outs["y"] = lambda: o["y"].full[:, :8 * nb + zc]                 # the allocated rows beyond M with it: the reference holds NaN there
    if not case.parts:
        return (lambda: ops.lora_down(x, wk, **kw)), outs, list(o.values())
    if bk.route(case)[0] <= 1:                                       # no K slices on this shape: S = 0, no partials, y complete after the one launch
        plain = Out(M, 8 * nb + zc, BF, NAN, ld=o["y"].full.shape[1], alloc_rows=M + bk.PAD_ROWS)
        ops.lora_down(x, wk, **{**kw, "out": plain.full[:M] if case.wide else plain.w})      # the plain call of the same case (outside the counted launches)

        def call_noslices():
            _, part, S, sc = ops.lora_down(x, wk, parts=True, **kw)
            assert part is None and S == 0 and sc == bk.ALPHA, (part, S, sc)      # the finish factor is reported all the same (no dropout here: alpha)
            assert torch.equal(_bits(o["y"].full), _bits(plain.full)), f"{case.name}: y differs from the plain call's"
        return call_noslices, outs, list(o.values())
    d, wt, nx, nw, a0, a1 = (_d(inp[k]) for k in ("d", "wt", "nx", "nw", "a0", "a1"))

    def call():              # the K-slice partials are left unfinished; the norm-backward tail of the dX product finishes them and writes y
        _, part, S, sc = ops.lora_down(x, wk, parts=True, **kw)
        assert part is not None and S == bk.route(case)[0], (S, bk.route(case))
        ops.gemm(d, wt, normbwd=(nx, nw, 1e-6, True, None), nb_lora=(kw["out"], a0, a1, 1.0, None, part, S, sc, zc))
    return call, outs, list(o.values())


def run_lora_outer(case, inp, ops):
    N, nz = case.N, case.nz
    a, b = [_d(t) for t in inp["a"]], _d(inp["b"])
    shape = (8, N) if case.rn else (N, 8)
    o = [Out(shape[0], shape[1], F32, bk.FILL) for _ in range(nz)]
    kw = dict(out_rn=bool(case.rn), alpha=bk.ALPHA, out=o[0].w, drop=_drop(case), **_ws(case))
    if nz == 2:
        kw.update(a2=a[1], b2=b[:, 8:16], out2=o[1].w)
    return (lambda: ops.lora_outer(a[0], b[:, :8], **kw)), {f"out{z}": (lambda t=o[z]: t.w) for z in range(nz)}, o


def run_lora_wgrads(case, inp, ops):
    N = case.N
    d, x, xa, t = (_d(inp[k]) for k in ("d", "x", "xa", "t"))
    o = {"gbq": Out(N, 8, F32, bk.FILL), "gbv": Out(N, 8, F32, bk.FILL), "gaq": Out(8, N, F32, bk.FILL), "gav": Out(8, N, F32, bk.FILL)}
    call = lambda: ops.lora_wgrads(d, N, x, xa, t, o["gbq"].w, o["gbv"].w, o["gaq"].w, o["gav"].w, bk.ALPHA, drop=_drop(case), **_ws(case))
    return call, {k: (lambda b=b: b.w) for k, b in o.items()}, list(o.values())


def run_lora_apply(case, inp, ops):
    M, N = case.M, case.N
    y0 = _d(inp["y"])
    o = Out(M, N, BF, NAN, ld=y0.shape[1])
    o.full.copy_(y0)
    o.full[:, N:] = NAN                                               # the columns beyond N of a strided y are not the kernel's
    o.before = o.buf.clone()
    xa, w0, w1 = _d(inp["xa"]), _d(inp["w0"]), _d(inp["w1"])
    call = lambda: ops.lora_apply_(o.w, xa, w0, w_rn=bool(case.rn), alpha=bk.ALPHA, drop=_drop(case), w2=w1 if case.nb == 2 else None)
    return call, {"y": lambda: o.w}, [o]


def run_lora_pack(case, inp, ops):
    o = _pack_outs(case.H)
    aq, bq, av, bv = (_d(inp[k]) for k in ("aq", "bq", "av", "bv"))
    call = lambda: ops.lora_pack(aq, bq, av, bv, bk.PACK_S, w2b=o["w2b"].w, w2a=o["w2a"].w, bt=o["bt"].w)
    return call, {k: (lambda b=b: b.w) for k, b in o.items()}, list(o.values())


def run_transpose_pad(case, inp, ops):
    x = _d(inp["x"])[:, :case.cols]
    o = Out(case.cols, case.pad, BF, NAN, ld=case.pad + (24 if case.wide else 0))
    out = o.full if case.wide else o.w
    return (lambda: ops.transpose_pad(x, rows_pad=case.pad, out=out)), {"out": lambda: o.w}, [o]


def run_swiglu_bwd(case, inp, ops):
    from llmseg_amd import _lib
    gu, dout = _d(inp["gu"]), _d(inp["dout"])
    o = Out(case.rows, 2 * case.I, BF, NAN)
    call = lambda: _c("swiglu_bwd", _lib.load().llmseg_swiglu_bwd(ops._ptr(gu), ops._ptr(dout), ops._ptr(o.w), case.rows, case.I, ops._stream()))
    return call, {"dgu": lambda: o.w}, [o]


def run_act_bwd(case, inp, ops):
    from llmseg_amd import _lib
    dy, y = _d(inp["dy"]), _d(inp["y"])
    o = Out(1, case.n, BF, NAN)
    act = _lib.ACT_RELU if case.act == "relu" else _lib.ACT_SIGMOID
    call = lambda: _c("act_bwd", _lib.load().llmseg_act_bwd(ops._ptr(dy), ops._ptr(y), ops._ptr(o.w), case.n, act, ops._stream()))
    return call, {"out": lambda: o.w[0]}, [o]


def run_softmax_ds(case, inp, ops):
    from llmseg_amd import _lib
    BH, T, ld = case.BH, case.T, case.ld
    S, dP, km = _d(inp["S"]), _d(inp["dP"]), _d(inp["km"])
    Pref = bk.sd_reference_P(case).to(BF).to(DEV)                     # attn_ds is handed the reference's P: its check does not inherit the softmax's error
    o = {"P": Out(BH * T, ld, BF, NAN), "dS": Out(BH * T, ld, BF, NAN)}
    p = ops._ptr

    def call():
        lib = _lib.load()
        _c("softmax_rows", lib.llmseg_softmax_rows(p(S), p(o["P"].w), BH, T, T, ld, inp["scale"], int(case.causal), p(km), case.heads, ops._stream()))
        _c("attn_ds", lib.llmseg_attn_ds(p(Pref), p(dP), p(o["dS"].w), BH * T, T, ld, inp["scale"], ops._stream()))
    return call, {k: (lambda b=b: b.w.view(BH, T, ld)) for k, b in o.items()}, list(o.values())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_parity_with_fp64(case):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    inp, ref, bounds = bk.reference(case)
    runner = globals()["run_" + case.op]
    if case.einval:                                                   # the documented refusal, and nothing launched
        call, _, _ = runner(case, inp, ops)
        n0 = lib.llmseg_launch_count()
        with pytest.raises(RuntimeError) as e:
            call()
        assert case.einval in str(e.value) and lib.llmseg_launch_count() == n0, str(e.value)
        return
    runs = []
    for _ in range(2 if case.op in TWICE else 1):
        call, outs, guarded = runner(case, inp, ops)
        torch.cuda.synchronize()
        n0 = lib.llmseg_launch_count()
        call()
        launches = lib.llmseg_launch_count() - n0
        torch.cuda.synchronize()
        assert launches == case.launches, f"{case.name}: {launches} launches, the table says {case.launches} (a dispatch threshold moved?)"
        assert all(g.guard_untouched() for g in guarded), f"{case.name}: a store outside the output (guard region changed)"
        runs.append({n: get().detach().clone() for n, get in outs.items()})
    if len(runs) == 2:
        for n in runs[0]:
            assert torch.equal(_bits(runs[0][n]), _bits(runs[1][n])), f"{case.name}: {n} differs between two runs of the same call"
    got = {n: t.cpu() for n, t in runs[0].items()}
    assert set(got) == set(ref), (set(got), set(ref))
    r = bk.ratios(got, ref, bounds)
    print(f"\n{case.name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    _lines.record([(f"{case.name} {n}", x, 1.0) for n, x in r.items()], tag="backward_kernels ")
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"
