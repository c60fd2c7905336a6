"""GPU: the forward glue, decode and head kernels (llmseg_amd/csrc/pointwise.hip, decode_attn, the pull-back, cosine, align / regression and dice / BCE kernels of head.hip) on every dispatch route
against fp64 references, under the local tolerances that tests/test_forward_kernels_cpu.py validates against emulations and mutants.  Every case also
asserts the number of library launches its call makes, that the guard region around every output it hands over is untouched, and -- through the
reference, which holds the input or a NaN sentinel there -- that every element inside the buffer that the op must not touch is what it was."""
import time

import pytest
import torch

from tests import _lines
from tests import forward_kernel_checks as fk
from tests.test_backward_kernels_gpu import Out, _bits, _c

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
CASES = fk.cases()
NAN = float("nan")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    t0 = time.time()
    yield
    print("\nworst ratio to the bound per op (must be <= 1)")
    for n in sorted(_WORST):
        print(f"  {n:28s} {_WORST[n][0]:8.3f}  at {_WORST[n][1]}")
    print(f"tests/test_forward_kernels_gpu.py: {time.time() - t0:.1f} s")


def _d(t):
    return None if t is None else t.to(DEV)


def _filled(o, src, fill=NAN):
    """an Out buffer that holds `src` (its .w part) as the op's in-place operand; the guard snapshot is retaken"""
    o.full.fill_(fill)
    o.w.copy_(src)
    o.before = o.buf.clone()
    return o


# every runner -> (call, outs, guarded): call() issues the library call(s); outs: name -> getter of the output; guarded: the Out buffers.  Where the ops wrapper
# allocates the output itself the entry point is called on an Out buffer directly, with the wrapper's own argument helpers.
def run_norm(case, inp, ops):
    c = case.cols
    x, w, b, rm = (_d(inp[k]) for k in ("x", "w", "b", "row_map"))
    o = Out(inp["out_rows"], c, BF, NAN, ld=inp["ldy"])
    call = lambda: ops.norm(x[:, :c], w, b, eps=inp["eps"], rms=bool(case.rms), out=o.w, row_map=rm)
    return call, {"y": lambda: o.full}, [o]


def run_rope(case, inp, ops):
    x0 = _d(inp["x"])
    rows, ld = x0.shape
    o = _filled(Out(rows, ld, BF, NAN), x0)
    cos, sin = _d(inp["cos"][:case.T].contiguous()), _d(inp["sin"][:case.T].contiguous())
    return (lambda: ops.rope_(o.w, cos, sin, rows, case.T, inp["heads"], case.hd, ld)), {"x": lambda: o.w}, [o]


def _act_call(ops, x, y, n, act):
    from llmseg_amd import _lib
    _c("act", _lib.load().llmseg_act(ops._ptr(x), ops._ptr(y), n, act, ops._stream()))


def run_act(case, inp, ops):
    x = _d(inp["x"])
    n = case.n
    if case.inplace:
        o = _filled(Out(1, n, BF, NAN), x[None])
        return (lambda: ops.act_(o.w[0], fk.ACTS[case.act])), {"y": lambda: o.w[0].view(-1, 8)}, [o]
    o = Out(1, n, BF, NAN)
    return (lambda: _act_call(ops, x, o.w, n, fk.ACTS[case.act])), {"y": lambda: o.w[0].view(-1, 8)}, [o]


def run_swiglu(case, inp, ops):
    gu = _d(inp["gu"])
    o = Out(case.rows, case.I, BF, NAN, ld=inp["ldo"])
    return (lambda: ops.swiglu(gu[:, :2 * case.I], case.I, out=o.w)), {"y": lambda: o.full}, [o]


def run_add_rows(case, inp, ops):
    x, add = _d(inp["x"]), _d(inp["add"])[:case.ar]
    o = Out(x.shape[0], x.shape[1], BF, NAN)
    return (lambda: ops.add_rows(x, add, out=o.w)), {"y": lambda: o.w}, [o]


def run_stride(case, inp, ops):
    idx = _d(inp["idx"])
    if case.kind == "act":
        x = _d(inp["x"])
        o = Out(1, x.numel(), BF, NAN)
        return (lambda: _act_call(ops, x, o.w, x.numel(), fk.ACTS["gelu"])), {"y": lambda: o.w[0].view(-1, 8)[idx]}, [o]
    gu = _d(inp["gu"])
    o = Out(gu.shape[0], case.I, BF, NAN)
    return (lambda: ops.swiglu(gu, case.I, out=o.w)), {"y": lambda: o.w.reshape(-1, 8)[idx]}, [o]


def run_patchify(case, inp, ops):
    img = _d(inp["img"])
    n = (case.H // case.pp) * (case.W // case.pp)
    o = Out(case.B * (n + case.extra), case.ldo, BF, NAN)
    return (lambda: ops.patchify(img, case.pp, case.ldo, rows_per_img=n + case.extra, row_off=case.off, out=o.w)), {"cols": lambda: o.w}, [o]


def run_im2col3x3(case, inp, ops):
    from llmseg_amd import _lib
    x = _d(inp["x"])
    B, H, W, Cc = case.B, case.H, case.W, case.C
    o = Out(B * H * W, 9 * Cc, BF, NAN)
    return (lambda: _c("im2col3x3", _lib.load().llmseg_im2col3x3(ops._ptr(x), ops._ptr(o.w), B, H, W, Cc, ops._stream()))), {"cols": lambda: o.w}, [o]


def run_embed_splice(case, inp, ops):
    from llmseg_amd import _lib
    N, L, P, Hd, V = (fk.SPLICE[k] for k in ("N", "L", "P", "Hd", "V"))
    ids, emb, buf = _d(inp["ids"]), _d(inp["embed"]), _d(inp["buf"])
    feats, stride = fk.splice_feats(case, {"buf": buf})
    o = Out(N * (L - 1 + P), Hd, BF, NAN)
    call = lambda: _c("embed_splice", _lib.load().llmseg_embed_splice(ops._ptr(ids), ops._ptr(emb), ops._ptr(feats), ops._ptr(o.w), N, L, P, Hd, V, stride, ops._stream()))
    return call, {"out": lambda: o.w}, [o]


def run_gather_rows(case, inp, ops):
    from llmseg_amd import _lib
    x, idx = _d(inp["x"]), _d(inp["idx"])
    o = Out(idx.numel(), case.cols, BF, NAN)
    call = lambda: _c("gather_rows", _lib.load().llmseg_gather_rows(ops._ptr(x), ops._ptr(idx), ops._ptr(o.w), idx.numel(), case.cols, case.ld, ops._stream()))
    return call, {"out": lambda: o.w}, [o]


def run_cosine(case, inp, ops):
    from llmseg_amd import _lib
    t, e = _d(inp["t"]), _d(inp["e"])
    o = Out(1, case.K, F32, NAN)
    call = lambda: _c("cosine_scores", _lib.load().llmseg_cosine_scores(ops._ptr(t), ops._ptr(e), ops._ptr(o.w), case.K, case.D, ops._stream()))
    return call, {"sim": lambda: o.w[0]}, [o]


def run_align(case, inp, ops):
    from llmseg_amd import _lib
    R, K, D, grads = case.items, case.K, case.D, bool(case.grads)
    e, t, gi, pr, gp = (_d(inp[k]) for k in ("e", "t", "gi", "pr", "gp"))
    o = {"out": Out(R, 2, F32, NAN)}
    if grads:
        o.update(d_e=Out(R * K, D, F32, NAN), d_t=Out(R, D, F32, NAN), d_pred=Out(R, K, F32, NAN))
    p = ops._ptr
    og = lambda n: p(o[n].w) if n in o else None

    def call():
        _c("align_reg_loss", _lib.load().llmseg_align_reg_loss(p(e), p(t), p(gi), p(pr), p(gp), p(o["out"].w), og("d_e"), og("d_t"), og("d_pred"), K, D, fk.TAU, R, ops._stream()))
        if R > 1:                                     # batched == single, bit for bit (the same kernel at another block index)
            for r in range(R):
                one = ops.align_reg_loss(e[r], t[r], gi[r], pr[r], gp[r], tau=fk.TAU, want_grads=grads)
                one = dict(zip(("out", "d_e", "d_t", "d_pred"), one)) if grads else {"out": one}
                for n, v in one.items():
                    assert torch.equal(_bits(v.reshape(-1)), _bits(o[n].w.reshape(R, -1)[r])), f"{n} of item {r} differs between the batched and the single call"
    outs = {"out": lambda: o["out"].w}
    if grads:
        outs.update(d_e=lambda: o["d_e"].w.view(R, K, D), d_t=lambda: o["d_t"].w, d_pred=lambda: o["d_pred"].w)
    return call, outs, list(o.values())


def run_decode(case, inp, ops):
    N, H, pos, cap = case.N, case.heads, case.pos, fk.CAP
    D = H * fk.HD
    qkv, cos, sin = (_d(inp[k]) for k in ("qkv", "cos", "sin"))
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    o = {n: _filled(Out(N * cap, D, BF, NAN), _d(inp[n[:2]]).view(N * cap, D)) for n in ("kc", "vc", "kc2", "vc2")}      # one pair of caches per route
    o["qkv"] = _filled(Out(N, 3 * D, BF, NAN), qkv)
    o["out"] = Out(N, D, BF, NAN)
    nf = fk.decode_scratch_floats(case)
    scratch = torch.empty(nf, dtype=F32, device=DEV) if nf else None
    cache = lambda n: o[n].w.view(N, cap, D)
    q0 = qkv.clone()

    def call():
        ops.decode_attn(qkv, cos, sin, cache("kc"), cache("vc"), posd, H, fk.HD, out=o["out"].w, scale=inp["scale"], scratch=scratch)
        ops.rope_kv_append_(o["qkv"].w, cos, sin, cache("kc2"), cache("vc2"), posd, H, fk.HD)
        assert torch.equal(_bits(qkv), _bits(q0)), "decode_attn wrote its qkv operand"
        assert torch.equal(_bits(o["kc"].w), _bits(o["kc2"].w)) and torch.equal(_bits(o["vc"].w), _bits(o["vc2"].w)), "decode_attn's caches differ from rope_kv_append's"
    return call, {"out": lambda: o["out"].w, "kc": lambda: cache("kc"), "vc": lambda: cache("vc"), "qkv": lambda: o["qkv"].w}, list(o.values())


def run_pullback(case, inp, ops):
    from llmseg_amd import _lib
    g, S, Cc = case.g, case.S, case.C
    segs, feat = _d(inp["segs"]), _d(inp["feat"])
    o = {"wn": Out(3, g * g, BF, NAN), "pb": Out(3, g * g, F32, NAN), "wsum": Out(1, 3, F32, NAN), "pooled": Out(3, Cc, BF, NAN), "wn2": Out(3, g * g, BF, NAN)}
    p = ops._ptr

    def call():              # the pull-back alone with its fp32 by-products, then the pooling entry point (pull-back + GEMM) without them
        lib = _lib.load()
        _c("mask_pullback", lib.llmseg_mask_pullback(p(segs), p(o["wn"].w), p(o["pb"].w), p(o["wsum"].w), 3, g, S, ops._stream()))
        _c("upsample_maskpool", lib.llmseg_upsample_maskpool(p(feat), p(segs), p(o["pooled"].w), p(o["wn2"].w), None, None, 3, Cc, g, S, ops._stream()))
        assert torch.equal(_bits(o["wn"].w), _bits(o["wn2"].w)), "the pull-back gives other bits inside upsample_maskpool"
    outs = {"wn": lambda: o["wn"].w, "pb": lambda: o["pb"].w, "wsum": lambda: o["wsum"].w[0], "pooled": lambda: o["pooled"].w}
    return call, outs, list(o.values())


def run_dice(case, inp, ops):
    from llmseg_amd import _lib
    x, y, g = _d(inp["x"]), _d(inp["y"]), _d(inp["g"])
    o, out = Out(case.M, case.HW, F32, NAN), Out(1, 2, F32, 0.0)          # dice_bce adds into a zeroed out[2], as ops.dice_bce hands it over
    p = ops._ptr

    def call():
        _c("dice_bce", _lib.load().llmseg_dice_bce(p(x), p(y), p(out.w), case.M, case.HW, fk.NUM_MASKS, *ops._reduce_ws(x.device), ops._stream()))
        _c("dice_bce_bwd", _lib.load().llmseg_dice_bce_bwd(ops._ptr(x), ops._ptr(y), ops._ptr(g), ops._ptr(o.w), case.M, case.HW, fk.NUM_MASKS, ops._stream()))
    return call, {"out": lambda: out.w[0], "dx": lambda: o.w}, [o, out]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_parity_with_fp64(case):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    inp, ref, bounds = fk.reference(case)
    call, outs, guarded = globals()["run_" + case.op](case, inp, ops)
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    call()
    launches = lib.llmseg_launch_count() - n0
    torch.cuda.synchronize()
    assert launches == case.launches, f"{case.name}: {launches} launches, the table says {case.launches} (a dispatch threshold moved?)"
    assert all(g.guard_untouched() for g in guarded), f"{case.name}: a store outside the output (guard region changed)"
    got = {n: get().detach().cpu() for n, get in outs.items()}
    assert set(got) == set(ref), (set(got), set(ref))
    r = fk.ratios(got, ref, bounds)
    print(f"\n{case.name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    _lines.record([(f"{case.name} {n}", x, 1.0) for n, x in r.items()], tag="forward_kernels ")
    for n, x in r.items():
        if x >= _WORST.get(f"{case.op} {n}", (-1.0, ""))[0]:
            _WORST[f"{case.op} {n}"] = (x, case.name)
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"
