"""GPU: the GEMM kernels (llmseg_amd/csrc/gemm.hip) on every case of tests/gemm_checks.py against fp64 references, under the per-element bounds that
tests/test_gemm_kernels_cpu.py validates against emulations and mutants.  Every case also asserts that the library launched as many kernels as the plan the
case declares (the CPU test ties that declaration to gemm_plan.h), that nothing outside the output was written -- the guard elements either side of C, the
columns N .. ld, the rows past M, the gaps between batch entries -- and, on the K-sliced routes, that the same call twice gives the same bits.
Forced kernels go through llmseg_gemm_set_variant and are restored in a `finally` (and once more by the module fixture)."""
import collections
import time

import pytest
import torch

from tests import _lines
from tests import gemm_checks as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
CASES = gc.cases()
GUARD = 128                    # elements in front of and behind every output buffer
PAST = 2                       # allocated rows past M
_WORST = collections.defaultdict(lambda: (0.0, ""))


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert torch.cuda.get_device_properties(0).multi_processor_count == gc.gp.NCU, "the declared plans are for 256 CUs"
    from llmseg_amd import _lib
    t0 = time.time()
    yield
    _lib.load().llmseg_gemm_set_variant(5)
    print("\nworst error / bound per group and output")
    for k in sorted(_WORST):
        print(f"  {k:16s} {_WORST[k][0]:.3f}  at {_WORST[k][1]}")
    print(f"tests/test_gemm_kernels_gpu.py: {time.time() - t0:.1f} s, {len(CASES)} cases")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


class Out:
    """an output inside a larger pre-filled buffer: GUARD elements, `off` more, then `batch` entries `stride` apart of [rows + PAST, ld]; .w = what the call may write"""

    def __init__(self, batch, rows, cols, dtype, fill, ld=None, stride=0, off=0):
        ld = ld or cols
        span = (batch - 1) * stride + (rows + PAST) * ld
        self.buf = torch.full((2 * GUARD + off + span,), fill, dtype=dtype, device=DEV)
        self.w = self.buf.as_strided((batch, rows, cols), (stride, ld, 1), GUARD + off)
        self.before = self.buf.clone()

    def guard_untouched(self):
        a, b = self.buf.clone(), self.before.clone()
        for t in (a, b):
            t.as_strided(self.w.shape, self.w.stride(), self.w.storage_offset()).zero_()
        return torch.equal(_bits(a), _bits(b))


def _runner(case, inp, ops):
    """-> (call, outputs name -> getter, the guarded buffers)"""
    M, N, K = case.M, case.N, case.K
    ldc, ldr, sC, B, wide = gc.dims(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    c = Out(B, M, wide, F32 if case.f32 else BF, gc.FILL if case.acc else gc.NAN, ld=ldc, stride=sC, off=case.off_c)
    outs, guarded = {"c": lambda: c.w}, [c]
    a, w = d["a"], d["w"]
    if B > 1:
        s_a, s_w = a.shape[1] * a.shape[2], 0 if case.w_bcast else w.shape[1] * w.shape[2]

        def call():
            ops.gemm_batched(a, w, c.w, M, N, K, a.shape[2], w.shape[2], ldc, case.b1, s_a, s_w, sC, out_f32=bool(case.f32), alpha=case.alpha, trans_a=bool(case.ta),
                             trans_w=bool(case.tw), batch2=case.b2, sA2=case.b1 * s_a, sW2=case.b1 * s_w, sC2=case.b1 * sC)
        return call, outs, guarded
    av = a[0][:, :M] if case.ta else a[0][:M, :(2 * K if case.a_swiglu else K)]
    wv = w[0][:, :N] if case.tw else w[0][:, :K]
    kw = dict(act=case.act, alpha=case.alpha, out=c.w[0], trans_a=bool(case.ta), trans_w=bool(case.tw), accumulate=bool(case.acc), a_swiglu=bool(case.a_swiglu))
    if case.bias:
        kw["bias"] = d["bias"][case.off_b:case.off_b + N]
    if case.gamma:
        kw["gamma"] = d["gamma"][case.off_g:case.off_g + N]
    if case.res:
        kw["residual"] = d["res"].as_strided((M, N), (ldr, 1), case.off_r)
    if case.ext:
        kw.update(a2=d["a2"][:, :64], w2=d["w2"])
    if case.a_norm:
        kw.update(a_norm_w=d["anw"], a_norm_eps=gc.EPS)
    if case.tail == "norm":
        h = Out(1, M, N, BF, gc.NAN)
        kw.update(norm_w=d["nw"], norm_eps=gc.EPS, norm_out=h.w[0])
    elif case.tail == "swiglu":
        h = Out(1, M, N // 2, BF, gc.NAN)
        kw["swiglu_out"] = h.w[0]
    elif case.tail == "dl":
        H = N // 128
        h = Out(1, M // case.T * H, case.T, F32, gc.NAN)
        kw["delta_of"] = (d["o"], h.w[0].view(M // case.T, H, case.T), H, case.T)
        outs["delta"] = lambda: h.w[0].view(M // case.T, H, case.T)
        guarded.append(h)
    elif case.tail == "nb":
        kw["normbwd"] = (d["nx"], d["nbw"], gc.EPS, True, d.get("dres"))
    elif case.tail == "rope":
        kw["rope"] = (d["cos"], d["sin"], case.T, case.fx_cols)
    elif case.tail == "swiglu_bwd":
        kw["swiglu_bwd_of"] = d["gu"]
    if case.tail in ("norm", "swiglu"):
        outs["h"] = lambda: h.w
        guarded.append(h)
    return (lambda: ops.gemm(av, wv, **kw)), outs, guarded


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_parity_with_fp64(case):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    inp, ref, bounds = gc.reference(case)
    runs = []
    try:
        if case.v != 5:
            lib.llmseg_gemm_set_variant(case.v | case.S << 8)           # (a zero skew field keeps the skew)
        for _ in range(2 if case.slices > 1 else 1):
            call, outs, guarded = _runner(case, inp, ops)
            torch.cuda.synchronize()
            n0 = lib.llmseg_launch_count()
            call()
            launches = lib.llmseg_launch_count() - n0
            torch.cuda.synchronize()
            assert launches == case.launches, f"{case.name}: {launches} launches, the table says {case.launches}"
            assert all(g.guard_untouched() for g in guarded), f"{case.name}: a store outside the output (guard, columns N .. ld, rows past M or a batch gap changed)"
            runs.append({n: get().detach().clone() for n, get in outs.items()})
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):          # a device fault: nothing more may be started on this GPU
            pytest.exit(f"{case.name}: {e}", returncode=3)
        raise
    finally:
        lib.llmseg_gemm_set_variant(5)
    if len(runs) == 2:
        for n in runs[0]:
            assert torch.equal(_bits(runs[0][n]), _bits(runs[1][n])), f"{case.name}: {n} differs between two runs of the same call"
    got = {n: t.cpu() for n, t in runs[0].items()}
    assert set(got) == set(ref), (set(got), set(ref))
    r = gc.ratios(got, ref, bounds)
    print(f"\n{case.name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    _lines.record([(f"{case.name} {n}", x, 1.0) for n, x in r.items()], tag="gemm_kernels ")
    for n, x in r.items():
        k = f"{case.group} {n} {'fp32' if case.f32 or n == 'delta' else 'bf16'}"
        _WORST[k] = max(_WORST[k], (x, case.name))
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"
