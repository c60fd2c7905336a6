"""GPU: `llmseg_linear_bwd` (one launch for a small trainable Linear's act_bwd + dX + dW + db) against the fp64 reference of tests/linear_bwd_checks.py under the
per-element bounds of tests/backward_kernel_checks.py, on every shape the benchmark step sends it and on the edge shapes.  Every case also asserts the launch count
(one; none where the library answers "not taken"), NaN / fill guard regions around each output, and that two runs of the same call give the same bits.  The last test
drives `LinearFn.backward` itself with the fused route on and off (the LLMSEG_NO_FUSE_LINEAR_BWD switch): both against the same reference, and the launches per layer."""
import pytest
import torch

from tests import backward_kernel_checks as bk
from tests import linear_bwd_checks as lb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CASES = lb.cases()
GUARD = 128
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


class Out:
    """an output buffer with GUARD elements either side, pre-filled; .w = the part the call may write"""

    def __init__(self, shape, dtype, fill):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((2 * GUARD + n,), fill, dtype=dtype, device=DEV)
        self.w = self.buf[GUARD:GUARD + n].view(*shape)
        self.before = self.buf.clone()

    def guard_untouched(self):
        a, b = _bits(self.buf), _bits(self.before)
        return torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:])

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def _act(ops, name):
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID}[name]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_parity_with_fp64(case):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    M, N, K = case.M, case.N, case.K
    if not case.taken:                                               # the refusal: nothing launched, nothing written
        g = torch.Generator().manual_seed(case.seed)
        dy, y, x, w = (torch.randn(s, generator=g).to(BF).to(DEV) for s in ((M, N), (M, N), (M, K), (N, K)))
        o = {"dx": Out((M, K), BF, NAN), "dw": Out((N, K), F32, bk.FILL), "db": Out((N,), F32, bk.FILL)}
        n0 = lib.llmseg_launch_count()
        r = ops.linear_bwd(dy, y, _act(ops, case.act), x, w, dx=o["dx"].w, dw=o["dw"].w, db=o["db"].w, accumulate=True)
        torch.cuda.synchronize()
        assert r == "not taken" and lib.llmseg_launch_count() == n0 and all(b.untouched() for b in o.values())
        return
    inp, ref, bounds = lb.reference(case)
    dy, y, x, w = (inp[k].to(DEV) for k in ("dy", "y", "x", "w"))
    runs = []
    for _ in range(2):
        fill = bk.FILL if case.arena else NAN
        o = {"dx": Out((M, K), BF, NAN), "dw": Out((N, K), F32, fill)}
        if case.bias:
            o["db"] = Out((N,), F32, fill)
        torch.cuda.synchronize()
        n0 = lib.llmseg_launch_count()
        r = ops.linear_bwd(dy, y, _act(ops, case.act), x, w, dx=o["dx"].w, dw=o["dw"].w, db=o["db"].w if case.bias else None, accumulate=bool(case.arena))
        launches = lib.llmseg_launch_count() - n0
        torch.cuda.synchronize()
        assert r is o["dx"].w and launches == case.launches <= 2, f"{case.name}: {launches} launches"
        assert all(b.guard_untouched() for b in o.values()), f"{case.name}: a store outside an output (guard region changed)"
        runs.append({n: b.w.detach().clone() for n, b in o.items()})
    for n in runs[0]:
        assert torch.equal(_bits(runs[0][n]), _bits(runs[1][n])), f"{case.name}: {n} differs between two runs of the same call"
    got = {n: t.cpu() for n, t in runs[0].items()}
    assert set(got) == set(ref)
    r = bk.ratios(got, ref, bounds)
    print(f"\n{case.name}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    bad = {n: v for n, v in r.items() if not v <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"


def test_only_some_outputs():
    """dx alone, db alone, dw alone: the skipped outputs are not touched, the others are what the full call gives (same bits)"""
    from llmseg_amd import ops
    case = next(c for c in CASES if c.name == "linear_bwd-15x4x56_relu_b_arena")
    inp = lb.inputs(case)
    dy, y, x, w = (inp[k].to(DEV) for k in ("dy", "y", "x", "w"))
    M, N, K = case.M, case.N, case.K
    full = {"dx": Out((M, K), BF, NAN), "dw": Out((N, K), F32, bk.FILL), "db": Out((N,), F32, bk.FILL)}
    ops.linear_bwd(dy, y, ops.ACT_RELU, x, w, dx=full["dx"].w, dw=full["dw"].w, db=full["db"].w, accumulate=True)
    for only in ("dx", "dw", "db"):
        o = {"dx": Out((M, K), BF, NAN), "dw": Out((N, K), F32, bk.FILL), "db": Out((N,), F32, bk.FILL)}
        kw = {n: (o[n].w if n == only else None) for n in ("dx", "dw", "db")}
        ops.linear_bwd(dy, y, ops.ACT_RELU, x, w, want_dx=only == "dx", accumulate=True, **kw)
        torch.cuda.synchronize()
        for n in o:
            assert (torch.equal(_bits(o[n].buf), _bits(full[n].buf)) if n == only else o[n].untouched()), (only, n)


ROUTE_CASES = [(512, 256, 256, "none", True), (512, 2048, 256, "relu", True), (512, 256, 2048, "none", True), (512, 1, 256, "sigmoid", True), (17, 4, 64, "none", False),
               (2, 256, 256, "none", True)]


@pytest.mark.parametrize("M,N,K,act,arena", ROUTE_CASES, ids=[f"{m}x{n}x{k}_{a}_{'arena' if ar else 'plain'}" for m, n, k, a, ar in ROUTE_CASES])
def test_linearfn_fused_and_unfused_routes(M, N, K, act, arena):
    """LinearFn.backward with the one-launch route (default) and with the switch that restores the separate launches: both inside the bounds, and the launches per layer"""
    from llmseg_amd import _lib, autograd, ops
    lib = _lib.load()
    case = bk.Case("linear_bwd", f"route_{M}x{N}x{K}_{act}", 1, M=M, N=N, K=K, act=act, bias=1, arena=int(arena), taken=1)
    inp = lb.inputs(case)
    if act != "none":                                                # y must be the Linear's own output: take the reference's dpre from what the forward stores
        inp.pop("y")
    launches = {}
    for fused in (True, False):
        autograd.FUSE_LINEAR_BWD = fused
        try:
            x = inp["x"].to(DEV).requires_grad_(True)
            w = inp["w"].to(DEV).requires_grad_(True)
            b = torch.zeros(N, dtype=BF, device=DEV).requires_grad_(True)
            if arena:
                w._g32 = torch.full((N, K), bk.FILL, dtype=F32, device=DEV)
                b._g32 = torch.full((N,), bk.FILL, dtype=F32, device=DEV)
            yv = autograd.linear(x, w, b, _act(ops, act))
            torch.cuda.synchronize()
            n0 = lib.llmseg_launch_count()
            yv.backward(inp["dy"].to(DEV))
            torch.cuda.synchronize()
            launches[fused] = lib.llmseg_launch_count() - n0
        finally:
            autograd.FUSE_LINEAR_BWD = True
        ref_in = dict(inp, y=yv.detach().cpu())
        ref, aux = lb.compute(case, ref_in)
        got = {"dx": x.grad.cpu(), "dw": (w._g32 if arena else w.grad).cpu(), "db": (b._g32 if arena else b.grad).cpu()}
        if arena:
            bounds = {"dx": bk.bf16_bound(ref["dx"]), "dw": bk.f32_bound(*aux["dw"]), "db": bk.f32_bound(*aux["db"])}
        else:                                                        # plain autograd: bf16 .grad
            assert w.grad.dtype == BF and b.grad.dtype == BF
            bounds = {n: bk.bf16_bound(ref[n]) if n != "db" else bk.C_BF16 * 2.0 ** -8 * 2 * ref[n].abs() for n in ref}
        r = bk.ratios(got, ref, bounds)
        print(f"\n{case.name} fused={fused}: launches {launches[fused]} " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), (fused, r)
    assert launches[True] == 1 <= 2 and launches[False] >= (3 if act == "none" else 4), launches
