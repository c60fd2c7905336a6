"""GPU: one call per route of the GEMM dispatch, at the smallest shape the plan table (tests/golden/gemm_plans.txt, the `gpu:` lines) shows reaching it.

Each call is checked against an fp32 product within tests/kernel_checks.tol_bf16 (k = 1.5 where an epilogue is applied), and the number of kernels the library
launches for it must be the plan line's.  Where the plan leaves the caller's tail to the entry function, the count is instead what the library launches for
the same call without the tail plus for the follow-up entry point alone."""
import ctypes as C
import math

import pytest
import torch

from tests import gemm_plan_checks as gp
from tests.kernel_checks import tol_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
EPS = 1e-6


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert torch.cuda.get_device_properties(0).multi_processor_count == gp.NCU, "the plan table is for 256 CUs"
    from llmseg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def plans():
    return gp.golden_plans()


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(BF)


def _operands(M, N, K, ext=False):
    a, w = _rnd(M, K, seed=1), _rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    ref = a.float() @ w.float().t()
    kw = {}
    if ext:
        kw["a2"], kw["w2"] = _rnd(M, 64, seed=3, scale=0.5), _rnd(N, 64, seed=4, scale=1 / 8)
        ref = ref + kw["a2"].float() @ kw["w2"].float().t()
    return a, w, ref, kw


def _count(lib, fn):
    n0 = lib.llmseg_launch_count()
    r = fn()
    n = lib.llmseg_launch_count() - n0
    torch.cuda.synchronize()
    return r, n


def _check_rmsnorm(h, x, nw, label):
    """h against RMSNorm(x) * nw in fp32 of the bf16 row x the call stored.  The kernels round to bf16 before and after the weight multiply: two roundings of
    half an ulp (2^-8 relative) each, bounded here by 2.1 x 2^-8 of the largest |h| (the 0.1 covers their product and the fp32 row sum)."""
    xf = x.float()
    ref = (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + EPS)) * nw.float()
    err, tol = (h.float() - ref).abs().max().item(), 2.1 * 2.0 ** -8 * ref.abs().max().item()
    print(f"{label} norm_out: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, label


def _check(y, ref, k, label):
    err = (y.float() - ref).abs().max().item()
    print(f"{label}: err {err:.3e} tol {tol_bf16(ref, k):.3e}")
    assert err <= tol_bf16(ref, k), label


# label -> (M, N, K, extension operands, bias + ReLU epilogue)
PLAIN = {"gpu:glds": (300, 520, 64, False, True), "gpu:pp128": (300, 520, 128, False, True), "gpu:pp128_s7": (64, 256, 1344, False, True),
         "gpu:pp128_s16": (129, 256, 4096, False, False), "gpu:tail_fuses:none": (128, 2048, 2048, False, False), "gpu:ext_slab": (638, 512, 4096, True, False),
         "gpu:ext_ktile": (300, 520, 64, True, False), "gpu:ext_second": (200, 264, 200, True, False), "gpu:t160": (638, 4096, 4096, False, False),
         "gpu:skinny_ksplit": (5, 520, 2048, False, False), "gpu:skinny": (5, 520, 256, False, False)}


@pytest.mark.parametrize("label", sorted(PLAIN))
def test_route(lib, plans, label):
    from llmseg_amd import ops
    M, N, K, ext, epi = PLAIN[label]
    a, w, ref, kw = _operands(M, N, K, ext)
    if epi:
        b = _rnd(N, seed=5)
        ref = torch.relu(ref + b.float())
        kw.update(bias=b, act=ops.ACT_RELU)
    y, n = _count(lib, lambda: ops.gemm(a, w, **kw))
    # k = 1.5 where an epilogue is applied; the extension as a second launch is one (C is rounded to bf16, then added back as the residual of the second product)
    _check(y, ref, 1.5 if (epi or label == "gpu:ext_second") else 1.0, label)
    assert n == int(plans[label]["launches"]), f"{label}: {n} launches, the plan says {plans[label]['launches']}"


@pytest.mark.parametrize("tail", ["norm", "nb", "dl"])
def test_tail_rides_in_the_reduce_launch(lib, plans, tail):
    from llmseg_amd import ops
    label = f"gpu:tail_fuses:{tail}"
    assert plans[label]["tail_done"] == "1" and plans[label]["reduce"] == tail
    M, N, K = 128, 2048, 2048
    a, w, ref, _ = _operands(M, N, K)
    if tail == "norm":
        r, nw, h = _rnd(M, N, seed=6), (1.0 + 0.1 * _rnd(N, seed=7).float()).to(BF), torch.empty((M, N), device=DEV, dtype=BF)
        y, n = _count(lib, lambda: ops.gemm(a, w, residual=r, norm_w=nw, norm_eps=EPS, norm_out=h))
        ref = ref + r.float()
        _check_rmsnorm(h, y, nw, label)
    elif tail == "nb":
        # C = rms_norm_bwd(product, x, nw) + dres, in fp32: with g = product * nw and s = rsqrt(mean(x^2) + eps), dx = s g - x s^3 mean(g x)
        x, nw, dres = _rnd(M, N, seed=6), (1.0 + 0.1 * _rnd(N, seed=7).float()).to(BF), _rnd(M, N, seed=8, scale=0.2)
        y, n = _count(lib, lambda: ops.gemm(a, w, normbwd=(x, nw, EPS, True, dres)))
        g, xf = ref * nw.float(), x.float()
        s = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + EPS)
        ref = s * g - xf * s ** 3 * (g * xf).mean(-1, keepdim=True) + dres.float()
    else:
        H, T = N // 128, 64
        o, delta = _rnd(M, N, seed=6, scale=0.5), torch.empty((M // T, H, T), device=DEV)
        y, n = _count(lib, lambda: ops.gemm(a, w, delta_of=(o, delta, H, T)))
        # delta = rowsum(dO * O) per head of the bf16 dO the call stored: 128 fp32 products summed in another order, bounded by 128 x 2^-23 x sum |dO O|
        prod = (y.float() * o.float()).view(M // T, T, H, 128)
        derr, dtol = (delta - prod.sum(-1).permute(0, 2, 1)).abs().max().item(), 128 * 2.0 ** -23 * prod.abs().sum(-1).max().item()
        print(f"{label} delta: err {derr:.3e} tol {dtol:.3e}")
        assert derr <= dtol, label
    _check(y, ref, 1.0 if tail == "dl" else 1.5, label)
    assert n == int(plans[label]["launches"]), f"{label}: {n} launches, the plan says {plans[label]['launches']}"


def test_tail_left_to_the_entry_function(lib, plans):
    """128 x 520 x 2048 runs K-sliced, but no row kernel covers N = 520: the reduce launch is the plain one and llmseg_norm follows."""
    from llmseg_amd import ops
    assert plans["gpu:tail_separate:norm"]["tail_done"] == "0"
    M, N, K = 128, 520, 2048
    a, w, ref, _ = _operands(M, N, K)
    r, nw, h = _rnd(M, N, seed=6), (1.0 + 0.1 * _rnd(N, seed=7).float()).to(BF), torch.empty((M, N), device=DEV, dtype=BF)
    y, n = _count(lib, lambda: ops.gemm(a, w, residual=r, norm_w=nw, norm_eps=EPS, norm_out=h))
    y0, n_product = _count(lib, lambda: ops.gemm(a, w, residual=r))
    _, n_norm = _count(lib, lambda: ops.norm(y0, nw, eps=EPS, rms=True))
    _check(y, ref + r.float(), 1.5, "gpu:tail_separate:norm")
    _check_rmsnorm(h, y, nw, "gpu:tail_separate:norm")
    assert n_product == int(plans["gpu:tail_separate:none"]["launches"]) and n == n_product + n_norm, (n, n_product, n_norm)


@pytest.mark.parametrize("label", ["gpu:dw_sliced", "gpu:dw_single"])
def test_transposed_dw(lib, plans, label):
    """dW [136, 72] = dY^T X over 2048 rows, both operands stored row-major over the rows: register staging, K-sliced when the call brings a workspace."""
    from llmseg_amd import _lib, ops
    M, N, K = 136, 72, 2048
    a, w = _rnd(K, M, seed=1), _rnd(K, N, seed=2, scale=1 / math.sqrt(K))
    ref = a.float().t() @ w.float()
    if label == "gpu:dw_sliced":
        y, n = _count(lib, lambda: ops.gemm(a, w, trans_a=True, trans_w=True, out_f32=True))
    else:                                  # ops.gemm always hands its workspace over at this K: the same call without one
        y = torch.empty((M, N), device=DEV)
        g = _lib.GemmArgs(A=a.data_ptr(), W=w.data_ptr(), C=y.data_ptr(), M=M, N=N, K=K, lda=a.stride(0), ldw=w.stride(0), ldc=N, batch=1, alpha=1.0, out_f32=1, trans_a=1,
                          trans_w=1)
        rc, n = _count(lib, lambda: lib.llmseg_gemm_bf16(C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert rc == 0, lib.llmseg_last_error()
    _check(y, ref, 1.0, label)
    assert plans[label]["route"] == ("reg_sliced" if label == "gpu:dw_sliced" else "reg")
    assert n == int(plans[label]["launches"]), f"{label}: {n} launches, the plan says {plans[label]['launches']}"
