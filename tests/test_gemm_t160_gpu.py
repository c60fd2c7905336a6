"""GPU: the 160 x 256 K-sliced GEMM tile (variant 10) against the 128 x 256 tile it replaces (variant 9) and against fp32.

At the same slice count both tiles run the same MFMA with the same per-block K-step order over the same slice boundaries, so their fp32 slabs --
and every reduce tail that sums them -- must agree bit for bit.  The automatic dispatch is checked against an fp32 product within tol_bf16."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
# the five N = 4096 products of a Llama layer at 2 images per micro-step (o_proj and dX(o) share a shape)
LLAMA = [(638, 4096, 4096, "o_proj / dX(o)"), (638, 4096, 11008, "down"), (638, 4096, 12288, "dX(q|k|v)"), (638, 4096, 22016, "dX(gate|up)")]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from llmseg_amd import _lib
    lib = _lib.load()
    yield lib
    lib.llmseg_gemm_set_variant(5)


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(BF)


def _tol(ref, k=1.0):                      # tests/kernel_checks.tol_bf16
    return k * (2.0 ** -7) * max(1.0, ref.float().abs().max().item())


def _forced(lib, variant, S, fn):
    lib.llmseg_gemm_set_variant(variant | (S << 8))
    try:
        return fn()
    finally:
        lib.llmseg_gemm_set_variant(5)


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int16) if x.dtype == BF else x, y.view(torch.int16) if y.dtype == BF else y)


def _ext(M, N, seed):
    a2, w2 = _rnd(M, 64, seed=seed, scale=0.5), _rnd(N, 64, seed=seed + 1, scale=1 / 8)
    a2[:, 16:] = 0                        # LoRA: rank-8 (x2) columns, the rest of the 64-wide tile zero
    return a2, w2


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("M,N,K,tag", LLAMA)
def test_t160_llama_shapes_bit_identical(lib, M, N, K, tag, S):
    from llmseg_amd import ops
    a, w = _rnd(M, K, seed=1), _rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    a2, w2 = _ext(M, N, 3) if K == 12288 else (None, None)
    ref = a.float() @ w.float().t()
    if a2 is not None:
        ref += a2.float() @ w2.float().t()
    y9 = _forced(lib, 9, S, lambda: ops.gemm(a, w, a2=a2, w2=w2))
    y10 = _forced(lib, 10, S, lambda: ops.gemm(a, w, a2=a2, w2=w2))
    assert _same_bits(y10, y9), f"{tag} S={S}: 160 x 256 != 128 x 256"
    assert (y10.float() - ref).abs().max().item() <= _tol(ref)
    if a2 is None:                        # the same product without the extension slab, and the fp32-output route
        c9 = _forced(lib, 9, S, lambda: ops.gemm(a, w, out_f32=True))
        c10 = _forced(lib, 10, S, lambda: ops.gemm(a, w, out_f32=True))
        assert torch.equal(c10, c9), f"{tag} S={S}: fp32 output differs"


@pytest.mark.parametrize("M", [1, 159, 161, 638, 700])
def test_t160_edges_bit_identical(lib, M):
    from llmseg_amd import ops
    # N = 520: not a multiple of 256 (a 8-column last tile); K = 1344 = 21 K-tiles: 4 slices of 6, 6, 6, 3 (a shorter last slice)
    N, K = 520, 1344
    a, w, b = _rnd(M, K, seed=11), _rnd(N, K, seed=12, scale=1 / math.sqrt(K)), _rnd(N, seed=13)
    r = _rnd(M, N, seed=14)
    ref = r.float() + torch.relu(a.float() @ w.float().t() + b.float())
    for S in (2, 4):
        f = lambda: ops.gemm(a, w, bias=b, act=ops.ACT_RELU, residual=r)
        y9, y10 = _forced(lib, 9, S, f), _forced(lib, 10, S, f)
        assert _same_bits(y10, y9), f"M={M} S={S}: 160 x 256 != 128 x 256"
        assert (y10.float() - ref).abs().max().item() <= _tol(ref, 1.5)
    a2, w2 = _ext(M, N, 15)
    ref2 = a.float() @ w.float().t() + a2.float() @ w2.float().t()
    y9 = _forced(lib, 9, 4, lambda: ops.gemm(a, w, a2=a2, w2=w2))
    y10 = _forced(lib, 10, 4, lambda: ops.gemm(a, w, a2=a2, w2=w2))
    assert _same_bits(y10, y9), f"M={M}: with the extension slab, 160 x 256 != 128 x 256"
    assert (y10.float() - ref2).abs().max().item() <= _tol(ref2, 1.5)
    c32 = torch.full((M, N), 2.0, device=DEV)
    _forced(lib, 10, 4, lambda: ops.gemm(a, w, out=c32, accumulate=True, alpha=0.5))
    assert (c32 - (2.0 + 0.5 * (a.float() @ w.float().t()))).abs().max().item() <= 2e-3


@pytest.mark.parametrize("S", [3, 4])
def test_t160_reduce_rmsnorm_tail(lib, S):
    from llmseg_amd import ops
    M, N, K = 638, 4096, 11008
    a, w = _rnd(M, K, seed=21), _rnd(N, K, seed=22, scale=1 / math.sqrt(K))
    r, nw = _rnd(M, N, seed=23), (1.0 + 0.1 * _rnd(N, seed=24).float()).to(BF)
    outs = {}
    for v in (9, 10):
        h = torch.full((M, N), float("nan"), device=DEV, dtype=BF)
        y = _forced(lib, v, S, lambda: ops.gemm(a, w, residual=r, norm_w=nw, norm_eps=1e-6, norm_out=h))
        outs[v] = (y, h)
    assert _same_bits(outs[10][0], outs[9][0]) and _same_bits(outs[10][1], outs[9][1])
    ref = a.float() @ w.float().t() + r.float()
    assert (outs[10][0].float() - ref).abs().max().item() <= _tol(ref, 1.5)


@pytest.mark.parametrize("S", [3, 4])
def test_t160_reduce_delta_tail(lib, S):
    from llmseg_amd import ops
    Nb, T, H, hd = 2, 319, 32, 128
    D, M = H * hd, Nb * T
    dy, wt, o = _rnd(M, D, seed=31, scale=0.3), _rnd(D, D, seed=32, scale=D ** -0.5), _rnd(M, D, seed=33, scale=0.5)
    outs = {}
    for v in (9, 10):
        delta = torch.full((Nb, H, T), float("nan"), device=DEV)
        do = _forced(lib, v, S, lambda: ops.gemm(dy, wt, delta_of=(o, delta, H, T)))
        outs[v] = (do, delta)
    assert _same_bits(outs[10][0], outs[9][0]) and torch.equal(outs[10][1], outs[9][1])
    ref = dy.float() @ wt.float().t()
    assert (outs[10][0].float() - ref).abs().max().item() <= _tol(ref)


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("K,lora", [(12288, True), (22016, False)])
def test_t160_reduce_lora_normbwd_tail(lib, K, lora, S):
    from llmseg_amd import ops
    M, N = 638, 4096
    d, wt = _rnd(M, K, seed=41, scale=0.3), _rnd(N, K, seed=42, scale=K ** -0.5)
    x, w, dres = _rnd(M, N, seed=43), _rnd(N, seed=44), _rnd(M, N, seed=45, scale=0.2)
    t2, a0, a1 = _rnd(M, 64, seed=46, scale=0.3), _rnd(8, N, seed=47, scale=0.1), _rnd(8, N, seed=48, scale=0.1)
    drop = (torch.tensor([1234, 7], device=DEV, dtype=torch.int64), 6, 0.05)
    nb_lora = (t2, a0, a1, 1.0, drop) if lora else None
    outs = {v: _forced(lib, v, S, lambda: ops.gemm(d, wt, normbwd=(x, w, 1e-6, True, dres), nb_lora=nb_lora)) for v in (9, 10)}
    assert _same_bits(outs[10], outs[9])


@pytest.mark.parametrize("M,N,K,tag", LLAMA)
def test_auto_dispatch_llama_shapes_vs_fp32(lib, M, N, K, tag):
    from llmseg_amd import ops
    a, w = _rnd(M, K, seed=51), _rnd(N, K, seed=52, scale=1 / math.sqrt(K))
    ref = a.float() @ w.float().t()
    y = ops.gemm(a, w)
    assert (y.float() - ref).abs().max().item() <= _tol(ref), tag
