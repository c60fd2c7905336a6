"""CPU: MXFP4 weight-only decode -- the header, the binding and the library agree on the new symbols, the struct and the ABI number; the quantiser's
restatement gives the hand-computed codes on the hand-built blocks and keeps the format's two promises (amax <= 6 * 2^e with the smallest such e, W^ exact in
bf16); on every case of tests/mxfp4_checks.py the fp32 emulation of llmseg_gemm_mxfp4 stays at <= EMU_MAX of the per-element bound and every applicable mutant
exceeds it by >= MUT_MIN; generate() refuses bad weight modes before it touches a device.  No GPU: the entry points are only called where they must refuse
before any launch."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from tests import mxfp4_checks as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = xc.cases()
NAMES = ("llmseg_quantize_rows_mxfp4", "llmseg_gemm_mxfp4")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmseg_hip.h")).read(), flags=re.S)


def test_symbols_struct_and_abi_number_agree_in_header_binding_and_library():
    from llmseg_amd import _lib
    src = _header()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/llmseg_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in llmseg_amd/_lib.py"
    decl = re.search(r"llmseg_quantize_rows_mxfp4\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    args = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", a)[-1] for a in decl.split(",")]
    assert args == ["w", "ldw", "N", "K", "packed", "ldq", "scale", "lds", "w_hat", "ldh", "stream"], args
    assert _lib.SIGNATURES["llmseg_quantize_rows_mxfp4"] == [C.c_void_p if "*" in a else C.c_int64 for a in decl.split(",")]
    # the struct, field for field: llmseg_gemm_w8_args plus lds
    end = re.search(r"\}\s*llmseg_gemm_mxfp4_args\s*;", src).start()
    body = src[src.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    fields = []
    for d in body.split(";"):
        if d.strip():
            fields += [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for part in d.split(",")]
    assert [f[0] for f in _lib.GemmMxfp4Args._fields_] == fields and fields[0] == "struct_size"
    assert [f for f in fields if f != "lds"] == [f[0] for f in _lib.GemmW8Args._fields_]
    abi = int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1))
    assert abi == _lib.ABI_VERSION >= 19
    assert re.search(r"llmseg_version\(\) == %d\b" % abi, open(os.path.join(ROOT, "INTEGRATION.md")).read())
    lib = _lib.load()
    assert lib.llmseg_version() == abi
    for name in NAMES:
        assert hasattr(lib, name), name


def test_abi_guard_and_argument_checks_refuse_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    n0 = lib.llmseg_launch_count()
    g = _lib.GemmMxfp4Args(M=1, N=1, K=32)
    assert g.struct_size == C.sizeof(_lib.GemmMxfp4Args) == C.sizeof(_lib.GemmW8Args) + 8
    g.struct_size -= 8                                                       # llmseg_gemm_w8_args' size: a caller that mixed the two structs up
    assert lib.llmseg_gemm_mxfp4(C.byref(g), None) == -1 and b"ABI mismatch" in lib.llmseg_last_error()
    ok = dict(A=4096, Q=4096, scale=4096, C=4096, M=1, N=4, K=64, lda=64, ldq=32, lds=2, ldc=4)
    for bad in (dict(M=9), dict(M=0), dict(K=48), dict(K=16), dict(K=0), dict(ldq=40), dict(ldq=16), dict(lda=68), dict(lda=32), dict(lds=1), dict(A=4098), dict(Q=4104),
                dict(ldc=3), dict(A=0), dict(scale=0), dict(residual=4096, ldr=3)):
        assert lib.llmseg_gemm_mxfp4(C.byref(_lib.GemmMxfp4Args(**dict(ok, **bad))), None) == -1, bad
    p = C.c_void_p
    q_ok = dict(w=4096, ldw=64, N=2, K=64, packed=4096, ldq=32, scale=4096, lds=2, w_hat=None, ldh=0)
    for bad in (dict(K=48), dict(K=0), dict(ldq=40), dict(ldq=16), dict(ldw=68), dict(lds=1), dict(N=0), dict(w=None), dict(scale=None), dict(packed=4104),
                dict(w_hat=4096, ldh=32), dict(w_hat=4100, ldh=64)):
        a = dict(q_ok, **bad)
        rc = lib.llmseg_quantize_rows_mxfp4(p(a["w"]), a["ldw"], a["N"], a["K"], p(a["packed"]), a["ldq"], p(a["scale"]), a["lds"], p(a["w_hat"]), a["ldh"], None)
        assert rc == -1, bad
    assert lib.llmseg_launch_count() == n0, "a refused call launched"


@pytest.mark.parametrize("K", (32, 64, 96))
def test_restatement_gives_the_hand_computed_codes(K):
    w, codes, scales = xc.hand_blocks(K)
    packed, scale, w_hat = xc.quantize_mxfp4_ref(w)
    got = xc.nibbles(packed)
    for r, name in enumerate(xc.HAND_BLOCKS):
        assert torch.equal(got[r], codes[r]), name
        assert torch.equal(scale[r].to(torch.int64), scales[r]), name
    assert int((got == 8).sum()) == 0, "-0 is never stored"
    assert packed.shape == (len(xc.HAND_BLOCKS), K // 2) and packed.dtype == torch.uint8 and scale.shape == (len(xc.HAND_BLOCKS), K // 32)
    assert int(packed[2, 0]) == 2 | (4 << 4) and int(packed[2, 1]) == 9, "element 2 j sits in the low nibble of byte j"
    assert not w_hat[0].any() and bool(torch.isfinite(w_hat.float()).all())


@pytest.mark.parametrize("N,K", [(5, 32), (64, 2080), (257, 96)])
def test_restatement_keeps_the_formats_promises(N, K):
    w = xc.quant_input(N, K, 8)[:, :K].contiguous()
    packed, scale, w_hat = xc.quantize_mxfp4_ref(w)
    f = w.double().view(N, -1, 32)
    amax = f.abs().amax(-1)
    e = scale.to(torch.int64) - 127
    two_e = torch.ldexp(torch.ones_like(amax), e)
    assert bool((amax <= 6 * two_e).all()), "a block's amax exceeds 6 * 2^e"
    assert bool(((e == -127) | (amax > 3 * two_e)).all()), "e is not the smallest exponent that holds amax"
    assert len(set(scale.flatten().tolist())) >= (3 if K > 32 else 2), "the blocks' scales must differ for the table to mean anything"
    deq = xc.dequantize(packed, scale, K)
    assert torch.equal(w_hat.double(), deq), "W^ = element * 2^e is not exact in bf16"
    # nearest: no other representable value of the block's grid is closer to w
    grid = torch.tensor(xc.VALUES + tuple(-v for v in xc.VALUES), dtype=torch.float64)
    x = (f / two_e[..., None]).reshape(-1, 1)
    best = (x - grid[None, :]).abs().min(-1).values
    assert torch.equal((x[:, 0] - (deq.view(N, -1, 32) / two_e[..., None]).reshape(-1)).abs(), best)
    assert float((w_hat.double() - w.double()).abs().max()) > 0, "the quantiser changed nothing: the input is too coarse to test it"


def test_case_table_covers_what_the_kernel_can_get_wrong():
    S, U = xc.STEP, xc.UNIT
    assert {c.rows for c in CASES} == {1, 2, 4, 8} and {c.M for c in CASES} == set(range(1, 9))
    assert {(c.mfma, c.ksplit) for c in CASES} == {(0, 0), (0, 1), (1, 0)} and {c.nw for c in CASES if c.mfma} == {4, 16}
    assert {c.M for c in CASES if c.mfma} == set(range(xc.MFMA_ROWS, 9)) and {c.M for c in CASES if not c.mfma} == {1, 2}, "both sides of the kernels' threshold"
    for rows in (1, 2, 4, 8):
        ks = {c.K for c in CASES if c.rows == rows}
        for mult in (S, 2 * S, 3 * S, 4 * S):                      # one block below, at and past every multiple of the step up to 4 S (a wave's, or the 16-wave workgroup's)
            assert {mult - 32, mult, mult + 32} <= ks, (rows, mult)
        assert {32, 11008} <= ks
    for rows in (1, 2):
        assert {(c.ksplit, c.K) for c in CASES if c.rows == rows} >= {(1, 4 * S), (1, 4 * S + 32), (0, 4 * S - 32), (1, 11008)}
    for nw in (4, 16):                                             # the matrix-core kernel: around one unit and around the narrow workgroup's step
        ks = {c.K for c in CASES if c.mfma and c.nw == nw}
        assert {4 * U - 32, 4 * U, 4 * U + 32} <= ks, nw
    assert {U - 32, U, U + 32} <= {c.K for c in CASES if c.mfma}
    assert {c.K for c in CASES if c.N == 8196} == {xc.KSPLIT_K, xc.KSPLIT_K + 32}, "rows above the K-split threshold at a K that would split"
    assert {c.N for c in CASES} >= set(xc.FP4_N)
    for key in ("f32", "res"):
        assert {c.p[key] for c in CASES} == {0, 1}
    for pad in ("lda_pad", "ldq_pad", "lds_pad", "ldr_pad", "ldc_pad"):
        assert any(c.p[pad] for c in CASES), pad
    for name in ("nibbles_swapped", "sign_ignored", "scale_block_plus_1", "scale_bias_off_by_one", "table_3_4_exchanged", "last_block_dropped", "ldq_ignored",
                 "lds_ignored", "row_m_plus_1", "residual_scaled"):
        assert sum(name in xc.mutant_names(c) for c in CASES) >= 8, name
    inp = xc.inputs(next(c for c in CASES if c.ldq_pad and c.lds_pad))
    K = next(c for c in CASES if c.ldq_pad and c.lds_pad).K
    assert torch.isnan(inp["a"][-1].float()).all() and torch.isnan(inp["a"][:, K:].float()).all()
    assert bool((inp["q"][:, K // 2:] == 0xFF).all()) and bool((inp["scale"][:, K // 32:] == 0xFF).all())
    s = inp["scale"][:, :K // 32]
    assert int(s.min()) < 127 < int(s.max()), "scale bytes on both sides of 127"
    assert len(set(xc.nibbles(inp["q"][:, :K // 2]).flatten().tolist())) == 16, "every 4-bit code occurs"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bound_passes_the_emulation_and_rejects_every_mutant(case):
    r = xc.emulation_ratio(case)
    assert r <= xc.EMU_MAX, f"{case.name}: the fp32 emulation reaches {r:.3f} of the bound"
    for name, x in xc.mutant_ratios(case).items():
        assert x >= xc.MUT_MIN, f"{case.name}: mutant {name} reaches only {x:.3f} of the bound"


def test_generate_refuses_bad_weight_modes_before_touching_a_device():
    """the checks come before the first use of the model: a stand-in for `self` is enough"""
    from llmseg_amd.generate import GenerateMixin
    stub = types.SimpleNamespace()
    ids = torch.zeros((1, 4), dtype=torch.int64)
    gen = lambda **kw: GenerateMixin.generate(stub, None, ids, max_new_tokens=2, **kw)
    with pytest.raises(ValueError, match="weight_bits"):
        gen(weight_bits=4)
    with pytest.raises(ValueError, match="weight_format"):
        gen(weight_format="int4")
    with pytest.raises(ValueError, match="weight_format"):
        gen(weight_format="MXFP4")
    with pytest.raises(ValueError, match="one of them"):
        gen(weight_format="mxfp4", weight_bits=8)
    with pytest.raises(ValueError, match="fuse_decode"):
        gen(weight_format="mxfp4", fuse_decode=False)
    with pytest.raises(ValueError, match="weight_bits"):
        gen(weight_format="mxfp4", weight_bits=4)
