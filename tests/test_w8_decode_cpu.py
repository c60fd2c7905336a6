"""CPU: int8 weight-only decode -- the header, the binding and the library agree on the new symbols and struct; the quantiser's restatement gives the
hand-computed results on the hand-built rows; on every case of tests/w8_checks.py the fp32 emulation of llmseg_gemm_w8 stays at <= EMU_MAX of the per-element
bound and every applicable mutant exceeds it by >= MUT_MIN.  No GPU: the entry points are only called where they must refuse before touching the device."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import w8_checks as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = wc.cases()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmseg_hip.h")).read(), flags=re.S)


def test_symbols_and_struct_agree_in_header_binding_and_library():
    from llmseg_amd import _lib
    src = _header()
    for name in ("llmseg_quantize_rows_i8", "llmseg_gemm_w8"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/llmseg_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in llmseg_amd/_lib.py"
    # the quantiser's ten arguments, in the header's order
    decl = re.search(r"llmseg_quantize_rows_i8\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    args = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", a)[-1] for a in decl.split(",")]
    assert args == ["w", "ldw", "N", "K", "q", "ldq", "scale", "w_hat", "ldh", "stream"], args
    kinds = [C.c_void_p if "*" in a else C.c_int64 for a in decl.split(",")]
    assert _lib.SIGNATURES["llmseg_quantize_rows_i8"] == kinds
    # the struct, field for field
    end = re.search(r"\}\s*llmseg_gemm_w8_args\s*;", src).start()
    body = src[src.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    fields = []
    for d in body.split(";"):
        if d.strip():
            fields += [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for part in d.split(",")]
    assert [f[0] for f in _lib.GemmW8Args._fields_] == fields
    assert fields[0] == "struct_size"
    assert int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION >= 13
    lib = _lib.load()
    for name in ("llmseg_quantize_rows_i8", "llmseg_gemm_w8"):
        assert hasattr(lib, name), name
    assert lib.llmseg_struct_size(4) == C.sizeof(_lib.GemmW8Args)
    assert lib.llmseg_struct_size(6) == -1                                   # (5 is llmseg_lora_down_args)
    assert re.search(r"llmseg_version\(\) == %d\b" % _lib.ABI_VERSION, open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_abi_guard_and_argument_checks_refuse_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    g = _lib.GemmW8Args(M=1, N=1, K=16)
    assert g.struct_size == C.sizeof(_lib.GemmW8Args)
    g.struct_size -= 8
    assert lib.llmseg_gemm_w8(C.byref(g), None) == -1 and b"ABI mismatch" in lib.llmseg_last_error()
    ok = dict(A=4096, Q=4096, scale=4096, C=4096, M=1, N=4, K=32, lda=32, ldq=32, ldc=4)
    for bad in (dict(M=9), dict(M=0), dict(K=24), dict(K=0), dict(ldq=40), dict(lda=36), dict(ldq=16), dict(A=4098), dict(Q=4104), dict(ldc=3), dict(A=0),
                dict(residual=4096, ldr=3)):
        assert lib.llmseg_gemm_w8(C.byref(_lib.GemmW8Args(**dict(ok, **bad))), None) == -1, bad
    p = C.c_void_p
    q_ok = dict(w=4096, ldw=32, N=2, K=32, q=4096, ldq=32, scale=4096, w_hat=None, ldh=0)
    for bad in (dict(K=24), dict(ldq=40), dict(ldw=36), dict(N=0), dict(w=None), dict(q=4104), dict(w_hat=4096, ldh=16), dict(w_hat=4100, ldh=32)):
        a = dict(q_ok, **bad)
        rc = lib.llmseg_quantize_rows_i8(p(a["w"]), a["ldw"], a["N"], a["K"], p(a["q"]), a["ldq"], p(a["scale"]), p(a["w_hat"]), a["ldh"], None)
        assert rc == -1, bad


@pytest.mark.parametrize("K", wc.QUANT_K)
def test_quantiser_restatement_on_hand_built_rows(K):
    w = wc.hand_rows(K)
    q, scale, w_hat = wc.quantize_ref(w)
    for r, want in wc.hand_rows_expected_q(K).items():
        assert torch.equal(q[r], want), wc.HAND_ROWS[r]
    assert scale[0] == 0 and not w_hat[0].any() and not torch.isnan(w_hat.float()).any()                 # all-zero row: scale 0, inv 0, no 0 / 0
    assert scale[1] == w[1].float().abs().max() / 127 and w_hat[1, 3 % K] == (127 * scale[1]).to(torch.bfloat16)
    assert q[2, 5 % K] == -127 and q[2].max() < 127 and scale[2] == torch.tensor(2.0) / 127              # amax is |-2|: the scale is positive
    assert q[3, K - 1] == 127 and q[3, :K - 1].abs().max() < 127                                         # the last column is part of the row's amax
    assert scale[4] == torch.tensor(127.0 * 2.0 ** wc.TIE_E) / 127
    assert q.abs().max() <= 127
    # bf16(q * scale) is within half a quantisation step (+ a bf16 rounding) of w on every row
    err = (w_hat.float() - w.float()).abs()
    assert bool((err <= 0.5 * scale[:, None] * (1 + 2.0 ** -6) + 2.0 ** -8 * w.float().abs()).all())


def test_case_table_covers_what_the_kernel_can_get_wrong():
    assert {c.rows for c in CASES} == {1, 2, 4, 8} and {c.ksplit for c in CASES} == {0, 1}
    for rows in (1, 2, 4, 8):
        step = 2048 if rows <= 2 else 1024
        ks = {c.K for c in CASES if c.rows == rows}
        for mult in (step, 2 * step, 4096, 8192):                  # one chunk below, at and past multiples of the wave's step and of the workgroup's
            assert {mult - 16, mult, mult + 16} <= ks, (rows, mult)
        assert {(c.ksplit, c.K) for c in CASES if c.rows == rows} >= {(1, 4096), (1, 4112), (0, 4096), (0, 4112), (0, 4080)}
    assert any(c.K == 11008 and c.N == 64 for c in CASES)
    for key in ("f32", "res"):
        assert {c.p[key] for c in CASES} == {0, 1}
    assert any(c.lda_pad for c in CASES) and any(c.ldr_pad for c in CASES) and any(c.ldc_pad for c in CASES) and any(c.ldq_pad for c in CASES)
    for name in ("last_chunk_dropped", "scale_row_plus_1", "q_unsigned", "row_m_plus_1", "scale_on_sum_plus_residual", "ldq_ignored"):
        assert sum(name in wc.mutant_names(c) for c in CASES) >= 8, name
    inp = wc.inputs(CASES[1])
    assert inp["q"].max() == 127 and inp["q"].min() == -127 and torch.isnan(inp["a"][-1].float()).all()
    assert any(wc.inputs(c)["scale"][1] == 0 for c in CASES[:8])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bound_passes_the_emulation_and_rejects_every_mutant(case):
    r = wc.emulation_ratio(case)
    assert r <= wc.EMU_MAX, f"{case.name}: the fp32 emulation reaches {r:.3f} of the bound"
    for name, x in wc.mutant_ratios(case).items():
        assert x >= wc.MUT_MIN, f"{case.name}: mutant {name} reaches only {x:.3f} of the bound"
