"""CPU: the GEMM dispatch decision (llmseg_amd/csrc/gemm_plan.h) against the plans pinned in tests/golden/gemm_plans.txt.

gemm_plan.h is host-only, so tests/gemm_plan_main.cpp is built with a plain g++ under AddressSanitizer and UBSan as a stand-alone program; it prints one plan
line per query of tests/gemm_plan_checks.py.  The golden lines come from the dispatch as it stood before the header existed (see gemm_plan_checks)."""
import ctypes as C

import pytest

from tests import gemm_plan_checks as gp


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    return gp.run_plan_program(gp.build_plan_program(tmp_path_factory.mktemp("gemm_plan")), gp.queries())


def test_plans_match_the_golden_file(plan_lines):
    golden = open(gp.GOLDEN).read().splitlines()
    assert len(golden) == len(gp.queries()) == len(plan_lines)
    diff = [(g, p) for g, p in zip(golden, plan_lines) if g != p]
    assert not diff, "%d plans differ from tests/golden/gemm_plans.txt; the first:\n  golden %s\n  plan   %s" % (len(diff), *diff[0])


def test_issue_table_plans():
    """The plans the workload depends on, spelled out.  Reads the golden file only, not the code: it guards against a golden file regenerated without
    a look at what moved (test_plans_match_the_golden_file ties the code to the file); a tile change edits these lines on purpose."""
    plans = gp.golden_plans()
    want = {"gpu:t160": ("t160", 4), "llama638:o_proj": ("pp128", 3), "llama638:dx_qkv": ("t160", 4), "llama638:gate_up": ("pp128", 1), "sam:8192x1280x1280": ("pp256", 1),
            "clip:514x1024x4096": ("pp128", 8), "gpu:pp128_s16": ("pp128", 16), "gpu:pp128_s7": ("pp128", 7), "gpu:glds": ("glds", 1), "gpu:pp128": ("pp128", 1)}
    for label, (kernel, slices) in want.items():
        assert (plans[label]["kernel"], int(plans[label]["slices"])) == (kernel, slices), label


def test_every_route_and_refusal_is_pinned():
    """Reads the golden file only: the query list must keep reaching every route, extension mode and reduce kernel, and some refusals."""
    plans = gp.golden_plans()
    live = [p for p in plans.values() if p is not None]
    assert {p["route"] for p in live} == {"skinny", "reg", "reg_sliced", "glds", "pp", "pp_sliced"}
    assert {p["ext"] for p in live} == {"none", "ktile", "slab", "second"}
    assert {p["reduce"] for p in live} == {"none", "plain", "norm", "nb", "dl"}
    assert any(p["fx"] == "1" for p in live) and any(p is None for p in plans.values())


def test_a_row_transform_with_extension_operands_is_refused():
    """a_norm_w / a_swiglu together with A2 / W2: on a route without the extension K-tile the K = 64 second launch would apply the transform to A2.  The plan
    refuses the call on every route, before any launch, so no device is needed (K = 200 takes the register-staging route)."""
    from llmseg_amd import _lib
    lib = _lib.load()
    for xform in (dict(a_norm_w=0x5000), dict(a_swiglu=1)):
        g = _lib.GemmArgs(A=0x1000, W=0x2000, C=0x3000, M=4, N=64, K=200, lda=400, ldw=200, ldc=64, alpha=1.0, A2=0x6000, W2=0x7000, lda2=64, ldw2=64, **xform)
        assert g.struct_size == C.sizeof(_lib.GemmArgs)
        assert lib.llmseg_gemm_bf16(C.byref(g), None) == -1 and b"do not go with extension operands" in lib.llmseg_last_error()
