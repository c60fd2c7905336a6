"""CPU: the per-element bounds of tests/test_gemm_kernels_gpu.py have teeth, and the table reaches what it claims.  On every case of tests/gemm_checks.py the
emulation of what the kernel rounds (fp32 accumulation per K-tile in slice order, the slabs summed in slice order, the epilogue in fp32 in the kernel's
operation order, the bf16 stores) stays at <= EMU_MAX of the bound, and every applicable mutant (the fp64 result of a slightly wrong problem) exceeds it by
>= MUT_MIN on at least one element.  Each case's GemmQuery line goes through the real gemm_plan.h (tests/gemm_plan_main.cpp, built as test_gemm_plan_cpu.py builds
it): a case that reaches another route than the one it declares is a failure of the table, found without a GPU.  Run with -s for the per-group summary that
profiles/gemm_parity.md records."""
import time

import pytest

from tests import gemm_checks as gc
from tests import gemm_plan_checks as gp

CASES = gc.cases()
_SEEN = {}
_T0 = time.time()

# every mutant must apply somewhere in the table
MUTANTS = {"last_k8_dropped", "k_at_tile_boundary_dropped", "last_tile_of_last_slice_dropped", "slice1_first_tile_twice", "ext_dropped", "ext_from_row_m-1",
           "last_row_from_M-2", "last_columns_keep_fill", "bias_shifted_one_column", "gamma_shifted_one_column", "residual_read_with_ldc", "alpha_after_bias",
           "gamma_before_act", "accumulate_ignored", "accumulate_twice", "batch_uses_W0", "batch_writes_at_C0", "transposed_read_untransposed", "skinny_row_plus_1",
           "a_norm_rstd_over_K-8", "a_swiglu_up_at_K-8"}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    lines = gp.run_plan_program(gp.build_plan_program(tmp_path_factory.mktemp("gemm_kernels_plan")), [gc.query_line(c) for c in CASES])
    assert len(lines) == len(CASES)
    return dict(gp.parse_plan(line) for line in lines)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\nratio to the bound per group (mutants: weakest, must be >= %g; emulation: worst, must be <= %g)" % (gc.MUT_MIN, gc.EMU_MAX))
        for n in sorted(_SEEN):
            r, where = (max if " emulation" in n else min)(_SEEN[n])
            print(f"  {n:48s} {r:12.3f}  at {where}  ({len(_SEEN[n])} cases)")
    print(f"tests/test_gemm_kernels_cpu.py: {time.time() - _T0:.1f} s, {len(CASES)} cases")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    emu = gc.emulation_ratios(case)
    mut = gc.mutant_ratios(case)
    for n, r in emu.items():
        _SEEN.setdefault(f"{case.group} emulation {n} {'fp32' if case.f32 or n == 'delta' else 'bf16'}", []).append((r, case.name))
    for n, r in mut.items():
        _SEEN.setdefault(f"{case.group} {n}", []).append((r, case.name))
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) + " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in mut.items()))
    assert all(r <= gc.EMU_MAX for r in emu.values()), f"{case.name}: an emulation of the kernel exceeds {gc.EMU_MAX} of the bound: {emu}"
    weak = {n: r for n, r in mut.items() if not r >= gc.MUT_MIN}
    assert not weak, f"{case.name}: the bound does not reject {weak}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_reaches_the_route_it_declares(case, plans):
    plan = plans[case.name]
    assert plan is not None, f"{case.name}: the plan refuses the call"
    want = gc.declared(case)
    got = {k: plan[k] for k in want}
    assert got == want, f"{case.name}: the table declares {want}, gemm_plan says {got}"


def test_the_table_reaches_every_kernel_and_template(plans):
    live = [p for p in plans.values() if p is not None]
    assert {p["kernel"] for p in live} == {"reg", "glds", "pp256", "pp128", "t160", "skinny"}
    assert {p["route"] for p in live} == {"skinny", "reg", "reg_sliced", "glds", "pp", "pp_sliced"}
    assert {p["ext"] for p in live} == {"none", "ktile", "slab", "second"}
    assert {p["reduce"] for p in live} == {"none", "plain", "norm", "nb", "dl"}
    assert {p["cpt"] for p in live if p["reduce"] == "norm"} == {"1", "2", "4"} and {p["cpt"] for p in live if p["reduce"] == "dl"} == {"1", "2", "4"}
    # all 24 skinny templates default knobs reach: [none, a_norm, a_swiglu] x [plain, K split among the waves] x [1, 2, 4, 8 rows]
    templates = {(gc.skinny_template(c)[0], int(plans[c.name]["ksplit"]), int(plans[c.name]["rows"])) for c in CASES if c.route == "skinny"}
    assert templates == {(at, sk, rows) for at in (0, 1, 2) for sk in (0, 1) for rows in (1, 2, 4, 8)}, sorted(templates)
    # register staging as K-slices with a last slice shorter than the others
    short = [c for c in CASES if c.route == "reg_sliced" and gc.cdiv(c.K, 64) % gc.cdiv(gc.cdiv(c.K, 64), c.slices)]
    assert short, "no reg_sliced case with a short last slice"
    # the ping-pong slices with an uneven last slice, on each of the three tiles
    assert {c.kernel for c in CASES if c.route == "pp_sliced" and (c.K // 64) % c.slices} == {"pp256", "pp128", "t160"}
    # the fused epilogues, the ragged column tile of SwiGLU backward among them
    assert {c.tail for c in CASES if c.fx} == {"rope", "swiglu", "swiglu_bwd"} and any(c.tail == "swiglu_bwd" and c.N % 256 for c in CASES)
    # all six activations on each store form of group E
    for form in ("interior", "edge", "skinny", "reduce"):
        assert {c.act for c in CASES if c.name.startswith(f"gemm-E-{form}-")} == set(range(6)), form


def test_every_mutant_applies_somewhere():
    seen = set()
    for c in CASES:
        seen |= set(gc.mutant_names(c))
    assert seen == MUTANTS, seen ^ MUTANTS
