"""CPU: the tolerance that tests/test_linear_bwd_gpu.py holds `llmseg_linear_bwd` to has teeth.  On every case of tests/linear_bwd_checks.py an fp32
emulation of the kernel's summation order (chunks of 256, four waves folded in order, existing content last; bf16 where the kernel stores bf16) stays
within EMU_MAX of the bound, and every applicable mutant (db skipped, activation mask dropped, last partial M-tile skipped, last row dropped, existing
content ignored) leaves it by at least MUT_MIN.  Bounds and margins are those of tests/backward_kernel_checks.py.  Run with -s for the ratios."""
import pytest

from tests import backward_kernel_checks as bk
from tests import linear_bwd_checks as lb

CASES = lb.cases()
MUTANTS = {"last_row_dropped", "db_skipped", "act_mask_dropped", "last_partial_m_tile_skipped", "existing_content_ignored"}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    assert bool(case.taken) == lb.taken(case.M, case.N, case.K) and case.launches == (1 if case.taken else 0)
    if not case.taken:
        return                                                       # not covered: the GPU test asserts the refusal and that nothing was launched
    emu = lb.emulation_ratios(case)
    mut = lb.mutant_ratios(case)
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) + " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in sorted(mut.items(), key=lambda x: x[1])))
    assert all(r <= bk.EMU_MAX for r in emu.values()), f"the emulation exceeds {bk.EMU_MAX} of the bound: {emu}"
    weak = {n: r for n, r in mut.items() if not r >= bk.MUT_MIN}
    assert mut and not weak, f"mutants the tolerance does not reject by {bk.MUT_MIN}x: {weak}"


def test_table_covers_the_issue():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    took = [c for c in CASES if c.taken]
    assert {1, 15, 17, 638} <= {c.M for c in took} and {1, 4, 32} <= {c.N for c in took} and {56, 64, 72} <= {c.K for c in took}
    assert {512, 1024} <= {c.M for c in took}                       # 256 and 512 proposals per image at two images
    assert {c.act for c in took} == {"none", "relu", "sigmoid"} and {c.arena for c in took} == {0, 1} and {c.bias for c in took} == {0, 1}
    assert any(not c.taken for c in CASES)
    seen = set()
    for c in took:
        seen.update(lb.mutant_names(c))
    assert seen == MUTANTS, seen ^ MUTANTS
    assert lb.BENCH, "the benchmark step's shapes are listed"
