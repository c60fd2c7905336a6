"""CPU: the tolerances of tests/test_backward_kernels_gpu.py have teeth.  On every case of the shared table the fp32 / bf16 emulations of what
the backward, LoRA and optimizer kernels round (terms in fp32, summed one after the other and as the kernel's slices folded in order, bf16 where
the kernel stores bf16) pass with a 2x margin, and every applicable mutant (an fp64 result of a subtly wrong problem) fails by at least 2x.
Run with -s to see each case's ratios and the per-mutant summary."""
import time

import pytest

from tests import backward_kernel_checks as bk

CASES = bk.cases()
_SEEN = {}
_T0 = time.time()

# every mutant that must apply somewhere in the table, per entry point
MUTANTS = {
    "norm_bwd": {"c1_dropped", "eps_dropped", "dres_dropped", "stats_over_padded_width", "c2_without_weight", "last_row_dropped", "last_partial_dropped",
                 "first_row_twice", "last_column_chunk_zero", "existing_content_ignored"},
    "colsum": {"last_row_dropped", "last_partial_dropped", "first_row_twice", "last_column_chunk_zero", "existing_content_ignored"},
    "ce": {"label_unshifted", "last_position_scored", "ignored_row_nonzero", "softmax_over_ld", "coef_not_applied", "onehot_missing", "count_includes_ignored"},
    "scatter_add": {"last_row_dropped", "existing_content_ignored", "second_hit_dropped", "hits_beyond_1024_dropped", "minus_one_to_row0"},
    "sumsq": {"last_row_dropped", "last_partial_dropped", "first_row_twice", "existing_content_ignored", "tail_dropped"},
    "adamw": {"bias_correction_missing", "eps_inside_sqrt", "wd_as_l2", "grad_scale_ignored", "m_v_from_unscaled_grad"},
    "lora_down": {"zero_cols_hold_1e-4", "row_m1_written_to_unused_tile_rows", "last_k_slice_dropped", "alpha_missing", "second_branch_reads_x", "v_uses_q_stream", "segment_offset_not_advanced", "dropout_scale_missing"},
    "lora_outer": {"last_row_dropped", "last_partial_dropped", "first_row_twice", "last_column_chunk_zero", "existing_content_ignored", "dropout_scale_missing",
                   "v_uses_q_stream"},
    "lora_wgrads": {"last_row_dropped", "last_partial_dropped", "first_row_twice", "last_column_chunk_zero", "existing_content_ignored", "dropout_scale_missing",
                    "v_uses_q_stream", "segment_offset_not_advanced"},
    "lora_apply": {"alpha_missing", "dropout_scale_missing", "v_uses_q_stream"},
    "lora_pack": {"bv_into_q_block", "scale_missing"},
    "transpose_pad": {"last_row_dropped"},
    "swiglu_bwd": {"gate_up_swapped", "silu_derivative_term_missing"},
    "act_bwd": {"derivative_from_preactivation", "relu_passes_at_zero"},
    "softmax_ds": {"padding_holds_1e-4", "masked_entries_hold_1e-4", "causal_k_lt_q", "mask_of_b_on_b+1", "delta_dropped", "scale_missing"},
}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\nratio to the bound over the table (mutants: weakest, must be >= %g; emulation: worst, must be <= %g)" % (bk.MUT_MIN, bk.EMU_MAX))
        for n in sorted(_SEEN):
            emu = " emulation " in n
            r, where = (max if emu else min)(_SEEN[n])
            print(f"  {n:55s} {r:12.3f}  at {where}  ({len(_SEEN[n])} cases)")
    print(f"tests/test_backward_kernels_cpu.py: {time.time() - _T0:.1f} s")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    if case.einval:
        assert bk.norm_route(case.rows, case.cols, True, case.ws_bytes)[0] == "einval"
        return
    emu = bk.emulation_ratios(case)
    mut = bk.mutant_ratios(case)
    for n, r in emu.items():
        _SEEN.setdefault(f"{case.op} emulation {n}", []).append((r, case.name))
    for n, r in mut.items():
        _SEEN.setdefault(f"{case.op} {n}", []).append((r, case.name))
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) +
          " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in sorted(mut.items(), key=lambda x: x[1])))
    assert all(r <= bk.EMU_MAX for r in emu.values()), f"an emulation exceeds {bk.EMU_MAX} of the bound: {emu}"
    assert mut, "no mutant applies to this case"
    weak = {n: r for n, r in mut.items() if not r >= bk.MUT_MIN}
    assert not weak, f"mutants the tolerance does not reject by {bk.MUT_MIN}x: {weak}"


def test_every_mutant_applies_somewhere():
    """every mutant of the list applies to at least one case of its entry point, and no case is left without one"""
    seen = {}
    for c in CASES:
        names = bk.mutant_names(c)
        assert names or c.einval, c
        seen.setdefault(c.op, set()).update(names)
    assert seen == MUTANTS, {op: (seen.get(op, set()) ^ MUTANTS.get(op, set())) for op in set(seen) | set(MUTANTS) if seen.get(op) != MUTANTS.get(op)}


def test_table_launches_and_routes_match_the_dispatch():
    """the launch count every case carries equals what the restated dispatch gives, and every norm_bwd case reaches the route it names"""
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        if c.einval:
            continue
        assert bk.route(c)[1] == c.launches, (c, bk.route(c), c.launches)
        if c.op == "norm_bwd":
            assert bk.norm_route(c.rows, c.cols, c.dw or c.db, c.ws_bytes)[0] == c.route, (c, bk.norm_route(c.rows, c.cols, c.dw or c.db, c.ws_bytes))
    routes = {c.route for c in CASES if c.op == "norm_bwd"}
    assert routes == {"wg_cpt1", "wg_cpt2", "wg_cpt4", "wave_cpl1", "wave_cpl2", "wave_cpl4", "wave_cpl8", "wave_cpl0", "acc_cpl1", "acc_cpl2", "wide", "einval"}, routes
    for rt in ("acc_cpl1", "acc_cpl2", "wide"):                 # each row class on each dw / db route
        assert {c.rows for c in CASES if c.op == "norm_bwd" and c.route == rt} >= {1, 3, 31, 33, 200, 638, 7656}, rt
    down = {c.name: bk.route(c)[0] for c in CASES if c.op == "lora_down"}
    assert down["lora_down-638x4096_S8"] == 8 and down["lora_down-7656x4096_S1"] == 1 and down["lora_down-638x4096_noscratch"] == 1
    assert down["lora_down-50x256_S2"] == 2 and down["lora_down-1x4096_S32"] == 32 and down["lora_down-17x384_S1"] == 1
    two = [c for c in CASES if isinstance(c.ws, int) and c.op != "sumsq"]
    assert two and all(bk.route(c)[0] == 2 for c in two), [(c, bk.route(c)) for c in two]


def test_adamw_bias_correction_host_vs_exact():
    """bc1 / bc2 as the host computes them (powf in fp32) against the exact values: the difference is reported and stays at fp32 resolution"""
    for step in (1, 2, 1000):
        (h1, h2), (e1, e2) = bk.adamw_bc(step), bk.adamw_bc(step, exact=True)
        print(f"\nstep {step}: bc1 host {h1:.9g} exact {e1:.9g} (rel {abs(h1 - e1) / e1:.2e}); bc2 host {h2:.9g} exact {e2:.9g} (rel {abs(h2 - e2) / e2:.2e})")
        assert abs(h1 - e1) <= 2.0 ** -22 * e1 and abs(h2 - e2) <= 2.0 ** -22 * e2
