"""CPU: the tolerances of tests/test_forward_kernels_gpu.py have teeth.  On every case of the shared table the fp32 / bf16 emulation of what the
forward glue and head kernels round passes with a 2x margin, and every applicable mutant (an fp64 result of a subtly wrong problem) fails by at
least 2x.  The table is also held to the dispatch: every route of llmseg_norm and of the mask pull-back is reached, and the launch count every
case carries is what the restated dispatch gives.  Run with -s to see each case's ratios and the per-mutant summary."""
import time

import pytest

from tests import forward_kernel_checks as fk

CASES = fk.cases()
_SEEN = {}
_T0 = time.time()

# every mutant that must apply somewhere in the table, per entry point
MUTANTS = {
    "norm": {"eps_dropped", "variance_without_mean", "stats_over_padded_width", "bias_dropped", "last_chunk_dropped", "last_row_dropped", "row_map_ignored",
             "minus_one_written_to_row0", "ldx_taken_as_cols"},
    "rope": {"position_not_wrapped", "sine_sign_flipped", "interleaved_pairs", "v_rotated_too", "last_head_dropped"},
    "act": {"tanh_gelu", "quickgelu_constant_1", "last_chunk_dropped"},
    "swiglu": {"gate_up_swapped", "ldgu_taken_as_2I", "last_chunk_dropped"},
    "add_rows": {"added_row_indexed_by_row_mod_rows", "last_chunk_dropped"},
    "stride": {"beyond_first_sweep_unwritten"},
    "patchify": {"pixel_major_layout", "padding_left_unzeroed", "row_off_ignored"},
    "im2col3x3": {"tap_order_transposed", "border_wraps"},
    "embed_splice": {"second_image_token_used", "ids_after_image_shifted_by_one", "feats_stride_ignored"},
    "gather_rows": {"ldx_taken_as_cols", "index_sorted"},
    "cosine": {"target_norm_missing", "last_row_dropped", "last_lane_group_dropped"},
    "align": {"tau_missing", "kl_direction_reversed", "exp_weight_missing", "dpred_factor_missing", "last_column_chunk_zero", "target_norm_missing"},
    "decode": {"key_pos_excluded", "key_pos_plus_1_included", "stale_cache_row_used_for_pos", "k_written_at_pos_plus_1", "v_rotated", "last_split_dropped", "scale_missing"},
    "pullback": {"align_corners_weights", "border_clamp_dropped", "seam_row_dropped", "normaliser_eps_missing", "wsum_from_mask_area"},
    "dice": {"scale_missing", "bce_not_averaged", "g_swapped", "dice_gradient_without_N", "hw_tail_dropped"},
}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\nratio to the bound over the table (mutants: weakest, must be >= %g; emulation: worst, must be <= %g)" % (fk.MUT_MIN, fk.EMU_MAX))
        for n in sorted(_SEEN):
            emu = " emulation " in n
            r, where = (max if emu else min)(_SEEN[n])
            print(f"  {n:55s} {r:12.3f}  at {where}  ({len(_SEEN[n])} cases)")
    print(f"tests/test_forward_kernels_cpu.py: {time.time() - _T0:.1f} s")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    emu = fk.emulation_ratios(case)
    mut = fk.mutant_ratios(case)
    for n, r in emu.items():
        _SEEN.setdefault(f"{case.op} emulation {n}", []).append((r, case.name))
    for n, r in mut.items():
        _SEEN.setdefault(f"{case.op} {n}", []).append((r, case.name))
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) +
          " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in sorted(mut.items(), key=lambda x: x[1])))
    assert all(r <= fk.EMU_MAX for r in emu.values()), f"an emulation exceeds {fk.EMU_MAX} of the bound: {emu}"
    assert mut, "no mutant applies to this case"
    weak = {n: r for n, r in mut.items() if not r >= fk.MUT_MIN}
    assert not weak, f"mutants the tolerance does not reject by {fk.MUT_MIN}x: {weak}"


def test_every_mutant_applies_somewhere():
    """every mutant of the list applies to at least one case of its entry point, and no case is left without one"""
    seen = {}
    for c in CASES:
        names = fk.mutant_names(c)
        assert names, c
        seen.setdefault(c.op, set()).update(names)
    assert seen == MUTANTS, {op: (seen.get(op, set()) ^ MUTANTS.get(op, set())) for op in set(seen) | set(MUTANTS) if seen.get(op) != MUTANTS.get(op)}


def test_table_reaches_every_route():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert fk.route(c)[1] == c.launches, (c, fk.route(c), c.launches)
    norm = [c for c in CASES if c.op == "norm"]
    assert {fk.route(c)[0] for c in norm} == {"wave_cpl1", "wave_cpl2", "wave_cpl3", "wave_cpl4", "wave_cpl8", "wave_cpl16", "wave_cpl0", "wg_cpt1", "wg_cpt2", "wg_cpt4"}
    # both sides of every switch: rows 63 | 64 and 2047 | 2048 at a wide row, cols 2040 | 2048, 8192 | 8200
    r = {(c.rows, c.cols): fk.route(c)[0] for c in norm}
    assert r[(63, 2048)] == "wave_cpl4" and r[(64, 2048)] == "wg_cpt1" and r[(2047, 2048)] == "wg_cpt1" and r[(2048, 2048)] == "wave_cpl4"
    assert r[(64, 2040)] == "wave_cpl4" and r[(64, 8192)] == "wg_cpt4" and r[(64, 8200)] == "wave_cpl0" and r[(63, 8192)] == "wave_cpl16"
    assert {c.cols for c in norm} == {8, 520, 1280, 1544, 2040, 2048, 2056, 4096, 8192, 8200} and {c.rows for c in norm} >= {1, 3, 5, 63, 64, 2047, 2048}
    for rt in {fk.route(c)[0] for c in norm}:                   # RMS and LayerNorm on every route; a bias, a stride and a row_map on both kernel families
        assert {c.rms for c in norm if fk.route(c)[0] == rt} == {0, 1}, rt
    for fam in ("wave", "wg"):
        sub = [c for c in norm if fk.route(c)[0].startswith(fam)]
        assert any(c.bias for c in sub) and any(c.ld for c in sub) and any(c.map and c.rows >= 3 for c in sub), fam
    pb = {(c.g, c.S): fk.route(c)[0] for c in CASES if c.op == "pullback"}
    assert pb == {(64, 256): "s256", (16, 64): "generic_regs", (8, 64): "generic_fallback", (16, 33): "generic_regs", (32, 32): "generic_regs"}, pb
    al = [c for c in CASES if c.op == "align"]
    assert {(c.K, c.D): fk.route(c)[0] for c in al if c.grads} == {(1, 8): "ny1", (5, 64): "ny1", (37, 200): "ny3", (256, 256): "ny4", (64, 640): "ny8"}
    assert {(c.grads, c.items) for c in al} == {(0, 1), (1, 1), (1, 3), (0, 3)} and {(c.K, c.D) for c in CASES if c.op == "cosine"} == {(c.K, c.D) for c in al}
    dec = {c.name: fk.route(c)[0] for c in CASES if c.op == "decode"}
    assert {c.pos for c in CASES if c.op == "decode" and fk.route(c)[0] == "splits16"} >= {0, 15, 16, 63, 64, 65, 129}          # pos 16: nk = 17, the splits 2 .. 15 are empty
    assert dec["decode-N3_h8_pos65"] == "splits10" and dec["decode-N33_h8_pos63_onesplit"] == "splits1" and dec["decode-N1_h2_pos64_noscratch"] == "splits1"
    assert dec["decode-N1_h2_pos129_smallscratch"] == "splits5" and fk.decode_scratch_floats([c for c in CASES if c.name == "decode-N33_h8_pos63_onesplit"][0]) > 0
    assert {fk.route(c)[0] for c in CASES if c.op == "stride"} == {"act_sweeps2", "swiglu_sweeps2"}
    assert {c.act for c in CASES if c.op == "act"} == set(fk.ACTS)
    assert {(c.M, c.HW) for c in CASES if c.op == "dice"} == {(m, hw) for m in (1, 3) for hw in (1, 255, 257, 4096)}


def test_bilinear_matrix_is_the_autograd_adjoint():
    """the separable weights the emulation and the mutants are built from reproduce the reference (F.interpolate's adjoint by autograd) in fp64"""
    import torch
    for g, S in ((16, 33), (8, 64), (32, 32)):
        m = torch.rand(2, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(S))
        U = fk.bilinear_matrix(S, g, torch.float64)
        sep = torch.einsum("py,kpq,qx->kyx", U, m, U).reshape(2, g * g)
        assert (sep - fk.pullback_adjoint(m, g, S)).abs().max() <= 1e-12 * S


def test_extra_bound_terms_are_needed_by_the_emulation():
    """without the RMS tie term and the pull-back coordinate term the emulation alone misses EMU_MAX; the figures the module's docstring quotes are recomputed here"""
    fk.PLAIN = True
    try:
        worst = {}
        for c in CASES:
            if (c.op == "norm" and c.rms) or c.op == "pullback":
                inp, ref, bounds = fk.reference.__wrapped__(c)
                got, _ = fk.OPS[c.op][1](c, inp, emu=True)
                n = "y" if c.op == "norm" else "pb"
                worst[c.op] = max(worst.get(c.op, (0.0, "")), (fk.ratio(got[n], ref[n], bounds[n]), c.name))
    finally:
        fk.PLAIN = False
    print(f"\nworst emulation ratio without the extra terms: {worst}")
    assert worst["norm"][1] == "norm-2048x2048_rms" and abs(worst["norm"][0] - 0.631) < 0.002, worst
    assert worst["pullback"][1] == "pullback-g16_S33_seam" and abs(worst["pullback"][0] - 26.1) < 0.1, worst
