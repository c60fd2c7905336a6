"""CPU: the tolerance of tests/test_attention_relpos_gpu.py has teeth.  On every case of the shared table (SAM's window, window-gather and
rel-pos grid attention), the bf16 emulation of what the kernels round passes the unchanged C_FWD / LSE_TOL rule of
tests/attention_edge_checks.py with a 2x margin, and every applicable mutant (a shifted, flipped, swapped, clamped or unscaled bias index, a
neighbour's rel rows, a dropped or duplicated key, a wrong pad row or window origin, the previous item's K / V, a rolled item mapping) fails
by at least 2x.  Run with -s to see each case's ratios and the per-mutant summary."""
import pytest
import torch

from tests import attention_relpos_checks as ar

CASES = ar.cases()
_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\nratio to the bound over the table (mutants: weakest, must be >= %g; emulation: worst, must be <= %g)" % (ar.MUT_MIN, ar.EMU_MAX))
        for n in sorted(_SEEN):
            emu = n.startswith("emulation")
            r, where = (max if emu else min)(_SEEN[n])
            print(f"  {n:42s} {r:12.3f}  at {where}  ({len(_SEEN[n])} cases)")


def _applicable(c):
    """the mutants that change case c's problem, from the case's shape alone"""
    m = {"h_index_plus_one", "h_index_sign_flipped", "last_key_row_takes_previous_row", "first_columns_keep_previous_row", "one_key_w_entry_off",
         "bias_scaled_by_scale", "no_bias", "drop_last_key"}
    if c.gh == c.gw:
        m.add("rel_h_w_swapped")
    if c.B > 1 and c.H > 1:
        m.add("rel_rows_batch_major")
    if c.kind in ("tab", "gather"):
        m.add("admit_key_196_as_copy_of_195")
    if c.kind == "gather" and c.g % ar.WS:
        m |= {"padded_token_is_zero", "pad_row_of_head_0_for_every_head"}
    if c.kind == "gather" and c.nw > 1:
        m.add("window_origin_transposed")
    if c.B * c.H > 1:
        m |= {"stale_kv_of_previous_item", "stale_v_only", "heads_rolled"}
    return m


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    emu = ar.emulation_ratios(case)
    mut = ar.mutant_ratios(case)
    assert {n for n in mut if not n.startswith("lse ")} == _applicable(case), "a mutant that changes this case's problem was not tried"
    for n, r in emu.items():
        _SEEN.setdefault("emulation " + n, []).append((r, case.name))
    for n, r in mut.items():
        _SEEN.setdefault(n, []).append((r, case.name))
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) +
          " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in sorted(mut.items(), key=lambda x: x[1])))
    assert all(r <= ar.EMU_MAX for r in emu.values()), f"the bf16 emulation exceeds {ar.EMU_MAX} of the bound: {emu}"
    weak = {n: r for n, r in mut.items() if not r >= ar.MUT_MIN}
    assert not weak, f"mutants the tolerance does not reject by {ar.MUT_MIN}x: {weak}"


def test_mutants_apply_across_the_table():
    names = set()
    for c in CASES:
        names |= _applicable(c)
    assert names == ar.ALL_MUTANTS


def test_case_table_reaches_every_route():
    """the shapes that the dispatch conditions of launch_hd need (profiles/attn_relpos_parity.md lists the condition per case)"""
    by = {c.name: c for c in CASES}
    assert len(by) == len(CASES)
    for n, items in (("win_b3_h2", 6), ("win_b5_h8", 40), ("win_b33_h8", 264)):       # one round; 5 rounds on 8 / 7 + 6 on 6 workgroups; 136 x 2 by default
        assert by[n].kind == "tab" and by[n].B * by[n].H == items and by[n].hd == 80
    assert {c.g for c in CASES if c.kind == "gather" and c.images == 2 and c.H == 2} == {15, 27, 28, 29}
    assert by["gather_g15_i3_h8"].B * by["gather_g15_i3_h8"].H == 96
    arr = {n: (c.hd, c.B, c.H, c.gh, c.gw) for n, c in by.items() if c.kind == "arr"}
    assert arr == {"rel14_hd80": (80, 3, 2, 14, 14), "rel14_hd64": (64, 3, 2, 14, 14), "rel9x21_hd80": (80, 2, 2, 9, 21), "rel21x9_hd80": (80, 2, 2, 21, 9),
                   "rel2x65_hd32": (32, 2, 2, 2, 65), "rel5x64_hd80": (80, 2, 2, 5, 64), "rel5x64_hd64": (64, 2, 2, 5, 64),
                   "rel17x64_hd80": (80, 1, 3, 17, 64), "rel16x64_hd64": (64, 1, 3, 16, 64), "rel16x64_hd80": (80, 1, 3, 16, 64),
                   "rel16x64_hd80_b3_h3": (80, 3, 3, 16, 64), "rel20x64_hd80": (80, 1, 2, 20, 64), "rel68x64_hd80": (80, 1, 1, 68, 64)}
    assert by["rel16x64_hd80"].lse and ar.has_lse(by["win_b3_h2"])
    for c in CASES:
        assert c.rel_ld >= 2 * max(c.gh, c.gw) - 1 + 4


def test_window_source_and_materialise():
    """g = 15: window (0, 1) holds a 14 x 1 strip, window (1, 1) a single real token; g = 28 has no padding; every token sits in one window row"""
    src = ar.window_source(15, 2)
    assert src.shape == (8, 196)
    assert [int((src[w] >= 0).sum()) for w in range(4)] == [196, 14, 14, 1]
    assert int(src[3, 0]) == 14 * 15 + 14 and int(src[1, 14 * 3]) == 3 * 15 + 14 and int(src[4, 0]) == 225
    assert bool((ar.window_source(28, 1) >= 0).all())
    for g in (15, 27, 28, 29):
        s = ar.window_source(g, 2)
        assert sorted(s[s >= 0].tolist()) == list(range(2 * g * g))
    tok = torch.arange(2 * 225 * 3 * 2, dtype=torch.float32).reshape(450, 3, 2)
    pad = -torch.ones(3, 2)
    w = ar.materialise(tok, pad, src)
    assert w.shape == (8, 3, 196, 2) and torch.equal(w[3, :, 0], tok[224]) and torch.equal(w[3, :, 1], pad) and torch.equal(w[4, :, 15], tok[225 + 16])


def test_rel_arrays_layout():
    """rel_arrays writes [H][B * N][rel_ld] with NaN in every column past 2 gh - 1 (rel_h) / 2 gw - 1 (rel_w)"""
    case = next(c for c in CASES if c.name == "rel9x21_hd80")
    P, _, (Gh, Gw) = ar.reference(case)
    rh, rw = ar.rel_arrays(case, Gh, Gw)
    assert rh.shape == rw.shape == (case.H, case.B * case.N, case.rel_ld) and rh.dtype == torch.float32
    assert bool(torch.isnan(rh[:, :, 17:]).all()) and bool(torch.isnan(rw[:, :, 41:]).all())
    assert not bool(torch.isnan(rh[:, :, :17]).any()) and not bool(torch.isnan(rw[:, :, :41]).any())
    assert float(rh[1, 1 * case.N + 7, 3]) == float(Gh[1, 1, 7, 3]) and float(rw[0, 1 * case.N + 100, 40]) == float(Gw[1, 0, 100, 40])


def test_reference_matches_dense_softmax():
    """attend() (batched, index-gathered bias) == torch.softmax over a bias filled in element by element from the formula, on the smallest non-square case"""
    case = next(c for c in CASES if c.name == "rel2x65_hd32")
    P, (ro, rl), (Gh, Gw) = ar.reference(case)
    qh, qw = ar.grid_coords(case.gh, case.gw)
    b, h = 1, 1
    q, k, v = (P[n][b, h].double() for n in "qkv")
    bias = torch.empty(case.N, case.N, dtype=torch.float64)
    for i in range(case.N):
        for j in range(case.N):
            bias[i, j] = Gh[b, h, i, qh[i] - qh[j] + case.gh - 1] + Gw[b, h, i, qw[i] - qw[j] + case.gw - 1]
    s = q @ k.t() * case.scale + bias
    assert float((torch.softmax(s, -1) @ v - ro[b, h]).abs().max()) < 1e-12
    assert float((torch.logsumexp(s, -1) / torch.log(torch.tensor(2.0, dtype=torch.float64)) - rl[b, h]).abs().max()) < 1e-12
