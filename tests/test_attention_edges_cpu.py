"""CPU: the tolerance of tests/test_attention_edges_gpu.py has teeth.  On every case of the shared table, the bf16 emulation of what the
attention kernels round passes with a 2x margin, and every applicable mutant (an fp64 result of a subtly wrong problem: an off-by-one
key mask or causal edge, a skipped partial tile, a neighbour's mask, a dropped delta, an unmasked gradient pass, a natural-log or
incomplete lse) fails by at least 2x.  Run with -s to see each case's ratios and the per-mutant summary."""
import pytest

from tests import attention_edge_checks as ae

CASES = ae.cases()
_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\nratio to the bound over the table (mutants: weakest, must be >= %g; emulation: worst, must be <= %g)" % (ae.MUT_MIN, ae.EMU_MAX))
        for n in sorted(_SEEN):
            emu = n.startswith("emulation")
            r, where = (max if emu else min)(_SEEN[n])
            print(f"  {n:42s} {r:12.3f}  at {where}  ({len(_SEEN[n])} cases)")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    emu = ae.emulation_ratios(case)
    mut = ae.mutant_ratios(case)
    for n, r in emu.items():
        _SEEN.setdefault("emulation " + n, []).append((r, case.name))
    for n, r in mut.items():
        _SEEN.setdefault(n, []).append((r, case.name))
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) +
          " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in sorted(mut.items(), key=lambda x: x[1])))
    assert all(r <= ae.EMU_MAX for r in emu.values()), f"the bf16 emulation exceeds {ae.EMU_MAX} of the bound: {emu}"
    weak = {n: r for n, r in mut.items() if not r >= ae.MUT_MIN}
    assert not weak, f"mutants the tolerance does not reject by {ae.MUT_MIN}x: {weak}"


def test_mutants_apply_across_the_table():
    """every mutant of the list applies somewhere in the table (so none is silently never tried)"""
    names = set()
    for c in CASES:
        names |= {"fwd " + n for n in ae.mutant_masks(c)}
    assert names == {"fwd drop_last_valid_key", "fwd admit_one_padded_key", "fwd causal_key_lt_q", "fwd causal_key_le_q+1",
                     "fwd last_partial_tile_ignored", "fwd mask_of_b_on_b+1"}, names
    assert any(c.bwd and c.lens is not None for c in CASES)       # where the backward-only key-mask mutants apply


def test_explicit_backward_equals_autograd():
    """the explicit backward (D from a given O) that the GPU test and the emulation use equals fp64 autograd when O is exact"""
    for name in ("T129_hd32_plain_mask", "T319_hd128_causal_mask", "cross300x70_hd128_mask"):
        case = next(c for c in CASES if c.name == name)
        (q, k, v, do), (o, _), rb = ae.reference(case)
        g = ae.attn_bwd_ref(q, k, v, case.scale, case.causal, case.key_mask(), do, o=o)
        for a, b in zip(g, rb):
            assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max())), name


def test_case_table_covers_the_edges():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for T in ae.TS:
        for form in ("plain_nomask", "causal_nomask", "plain_mask", "causal_mask"):
            assert any(n.startswith(f"T{T}_") and n.endswith(form) for n in names), (T, form)
    for c in CASES:
        if c.lens is not None and c.name.startswith("T"):
            assert len(c.lens) >= 4 and {L for L in (1, 63, 64, 65, 128, c.Nk - 1, c.Nk) if 1 <= L <= c.Nk} <= set(c.lens), c
    assert len({(c.hd, c.causal, c.lens is not None) for c in CASES if c.name.startswith("T")}) == 12
    assert {(c.Nq, c.Nk) for c in CASES if c.Nq != c.Nk} == {(70, 300), (300, 70)}
    wide = [c for c in CASES if c.Nq >= 1024]
    assert {c.Nq for c in wide} == {1024, 1025, 4097} and any(c.lens for c in wide) and any(c.nk_valid for c in wide)
    assert all(not c.causal and not c.bwd for c in wide)
