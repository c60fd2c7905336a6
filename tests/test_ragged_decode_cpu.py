"""CPU: the per-row decode_attn checks (tests/ragged_decode_checks.py) pass the emulation with a 2x margin and reject every applicable mutant by 2x on every
case; `pad_prompts` round-trips; the header declares the entry point and the binding follows its ABI version."""
import os
import re

import pytest
import torch

from tests import ragged_decode_checks as rc
from tests.ragged_decode_checks import EMU_MAX, MUT_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.cases()


def test_case_table_reaches_every_split_class():
    got = {c.name.split("-", 1)[1]: rc.splits(c) for c in CASES}
    assert got == {"N3_h2": 16, "N2_h2": 16, "N4_h8": 8, "N5_h64": 1, "N2_h2_noscratch": 1, "N1_h2_smallscratch": 5, "N2_h4_scores60": 16}, got
    assert [c.launches for c in CASES] == [2, 2, 2, 1, 1, 2, 2]
    c = CASES[0]                                            # pos 16 on 16 splits: one split of 16 keys and the owner of key 16; 14 splits hold nothing
    per = ((c.pos[1] + 1 + 15) // 16 + 15) // 16 * 16
    assert per == 16 and sum(1 for s in range(16) if s * per < c.pos[1] + 1) == 2


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_inputs_hold_the_sentinels_per_row(case):
    inp, ref, bounds = rc.reference(case)
    for n, p in enumerate(case.pos):
        for k in ("kc", "vc"):
            assert bool(torch.isfinite(inp[k][n, :p + 1].float()).all()) and bool(torch.isnan(inp[k][n, p + 1:].float()).all())
            assert bool(torch.isnan(ref[k][n, p + 1:]).all()) and bool((bounds[k][n, p + 1:] == 0).all()), "a sentinel beyond the row's position must stay, exactly"
            assert not torch.equal(ref[k][n, p], inp[k][n, p].double()), "the slot at the row's position takes the new row"
            assert torch.equal(ref[k][n, :p], inp[k][n, :p].double()) and bool((bounds[k][n, :p] == 0).all())
        assert bool((bounds["vc"][n, p] == 0).all()) and bool((bounds["kc"][n, p] > 0).all())
    assert bool(torch.isfinite(ref["out"]).all()) and bool((bounds["out"] > 0).all())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    emu = rc.emulation_ratios(case)
    print(f"\n{case.name}: emulation " + " ".join(f"{k}={v:.3f}" for k, v in emu.items()))
    assert max(emu.values()) <= EMU_MAX, emu
    mut = rc.mutant_ratios(case)
    print("  mutants " + " ".join(f"{k}={v:.3g}" for k, v in mut.items()))
    assert case.N == 1 or len(mut) >= 5, mut
    weak = {k: v for k, v in mut.items() if not v >= MUT_MIN}
    assert not weak, f"{case.name}: mutants within {MUT_MIN}x of the bound: {weak}"


def test_every_mutant_applies_somewhere():
    names = set()
    for c in CASES:
        names.update(rc.mutant_names(c))
    assert names == {"row0_pos_for_every_row", "longest_pos_for_every_row", "neighbour_rows_swap_positions", "rope_at_row_pos_keys_of_longest_row",
                     "append_at_row_pos_plus_1", "key_pos_excluded_per_row", "stale_cache_row_used_for_pos_per_row"}


def test_equal_positions_are_the_scalar_reference():
    """the row-by-row reference of a batch whose rows share a position is decode_compute's own batched result"""
    from tests import forward_kernel_checks as fk
    case = next(c for c in fk.cases() if c.name == "decode-N3_h8_pos65")
    inp, ref, _ = fk.reference(case)
    rows = rc.Case("decode_rows", "same", 0, N=case.N, heads=case.heads, pos=(case.pos,) * case.N, scratch=case.scratch, qscale=case.qscale)
    got, _ = rc.compute(rows, inp)
    for k in rc.OUTPUTS:
        assert torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(ref[k], nan=-7.0)), k


def test_pad_prompts_round_trips():
    from llmseg_amd.generate import pad_prompts
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, 1000, (n,), generator=g) for n in (24, 17, 9, 24, 1)]
    for pad in (0, 7, None):
        ids, mask = pad_prompts(prompts, pad)
        assert ids.shape == mask.shape == (5, 24) and ids.dtype == torch.int64 and mask.dtype == torch.bool
        for i, p in enumerate(prompts):
            assert torch.equal(ids[i][mask[i]], p) and torch.equal(ids[i, :p.numel()], p), "a row is its prompt, left-aligned"
            assert int(mask[i].sum()) == p.numel() and bool(mask[i, :p.numel()].all())
            assert bool((ids[i, p.numel():] == (0 if pad is None else pad)).all())
    ids, mask = pad_prompts(prompts[:1], 0)
    assert ids.shape == (1, 24) and bool(mask.all())


def test_header_declares_the_entry_point_and_the_binding_follows():
    from llmseg_amd import _lib
    src = open(os.path.join(ROOT, "include", "llmseg_hip.h")).read()
    assert re.search(r"\bint llmseg_decode_attn_rows\(", src)
    version = int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1))
    assert version == _lib.ABI_VERSION >= 14
    # the two entry points differ in the name of the position argument alone
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"int %s\((.*?)\);" % name, src, re.S).group(1))
    assert sig("llmseg_decode_attn_rows") == sig("llmseg_decode_attn").replace("pos_dev", "pos_rows_dev")
    table = open(os.path.join(ROOT, "llmseg_amd", "_lib.py")).read()
    rows = dict(re.findall(r'"(llmseg_decode_attn(?:_rows)?)": (\[.*?\])', table))
    assert rows["llmseg_decode_attn_rows"] == rows["llmseg_decode_attn"]
