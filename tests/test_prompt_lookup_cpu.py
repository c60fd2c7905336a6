"""CPU: prompt-lookup decoding.  The restated draft rule equals the installed transformers' PromptLookupCandidateGenerator; the accept rule on hand-built logit
tables; the restated loop returns the oracle's greedy sequences on any forward (a seeded fp64 toy model and the tiny oracle model), unforced and under forced
drafts; every rule mutant fails one of those; the chunk-attention checks (tests/lookup_checks.py) pass the emulation with a 2x margin and reject every applicable
mutant by 2x on every case; the header declares the three entry points at ABI 22."""
import os
import re

import pytest
import torch

from tests import lookup_checks as lc
from tests.lookup_checks import EMU_MAX, MUT_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = lc.chunk_cases()


# 1 --------------------------------------------------------------------------------------------------------------------------------------------
def test_draft_rule_equals_the_installed_candidate_generator():
    """The restatement follows the installed class everywhere but at an eos inside a candidate (the class cuts the candidate there; here the accept rule ends the
    emission after the first eos, so the eos may be drafted -- the comparison therefore runs the class without an eos id) and at ids outside the vocabulary,
    which the class does not know (checked below on its own)."""
    bad = lc.check_draft(lc.draft)
    assert not bad, bad[:5]
    assert len(lc.draft_random_cases()) >= 300
    n_match = sum(1 for h, k, g in lc.draft_random_cases() if lc.draft(h, k, g))
    assert n_match >= 200, n_match                            # matches abound


def test_draft_cuts():
    h = [1, 2, 3, 4, 5, 1, 2]
    assert lc.draft(h, 5, 2) == [3, 4, 5, 1, 2]
    assert [lc.draft(h, 5, 2, limit=m) for m in (0, 1, 3, 9)] == [[], [3], [3, 4, 5], [3, 4, 5, 1, 2]]
    hi = [1, 2, 3, lc.IMAGE, 5, 1, 2]                          # the placeholder takes part in the windows as a value and ends a draft
    assert lc.draft(hi, 5, 2, vocab=10) == [3] and lc.draft(hi, 5, 2) == [3, lc.IMAGE, 5, 1, 2]
    assert lc.draft([lc.IMAGE, 7, 4, lc.IMAGE], 3, 2, vocab=10) == [7, 4] and lc.draft([4, lc.IMAGE, 7, 4], 3, 2, vocab=10) == []
    assert lc.draft([1, 2, 3, 11, 1, 2], 3, 2, vocab=10) == [3]


# 2 --------------------------------------------------------------------------------------------------------------------------------------------
def test_accept_rule_on_hand_built_tables():
    bad = lc.check_accept(lc.accept)
    assert not bad, bad
    names = {c[0] for c in lc.accept_cases()}
    assert {"all_accepted", "none_accepted", "partial", "accepted_draft_is_eos", "max_new_cut_mid_chunk", "finished_row", "two_equal_maxima_lowest_wins"} <= names
    first = lc.accept([], 0, [4], 0, 1, 5, 4, 30, first=True)  # the pick after the prefill: nothing was fed, the position stays
    assert first == dict(accepted=0, emitted=[4], count=1, unfinished=0, pos=30, stand=0)


# 3 --------------------------------------------------------------------------------------------------------------------------------------------
def test_loop_returns_the_greedy_sequences_on_the_toy_forward():
    bad = lc.check_invariance()
    assert not bad, bad[:3]
    table = lc.invariance_cases()
    assert {c[3] for c in table} == {1, 2, 3, 4, 5, 7} and {c[5] for c in table} == {None, 1, 4} and {c[6] for c in table} == {1, 2, 9, 24}


def test_toy_table_accepts_drafts_and_finishes_rows_inside_chunks():
    """the table is no formality: drafts are accepted, rejected and cut by eos inside a chunk somewhere in it"""
    acc = rej = eos_mid = 0
    for seed, N, L, k, g, eos, max_new in lc.invariance_cases():
        _, per_row = lc.toy_forward(seed)
        ids = torch.randint(0, 6, (N, L), generator=torch.Generator().manual_seed(seed))
        trace = []
        seqs, counts = lc.lookup_generate(per_row, [r.tolist() for r in ids], k, g, max_new, eos=eos, trace=trace)
        for t in trace:
            acc += sum(t["accepted"])
            rej += sum(d - a for d, a in zip(t["draft_len"], t["accepted"]))
        for n in range(N):
            if eos is not None and counts[n] < max_new and seqs[n][-1] == eos:
                full, _ = lc.lookup_generate(per_row, [ids[n].tolist()], k, g, max_new, eos=None)
                eos_mid += full[0][L:].index(eos) + 1 == counts[n]
    print(f"\naccepted {acc}, rejected {rej}, rows finished by eos {eos_mid}")
    assert acc >= 50 and rej >= 50 and eos_mid >= 10


@pytest.mark.parametrize("k,g", ((1, 2), (3, 2), (7, 3)))
def test_loop_returns_the_greedy_sequences_on_the_tiny_oracle_model(k, g):
    from oracle import cases, generate as ogen, lisa as olisa
    cfg = cases.tiny_lisa_cfg()
    sd = {n: v.to(torch.bfloat16).float() for n, v in cases.tiny_lisa_state(cfg).items()}
    batch = cases.tiny_lisa_batch()
    clip, ids = batch["images_clip"][:2], batch["input_ids"][:2]
    L, max_new = ids.shape[1], 6
    with torch.no_grad():
        free, _ = ogen.greedy_generate(sd, cfg, clip, ids, max_new_tokens=max_new, eos_token_id=None)
        eos = int(free[0, L + 2])

        def fwd(n, row):                                        # the last len(row) positions: behind the <image> token (index 2) they are the ids' own, one to one
            t = torch.tensor([row], dtype=torch.int64)
            return olisa.llava_forward(sd, cfg, clip[n:n + 1], torch.ones_like(t, dtype=torch.bool), t)[1][0, -len(row):].double()
        for e in (None, eos):
            want, _ = ogen.greedy_generate(sd, cfg, clip, ids, max_new_tokens=max_new, eos_token_id=e, pad_token_id=0)
            prompts = [r.tolist() for r in ids]
            for kind in (None, "right", "mixed"):
                forced = None if kind is None else lc.forced_drafts(free[:, L:], kind, cfg.llama.vocab).tolist()
                seqs, counts = lc.lookup_generate(fwd, prompts, k, g, max_new, eos=e, forced=forced, vocab=cfg.llama.vocab)
                got = lc.pack(prompts, seqs, counts, 0)
                assert torch.equal(got, want), (k, g, e, kind, got[:, L:].tolist(), want[:, L:].tolist())


# 4 --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.RULE_MUTANTS)
def test_rule_mutants_fail(name):
    f = lc.mutant_failures(name)
    print(f"\n{name}: " + " ".join(f"{k}={len(v)}" for k, v in f.items()))
    assert any(f.values()), f"{name} passes the draft, accept and invariance checks"


# 5 --------------------------------------------------------------------------------------------------------------------------------------------
def test_chunk_case_table():
    got = {c.name.split("-", 1)[1]: (lc.chunk_splits(c), c.launches) for c in CHUNK}
    assert got == {"Q1_N3_h2": (16, 2), "Q2_N3_h2": (16, 2), "Q5_N3_h2": (16, 2), "Q8_N3_h2": (16, 2), "Q8_N2_h2_noscratch_trip": (1, 1), "Q5_N2_h2_group_edge": (16, 2),
                   "Q2_N5_h64": (1, 1), "Q5_N1_h2_smallscratch": (5, 2), "Q3_N2_h4_scores60": (16, 2)}, got
    assert any(p + c.Q == lc.CAP for c in CHUNK for p in c.pos), "one chunk must end exactly at the capacity"
    trip = next(c for c in CHUNK if "trip" in c.name)
    assert trip.pos[0] < 64 <= trip.pos[0] + trip.Q - 1 and lc.chunk_splits(trip) == 1
    names = set()
    for c in CHUNK:
        names.update(lc.chunk_mutant_names(c))
    assert names == {"query_sees_next_chunk_key", "every_query_rotated_at_pos", "stale_slot_read", "row_takes_neighbour_position"}


@pytest.mark.parametrize("case", CHUNK, ids=[c.name for c in CHUNK])
def test_chunk_inputs_hold_the_sentinels(case):
    inp, ref, bounds = lc.chunk_reference(case)
    Q = case.Q
    for n, p in enumerate(case.pos):
        for k in ("kc", "vc"):
            assert bool(torch.isfinite(inp[k][n, :p + Q].float()).all()) and bool(torch.isnan(inp[k][n, p + Q:].float()).all())
            assert bool(torch.isnan(ref[k][n, p + Q:]).all()) and bool((bounds[k][n, p + Q:] == 0).all())
            assert torch.equal(ref[k][n, :p], inp[k][n, :p].double()) and bool((bounds[k][n, :p] == 0).all())
            for j in range(Q):
                assert not torch.equal(ref[k][n, p + j], inp[k][n, p + j].double()), "every slot of the chunk takes its new row"
        assert bool((bounds["vc"][n, p:p + Q] == 0).all()) and bool((bounds["kc"][n, p:p + Q] > 0).all())
    assert ref["out"].shape[0] == case.N * Q and bool(torch.isfinite(ref["out"]).all()) and bool((bounds["out"] > 0).all())


def test_chunk_of_one_is_the_per_row_reference():
    from tests import ragged_decode_checks as rc
    case = next(c for c in CHUNK if c.Q == 1)
    inp, ref, _ = lc.chunk_reference(case)
    rows = rc.Case("decode_rows", "same", 0, N=case.N, heads=case.heads, pos=case.pos, scratch=case.scratch, qscale=case.qscale)
    got, _ = rc.compute(rows, inp)
    for k in lc.OUTPUTS:
        assert torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(ref[k], nan=-7.0)), k


@pytest.mark.parametrize("case", CHUNK, ids=[c.name for c in CHUNK])
def test_chunk_emulation_passes_and_mutants_fail(case):
    emu = lc.chunk_emulation_ratios(case)
    print(f"\n{case.name}: emulation " + " ".join(f"{k}={v:.3f}" for k, v in emu.items()))
    assert max(emu.values()) <= EMU_MAX, emu
    mut = lc.chunk_mutant_ratios(case)
    print("  mutants " + " ".join(f"{k}={v:.3g}" for k, v in mut.items()))
    weak = {k: v for k, v in mut.items() if not v >= MUT_MIN}
    assert not weak, f"{case.name}: mutants within {MUT_MIN}x of the bound: {weak}"


# -----------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_follows():
    from llmseg_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "llmseg_hip.h")).read()
    for name in ("llmseg_decode_attn_chunk", "llmseg_lookup_draft", "llmseg_lookup_accept"):
        assert re.search(r"\bint %s\(" % name, src) and name in _lib.SIGNATURES, name
        n_args = len(re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % name, src, re.S).group(1), flags=re.S).split(","))
        assert n_args == len(_lib.SIGNATURES[name]), (name, n_args)
    assert int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION >= 22
    assert int(re.search(r"#define LLMSEG_DECODE_CHUNK_MAX (\d+)", src).group(1)) == ops.DECODE_CHUNK_MAX == 8
    assert "lookup.hip" in open(os.path.join(ROOT, "llmseg_amd", "csrc", "build.sh")).read()


def test_check_lookup_refuses_what_is_out_of_scope():
    import types
    from llmseg_amd.generate import _check_lookup
    model = types.SimpleNamespace(config=types.SimpleNamespace(llama=types.SimpleNamespace(head_dim=128)))
    ids = torch.zeros((2, 5), dtype=torch.int64)
    ok = dict(forced=None, trace=None, input_ids=ids, max_new_tokens=4, do_sample=False, num_beams=1, controls=None, kv=(), fuse_decode=True)
    assert _check_lookup(model, None, 2, **ok) is None and _check_lookup(model, 3, 2, **ok) == (3, 2) and _check_lookup(model, 7, 1, **ok) == (7, 1)
    for k, g in ((0, 2), (8, 2), (True, 2), (2.0, 2), (3, 0), (3, None), (None, 3)):
        with pytest.raises(ValueError):
            _check_lookup(model, k, g, **ok)
    for kw, word in ((dict(do_sample=True), "do_sample"), (dict(num_beams=2), "num_beams"), (dict(controls=dict(repetition_penalty=1.2)), "repetition_penalty"),
                     (dict(kv=("kv", "mxfp8", "packed")), "kv_format"), (dict(fuse_decode=False), "fuse_decode"), (dict(forced=torch.zeros((2, 3), dtype=torch.int64)), "_lookup_forced")):
        with pytest.raises(ValueError, match=word):
            _check_lookup(model, 3, 2, **{**ok, **kw})
    model.config.llama.head_dim = 64
    with pytest.raises(ValueError, match="head_dim 128"):
        _check_lookup(model, 3, 2, **ok)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        _check_lookup(model, None, 2, **{**ok, "trace": []})
