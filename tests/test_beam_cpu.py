"""CPU: beam search -- the rule of tests/beam_checks.py against the installed transformers (`LlamaForCausalLM.generate(num_beams=...)` on a tiny random fp32
model built from a config); the case table of llmseg_beam_step meets its conditions (every gap among the 2 B + 1 best fp64 scores >= 16 x the bound, exact ties
only where planted, eos at the rank its case names); the fp32 / integer emulation of the kernel's arithmetic stays under the bound on every case with exact
picks; every named mutant fails a check; generate()'s host bookkeeping (`BeamBook`) driven by the rule's own picks returns the rule's winners; the header, the binding and INTEGRATION.md agree on the two symbols and bad arguments are refused before any launch."""
import ctypes as C
import functools
import math
import os
import re

import pytest
import torch

from tests import beam_checks as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bc.cases()
SETTINGS = [(3, 2, 1.0, False), (4, None, 1.0, False), (2, 7, 2.0, True), (3, 5, 0.5, False)]      # (beams, eos, length_penalty, early_stopping)
SEEDS = range(6)
MAX_NEW = 8
ARGS = {"llmseg_decode_attn_beams": ["qkv", "ld", "cos", "sin", "kcache", "vcache", "cache_stride_n", "pos_rows_dev", "src", "ld_src", "capacity", "N", "heads",
                                     "head_dim", "scale", "out", "ldo", "scratch", "scratch_bytes", "stream"],
        "llmseg_beam_step": ["logits", "ldl", "beam_scores", "done", "eos", "pad", "src_in", "src_out", "ld_src", "pos_rows", "N", "B", "beams_in", "V", "next_token",
                             "parent", "next_scores", "step_best", "fin_count", "fin_parent", "fin_score", "workspace", "workspace_bytes", "stream"]}


# ------------------------------------------------------------------------------------------------------------- the rule against transformers
@functools.lru_cache(maxsize=None)
def _hf_model(seed):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=24, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                      max_position_embeddings=64)
    m = LlamaForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(4.0)                                        # a distribution that is not flat
    g = torch.Generator().manual_seed(100 + seed)
    return m, [torch.randint(8, 24, (5,), generator=g), torch.randint(8, 24, (7,), generator=g)]


@functools.lru_cache(maxsize=None)
def _hf_run(seed, setting, which):
    B, eos, lp, early = setting
    m, prompts = _hf_model(seed)
    pr = prompts[which]
    with torch.no_grad():
        out = m.generate(pr[None], num_beams=B, max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=0, length_penalty=lp, early_stopping=early, do_sample=False,
                         return_dict_in_generate=True, output_scores=True, num_return_sequences=1)
    return out.sequences[0, len(pr):].tolist(), float(out.sequences_scores[0])


def _ours(seed, setting, which, mut=None):
    B, eos, lp, early = setting
    m, prompts = _hf_model(seed)
    pr = prompts[which]

    def logits_fn(seqs):
        ids = torch.stack([torch.cat([pr, torch.tensor(s, dtype=torch.long)]) for s in seqs])
        with torch.no_grad():
            return m(ids).logits[:, -1].float()
    return bc.search(logits_fn, B, eos, MAX_NEW, lp, early, mut)


def _agrees(seed, setting, which, mut=None):
    hf_toks, hf_score = _hf_run(seed, setting, which)
    _, (value, toks) = _ours(seed, setting, which, mut)
    return hf_toks[:len(toks)] == toks and abs(hf_score - value) <= 1e-4, len(toks), abs(hf_score - value)


@pytest.mark.parametrize("setting", SETTINGS, ids=[f"B{s[0]}_eos{s[1]}_lp{s[2]}_early{s[3]}" for s in SETTINGS])
def test_rule_against_the_installed_transformers(setting):
    early, worst = 0, 0.0
    for seed in SEEDS:
        for which in (0, 1):
            ok, n, err = _agrees(seed, setting, which)
            assert ok, f"seed {seed} prompt {which}: the rule and transformers differ ({_hf_run(seed, setting, which)} vs {_ours(seed, setting, which)[1]})"
            early += n < MAX_NEW
            worst = max(worst, err)
    print(f"\n{setting}: {early} of {2 * len(SEEDS)} runs ended before max_new_tokens; worst |sequences_scores - value| {worst:.2e}")
    if setting[1] is not None:                                 # a setting with an eos must exercise the eos and done rules
        assert early >= 1, f"{setting}: no run ended early"


def _table_search(seed, mut=None, V=6, B=2, eos=0, lp=1.0):
    """the loop on logits that are a fixed random function of the generated tokens (V small, so eos candidates are frequent)"""
    def logits_fn(seqs):
        return torch.stack([torch.randn(V, generator=torch.Generator().manual_seed(hash((seed,) + tuple(s)) % (2 ** 31))) * 2.0 for s in seqs])
    return bc.search(logits_fn, B, eos, 6, lp, False, mut)[1]


@pytest.mark.parametrize("mut", ("length_without_eos", "done_against_best_hypothesis", "eos_rank_ge_B_kept"))
def test_loop_mutants_are_caught(mut):
    """against transformers where its runs reach the defect, and against the rule itself (pinned above) on 80 small random logit tables"""
    hf = [(seed, s, w) for seed in SEEDS for s in SETTINGS for w in (0, 1) if s[1] is not None and not _agrees(seed, s, w, mut)[0]]
    tab = [(seed, kw["B"]) for seed in range(40) for kw in (dict(V=6, B=2), dict(V=8, B=3, lp=0.5)) if _table_search(seed, mut, **kw) != _table_search(seed, **kw)]
    print(f"\n{mut}: disagrees with transformers on {len(hf)} runs, with the rule on {len(tab)} of 80 tables")
    assert tab, f"the mutant {mut} passes every table"
    if mut != "done_against_best_hypothesis":                  # (no transformers run above reaches a step at which the best and the worst hypothesis decide differently)
        assert hf, f"the mutant {mut} passes every comparison with transformers"


# ------------------------------------------------------------------------------------------------------------------ llmseg_beam_step: the table
def test_case_table_covers_what_it_claims():
    assert {c.V for c in CASES} >= {1000, 32000, 32003} and {c.V - 2 * c.B for c in CASES} >= {0, 1}
    assert {c.B for c in CASES} == {2, 3, 4, 16} and {c.N for c in CASES} == {1, 3}
    assert {c.beams_in == 1 for c in CASES} == {True, False}
    assert {c.eos for c in CASES} == {"none", "rank0", "rankB-1", "rankB", "every_beam"} and {c.shape for c in CASES} == {"mixed", "identity", "allsame", "perm"}
    assert any(c.done and len(c.done) < c.N for c in CASES) and any(c.neg_inf for c in CASES) and any(c.ties for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_conditions(case):
    inp, ref, _ = bc.reference(case)
    ratio, zero = bc.gap_condition(case)
    print(f"\n{case.name}: smallest gap among the 2B + 1 best = {ratio:.1f} x (16 x bound), {zero} exact ties")
    assert ratio >= 1.0, f"{case.name}: a gap of {ratio:.3f} x (16 x bound): the order would not be decidable"
    assert (zero > 0) == case.ties, f"{case.name}: {zero} exact ties"
    B = case.B
    live = next(n for n in range(case.N) if n not in case.done)
    ranked = ref["ranked"][live]
    eos_ranks = [k for k, (_, v, _) in enumerate(ranked) if v == inp["eos"]]
    if case.eos == "none":
        assert inp["eos"] is None and int(ref["fin_count"].sum()) == 0
    if case.eos == "rank0":
        assert eos_ranks[0] == 0 and int(ref["fin_parent"][live, 0]) == ranked[0][0]
    if case.eos == "rankB-1":
        assert B - 1 in eos_ranks and int(ref["fin_count"][live]) == sum(k < B for k in eos_ranks) >= 1
    if case.eos == "rankB":
        assert B in eos_ranks and int(ref["fin_count"][live]) == sum(k < B for k in eos_ranks)            # present among the 2 B best, and not recorded
    if case.eos == "every_beam" and case.beams_in > 1:
        assert len({b for b, v, _ in ranked if v == inp["eos"]}) >= min(B, 2)
    par = ref["parent"].view(case.N, B)[live].tolist()
    if case.shape == "identity" and case.eos == "none":
        assert par == list(range(B))
    if case.shape == "perm":
        assert sorted(par) == list(range(B)) and par != list(range(B))
    if case.shape == "allsame":
        assert len(set(par)) == 1
    for n in case.done:                                        # a done prompt: pad, own slot, unchanged scores
        rows = slice(n * B, (n + 1) * B)
        assert ref["next_token"][rows].tolist() == [inp["pad"]] * B and ref["parent"][rows].tolist() == list(range(B)) and int(ref["fin_count"][n]) == 0
    if case.neg_inf:
        fin = torch.isfinite(inp["logits"].float()).sum(-1)
        assert int(fin.min()) >= 2 * B and bool((fin < case.V).all())
    # the table: what is not written keeps the sentinel; a first pick names row n * B for every prompt key
    src = ref["src_out"]
    for r in range(case.N * B):
        p = int(inp["pos_rows"][r])
        assert bool((src[r, p:] == bc.SENTINEL).all()) and bool((src[r, :p] >= 0).all()) and bool((src[r, :p] < case.N * B).all())
        if case.beams_in == 1:
            assert bool((src[r, :p] == r // B * B).all())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_of_the_kernels_arithmetic_stays_under_the_bound(case):
    bad, worst = bc.compare(case, bc.emulation(case))
    print(f"\n{case.name}: emulation error / bound = {worst:.3f}")
    assert not bad, f"{case.name}: {bad[:4]}"
    assert worst <= 1.0


def test_equal_logits_of_a_row_get_equal_scores_in_the_emulation():
    for case in (c for c in CASES if c.ties):
        inp, _, _ = bc.reference(case)
        sc = bc.emulated_scores(inp, case).view(case.N * case.beams_in, case.V)
        for r, pos in enumerate(inp["plant"]):
            assert float(sc[r, pos[0]]) == float(sc[r, pos[1]]) and float(sc[r, pos[2]]) == float(sc[r, pos[3]]) == float(sc[r, pos[4]])


@pytest.mark.parametrize("mut", ("eos_rank_ge_B_kept", "ties_by_larger_index") + bc.TABLE_MUTANTS)
def test_step_mutants_fail_the_comparison(mut):
    hit = [c.name for c in CASES if bc.compare(c, bc.mutant(c, mut), exact_only=True)[0]]
    print(f"\n{mut}: rejected on {len(hit)} cases: {hit[:6]}")
    assert hit, f"the mutant {mut} passes every case"
    if mut == "ties_by_larger_index":
        assert set(hit) <= {c.name for c in CASES if c.ties}
    if mut == "prompt_keys_from_own_row":
        assert set(hit) <= {c.name for c in CASES if c.beams_in == 1}


# -------------------------------------------------------------------------------------------------------------------- header, binding, library
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmseg_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("sym", sorted(ARGS))
def test_symbols_are_declared_bound_and_exported_with_the_headers_argument_order(sym):
    from llmseg_amd import _lib
    src = _header()
    assert re.search(r"\bint\s+%s\s*\(" % sym, src), f"{sym} is not declared in include/llmseg_hip.h"
    assert sym in _lib.SIGNATURES, f"{sym} is not bound in llmseg_amd/_lib.py"
    decl = re.search(r"%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")
    assert [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", a)[-1] for a in decl] == ARGS[sym]
    kinds = [C.c_void_p if "*" in a else C.c_float if "float" in a else C.c_int32 if "int32_t" in a else C.c_int64 for a in decl]
    assert _lib.SIGNATURES[sym] == kinds
    assert int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION >= 18
    lib = _lib.load()
    assert hasattr(lib, sym)
    assert lib.llmseg_struct_size(6) == -1                     # plain argument lists: no new argument struct
    assert re.search(r"llmseg_version\(\) == %d\b" % _lib.ABI_VERSION, open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert sym in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "beam.hip" in open(os.path.join(ROOT, "llmseg_amd", "csrc", "build.sh")).read()


def test_beam_step_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    ok = dict(logits=4096, ldl=40, beam_scores=4096, done=4096, eos=2, pad=0, src_in=4096, src_out=8192, ld_src=16, pos_rows=4096, N=2, B=3, beams_in=3, V=33,
              next_token=4096, parent=4096, next_scores=4096, step_best=4096, fin_count=4096, fin_parent=4096, fin_score=4096, workspace=4096, workspace_bytes=2 * 3 * 6 * 8)
    ptrs = ("logits", "beam_scores", "done", "src_in", "src_out", "pos_rows", "next_token", "parent", "next_scores", "step_best", "fin_count", "fin_parent", "fin_score",
            "workspace")
    bads = [dict({k: None}) for k in ptrs] + [dict(src_out=4096), dict(B=1), dict(B=17), dict(beams_in=2), dict(beams_in=0), dict(V=5), dict(ldl=32), dict(N=0),
                                                dict(ld_src=0), dict(eos=33), dict(pad=-1), dict(workspace_bytes=2 * 3 * 6 * 8 - 1), dict(logits=4097), dict(beam_scores=4098),
                                                dict(src_in=4098), dict(next_token=4100), dict(workspace=4100), dict(fin_score=4097), dict(V=(1 << 22) + 1, ldl=1 << 23)]
    n0 = lib.llmseg_launch_count()
    for bad in bads:
        a = dict(ok, **bad)
        rc = lib.llmseg_beam_step(p(a["logits"]), a["ldl"], p(a["beam_scores"]), p(a["done"]), a["eos"], a["pad"], p(a["src_in"]), p(a["src_out"]), a["ld_src"],
                                  p(a["pos_rows"]), a["N"], a["B"], a["beams_in"], a["V"], p(a["next_token"]), p(a["parent"]), p(a["next_scores"]), p(a["step_best"]),
                                  p(a["fin_count"]), p(a["fin_parent"]), p(a["fin_score"]), p(a["workspace"]), a["workspace_bytes"], None)
        assert rc == -1 and b"beam_step" in lib.llmseg_last_error(), bad
    assert lib.llmseg_launch_count() == n0


def test_decode_attn_beams_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    ok = dict(qkv=4096, ld=768, cos=4096, sin=4096, kcache=4096, vcache=4096, cache_stride_n=64 * 256, pos=4096, src=4096, ld_src=64, capacity=64, N=2, heads=2,
              head_dim=128, out=4096, ldo=256)
    bads = [dict(src=None), dict(src=4098), dict(ld_src=63), dict(capacity=0), dict(qkv=None), dict(pos=None), dict(out=None), dict(head_dim=64), dict(ld=772),
            dict(cache_stride_n=100), dict(kcache=4104), dict(N=0), dict(heads=0)]
    n0 = lib.llmseg_launch_count()
    for bad in bads:
        a = dict(ok, **bad)
        rc = lib.llmseg_decode_attn_beams(p(a["qkv"]), a["ld"], p(a["cos"]), p(a["sin"]), p(a["kcache"]), p(a["vcache"]), a["cache_stride_n"], p(a["pos"]), p(a["src"]),
                                          a["ld_src"], a["capacity"], a["N"], a["heads"], a["head_dim"], 0.1, p(a["out"]), a["ldo"], None, 0, None)
        assert rc == -1 and b"decode_attn_beams" in lib.llmseg_last_error(), bad
    assert lib.llmseg_launch_count() == n0


# ------------------------------------------------------------------------------------------------------ generate()'s host bookkeeping: BeamBook
BOOK_MAX_NEW, BOOK_V, BOOK_PAD = 4, 8, 7
BOOK_SETTINGS = [(B, eos, lp, early) for B in (2, 3) for eos in (1, None) for lp in (0.5, 1.0, 2.0) for early in (False, True)]


def _book_logits(n):
    """prompt n's logits, a fixed function of its generated tokens: V = 8, eos = 1 likely enough to finish hypotheses, prompt 0 much more so than prompt 1"""
    def logits_fn(seqs):
        rows = []
        for s in seqs:
            l = torch.randn(BOOK_V, generator=torch.Generator().manual_seed(1000 * n + sum((i + 1) * (t + 1) * 31 ** i for i, t in enumerate(s)))).double() * 1.5
            l[1] += (1.0 + 2.0 * len(s)) * (1 - n) - 1.0 * n
            rows.append(l)
        return torch.stack(rows)
    return logits_fn


@pytest.mark.parametrize("setting", BOOK_SETTINGS, ids=[f"B{s[0]}_eos{s[1]}_lp{s[2]}_early{s[3]}" for s in BOOK_SETTINGS])
def test_beam_book_keeps_the_rules_pools_and_backtraces_the_winner(setting):
    """generate()'s loop without a device: per pick the records `llmseg_beam_step` would write, made by `walk` on hand-built logits (a done prompt's rows emit pad from
    their own slots, as the kernel's do), go through `BeamBook.step`; `BeamBook.finish` must return, for both prompts, the winner of `beam_checks.search`."""
    from llmseg_amd.generate import BeamBook
    B, eos, lp, early = setting
    N = 2
    want = [bc.search(_book_logits(n), B, eos, BOOK_MAX_NEW, lp, early) for n in range(N)]
    for n, (p, _) in enumerate(want):                          # the reference side: no two hypotheses a pool ever met have the same value (else the winner is not unique)
        vals = [s / (g + 1) ** lp for g, pick in enumerate(p.picks) for _, s in pick["fin"]] + ([] if p.done else [s / p.steps ** lp for s in p.scores])
        assert len(set(vals)) == len(vals), f"prompt {n}: equal values among the hypotheses {vals}"
    book = BeamBook(N, B, float(lp), early, eos)
    seqs, scores = [[[]] for _ in range(N)], [[0.0] for _ in range(N)]
    tokens, parents, step, done_after = [], [], 0, [None] * N
    while True:
        rec = dict(step_best=[0.0] * N, fin_count=[0] * N, fin_parent=[[-7] * B for _ in range(N)], fin_score=[[math.nan] * B for _ in range(N)])
        tok, par = [], []
        for n in range(N):
            if book.done[n]:
                tok, par = tok + [BOOK_PAD] * B, par + list(range(B))          # (its scores stay as they are)
                continue
            lg = _book_logits(n)(seqs[n])
            pick = bc.walk(torch.tensor(scores[n], dtype=torch.float64)[:, None] + lg - torch.logsumexp(lg, -1, keepdim=True), B, eos)
            rec["step_best"][n], rec["fin_count"][n] = pick["best"], len(pick["fin"])
            for k, (b, s) in enumerate(pick["fin"]):
                rec["fin_parent"][n][k], rec["fin_score"][n][k] = b, s
            seqs[n], scores[n] = [seqs[n][b] + [v] for b, v in zip(pick["parents"], pick["tokens"])], pick["scores"]
            tok, par = tok + pick["tokens"], par + pick["parents"]
        tokens.append(tok)
        parents.append(par)
        book.step(step, **rec)
        step += 1
        done_after = [step if d and a is None else a for d, a in zip(book.done, done_after)]
        if all(book.done) or step == BOOK_MAX_NEW:
            break
    winners = book.finish([s for n in range(N) for s in scores[n]], tokens, parents)
    print(f"\n{setting}: {step} picks, the prompts end after {[p.steps for p, _ in want]}, done {book.done}, winners {[(w[0], round(w[1], 4)) for w in winners]}")
    assert done_after == [p.steps if p.done else None for p, _ in want] and step == max(p.steps for p, _ in want), "a prompt is done at another pick than the rule's"
    for n, ((p, (value, toks)), (seq, val, gather)) in enumerate(zip(want, winners)):
        assert seq == toks, f"prompt {n}: tokens {seq}, the rule's {toks}"
        assert abs(val - value) <= 1e-4, f"prompt {n}: value {val!r}, the rule's {value!r}"
        # the hidden state of every fed token: pick t's row of the beam that carries the winner there, i.e. whose tokens so far are the winner's first t + 1
        assert all(n * B <= g - t * N * B < (n + 1) * B for t, g in enumerate(gather)) and [tokens[t][g - t * N * B] for t, g in enumerate(gather)] == seq[:-1]
    if eos is not None and (early or B == 2):                  # (three beams: the pool's worst outranks the best candidate only at the last pick)
        assert want[0][0].steps < want[1][0].steps, "the case must finish one prompt before the other"


def test_generate_signature_and_defaults():
    import inspect
    from llmseg_amd.generate import GenerateMixin
    from llmseg_amd.sam_decoder import SamDecoderMixin
    sig = inspect.signature(GenerateMixin.generate).parameters
    assert [sig[k].default for k in ("num_beams", "length_penalty", "early_stopping", "return_beam_scores", "beam_cache")] == [1, 1.0, False, False, "indirect"]
    ev = inspect.signature(SamDecoderMixin.evaluate).parameters
    assert [ev[k].default for k in ("num_beams", "length_penalty", "early_stopping")] == [1, 1.0, False]
