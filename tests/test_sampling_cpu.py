"""CPU: sampling -- the header, the binding and the library agree on llmseg_sample_tokens and every bad argument is refused before any launch; the fp64 restatement of
the rule (tests/sampling_checks.py) gives the hand-written kept sets and stands in the stated relation to the installed transformers warpers; on every case the two
fp64 kept sets at 1 - p -+ delta_p are equal (no case is silently loose), the fp32 / integer emulation of the kernel stays at <= EMU_MAX of the bounds, and every
named mutant exceeds them by >= MUT_MIN on several cases.  No GPU: the entry point is only called where it must refuse before touching the device."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests import sampling_checks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
ARGS = ["logits", "ldl", "N", "V", "temperature", "top_k", "top_p", "u", "eos", "pad", "unfinished", "next", "logprob", "kept", "probs", "ldp", "stream"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmseg_hip.h")).read(), flags=re.S)


def test_symbol_is_declared_bound_and_exported_with_the_headers_argument_order():
    from llmseg_amd import _lib
    src = _header()
    assert re.search(r"\bint\s+llmseg_sample_tokens\s*\(", src), "llmseg_sample_tokens is not declared in include/llmseg_hip.h"
    assert "llmseg_sample_tokens" in _lib.SIGNATURES, "llmseg_sample_tokens is not bound in llmseg_amd/_lib.py"
    decl = re.search(r"llmseg_sample_tokens\s*\((.*?)\)\s*;", src, flags=re.S).group(1).split(",")
    assert [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", a)[-1] for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_float if "float" in a else C.c_int32 if "int32_t" in a else C.c_int64 for a in decl]
    assert _lib.SIGNATURES["llmseg_sample_tokens"] == kinds
    assert int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION >= 16
    lib = _lib.load()
    assert hasattr(lib, "llmseg_sample_tokens")
    assert lib.llmseg_struct_size(6) == -1                                   # a plain argument list: no argument struct of its own (5, the last index, is llmseg_lora_down_args)
    assert re.search(r"llmseg_version\(\) == %d\b" % _lib.ABI_VERSION, open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert "sample.hip" in open(os.path.join(ROOT, "llmseg_amd", "csrc", "build.sh")).read()


def test_every_bad_argument_is_refused_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    ok = dict(logits=4096, ldl=40, N=2, V=33, temperature=1.0, top_k=0, top_p=1.0, u=4096, eos=2, pad=0, unfinished=4096, next=4096, logprob=4096, kept=4096,
              probs=4096, ldp=33)
    bads = (dict(logits=None), dict(u=None), dict(next=None), dict(N=0), dict(V=0), dict(V=2 ** 31), dict(N=2 ** 31), dict(ldl=32), dict(ldp=32),
            dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf), dict(temperature=math.nan), dict(top_k=-1),
            dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001), dict(top_p=math.nan),
            dict(logits=4097), dict(u=4098), dict(next=4100), dict(unfinished=4100), dict(logprob=4098), dict(kept=4097), dict(probs=4098))
    for bad in bads:
        a = dict(ok, **bad)
        rc = lib.llmseg_sample_tokens(p(a["logits"]), a["ldl"], a["N"], a["V"], a["temperature"], a["top_k"], a["top_p"], p(a["u"]), a["eos"], a["pad"], p(a["unfinished"]),
                                      p(a["next"]), p(a["logprob"]), p(a["kept"]), p(a["probs"]), a["ldp"], None)
        assert rc == -1 and b"sample_tokens" in lib.llmseg_last_error(), bad


@pytest.mark.parametrize("row", sc.HAND, ids=[h[0] for h in sc.HAND])
def test_rule_on_hand_built_rows(row):
    _, logits, T, k, p, kept = row
    l = torch.tensor(logits).to(sc.BF)
    ref = sc.rule(l, T, k, p)
    assert ref["K2"].nonzero().flatten().tolist() == kept
    assert abs(float(ref["r"].sum()) - 1.0) < 1e-12 and bool((ref["r"][~ref["K2"]] == 0).all())
    # the draw walks token ids: u = 0 gives the first kept id, u just below 1 the last
    assert sc.draw(ref, 0.0) == kept[0] and sc.draw(ref, sc.U_MAX) == kept[-1]
    # the emulation of the kernel keeps the same set and renormalises over it
    tok, lp, n_kept, probs = sc._emulate_row(l, T, k, p, torch.tensor(0.0))
    assert (probs > 0).nonzero().flatten().tolist() == kept and n_kept == len(kept) and tok == kept[0]
    assert abs(float(lp) - math.log(float(ref["r"][tok]))) < 1e-5


def test_draw_is_in_token_id_order_with_the_stated_inequality():
    l = torch.tensor([0.0, 0.0, 0.0, 0.0]).to(sc.BF)                          # r = 1/4 each, C = 1/4, 1/2, 3/4, 1
    ref = sc.rule(l, 1.0, 0, 1.0)
    assert [sc.draw(ref, u) for u in (0.0, 0.2499, 0.25, 0.4999, 0.5, 0.75, sc.U_MAX)] == [0, 0, 1, 1, 2, 3, 3]     # C_i > u, strictly


@pytest.mark.parametrize("V", sc.HF_V)
def test_rule_against_the_transformers_warpers(V):
    """superset; extras only at the smallest kept logit; the filtered softmax within HF_TOL elsewhere"""
    pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(V)
    l = (3.0 * torch.randn(V, generator=g)).to(sc.BF)
    n_extra = 0
    for T, k, p in sc.HF_SETTINGS:
        hf = sc.hf_filtered_softmax(l, T, k, p).double()
        ref = sc.rule(l, T, k, p)
        mine, theirs = ref["K2"], hf > 0
        assert bool((theirs <= mine).all()), (V, T, k, p, "HF keeps a token the rule drops")
        extra = mine & ~theirs
        z = l.double()
        assert bool((z[extra] == z[mine].min()).all()), (V, T, k, p, "an extra token is not at the smallest kept logit")
        n_extra += int(extra.sum())
        if bool(extra.any()):                                                  # renormalise the rule over HF's set to compare the rest
            r = torch.where(theirs, ref["r"], torch.zeros_like(ref["r"]))
            r = r / r.sum()
        else:
            r = ref["r"]
        assert float((r - hf).abs().max()) <= sc.HF_TOL, (V, T, k, p, float((r - hf).abs().max()))
    print(f"V = {V}: {n_extra} extra tokens over {len(sc.HF_SETTINGS)} settings")


def test_case_table_covers_what_the_kernel_can_get_wrong():
    assert {c.V for c in CASES} >= {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 32003, sc.REG_MAX - 1, sc.REG_MAX, sc.REG_MAX + 1}
    assert {c.N for c in CASES} == {1, 2, 8}
    assert any(c.ldl_pad % 8 for c in CASES) and any(c.ldl_pad and c.ldl_pad % 8 == 0 for c in CASES) and any(c.ldp_pad for c in CASES)
    for big in (False, True):                                                  # both paths see every setting and every kind of row
        cs = [c for c in CASES if (c.V > sc.REG_MAX) == big]
        assert cs
    cs = CASES
    assert any(c.k == 0 for c in cs) and any(c.k == 1 for c in cs) and any(c.k == c.V - 1 and c.V > 2 for c in cs) and any(c.k >= c.V for c in cs)
    assert any(c.p == 1.0 for c in cs) and any(c.p == 1e-3 for c in cs) and any(c.T == 0.01 for c in cs) and any(c.T == 2.0 for c in cs)
    for kind in sc.KINDS:
        assert sum(kind in c.kinds for c in cs) >= 4, kind
        assert any(kind in c.kinds and c.V >= 32003 for c in cs), kind
    assert any(c.eos for c in cs) and any(not c.eos and c.N >= 2 for c in cs)
    # the rows are what their names say
    c = next(c for c in cs if "neg_inf" in c.kinds and c.V > 64)
    assert bool(torch.isinf(sc.inputs(c)["logits"][c.kinds.index("neg_inf"), :c.V].float()).any())
    c = next(c for c in cs if "big" in c.kinds and c.V > 64)
    assert 5e3 < float(sc.inputs(c)["logits"][c.kinds.index("big"), :c.V].float().abs().max()) <= 1e4
    c = next(c for c in cs if "tie_k" in c.kinds and 2 < c.k < c.V - 1)
    v = torch.sort(sc.inputs(c)["logits"][c.kinds.index("tie_k"), :c.V].float(), descending=True).values
    assert v[c.k - 2] == v[c.k - 1] == v[c.k], "no tie group across the k-th value"
    small = [(c, n) for c in cs if c.p == 1e-3 and c.V > 2 for n in range(c.N)]         # p small enough: only the top group survives
    for c, n in small:
        R = sc.reference(c)[n]
        assert bool((R["l"][R["K2"]] == R["l"][R["K1"]].max()).all()), (c.name, n)
    assert len(small) >= 8
    straddles = 0
    for c in cs:                                                              # top-p boundaries inside a tie group: HF would split these
        if c.p < 1 and "tie_p" in c.kinds and c.V > 64:
            R = sc.reference(c)[c.kinds.index("tie_p")]
            low = R["l"] == R["l"][R["K2"]].min()                              # the lowest kept group, of mass qg in the softmax over K1
            qg = float(R["e"][low].sum() / R["e"][R["K1"]].sum())
            straddles += int(low.sum() > 1 and float(R["m"][low][0]) - qg + qg / int(low.sum()) <= 1.0 - c.p)      # HF drops its first member
    assert straddles >= 1


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bounds_pass_the_emulation_and_no_case_is_loose(case):
    for n, R in enumerate(sc.reference(case)):
        assert torch.equal(R["lo"], R["hi"]), f"{case.name} row {n}: a cumulative mass lies within delta_p = {R['b']['dp']:.2e} of 1 - p (change the seed: SEED_BUMP)"
        assert torch.equal(R["lo"], R["K2"])
        assert R["b"]["dp"] < 1e-5 and R["b"]["du"] < 1e-5
    r = sc.check(case, sc.emulate(case))
    print(f"\n{case.name}: emulation error / bound {r:.3f}")
    assert r <= sc.EMU_MAX, f"{case.name}: the emulation reaches {r:.3f} of the bound"


def test_bounds_reject_every_mutant_on_several_cases():
    caught = {m: [] for m in sc.MUTANTS}
    for case in CASES:
        for name in sc.mutant_names(case):
            x = sc.check(case, sc.emulate(case, name))
            if x >= sc.MUT_MIN:
                caught[name].append(case.name)
    for name, cs in caught.items():
        print(f"{name}: exceeds the bounds on {len(cs)} of {sum(name in sc.mutant_names(c) for c in CASES)} applicable cases")
    for name, cs in caught.items():
        assert len(cs) >= 4, f"mutant {name} exceeds the bounds on only {len(cs)} cases"


def test_distribution_reference_is_usable():
    l, T, k, p, u, ref = sc.distribution_case()
    assert int(ref["K2"].sum()) >= 20 and ref["b"]["du"] < 1e-5 and u.shape == (sc.DIST_M,)
    # the emulation's counts obey the bound the GPU test holds the kernel to
    counts = torch.zeros(sc.DIST_V, dtype=torch.float64)
    for j in range(0, sc.DIST_M, 64):                                          # a 64th of the draws: the CPU loop is slow, the property is per draw
        counts[sc._emulate_row(l, T, k, p, u[j])[0]] += 1
    assert bool(((counts * 64 / sc.DIST_M - ref["r"]).abs() <= 64.0 / sc.DIST_M + ref["b"]["du"]).all())


def test_generate_refuses_sampling_arguments_without_a_device():
    """the argument checks of generate() come before anything touches the model"""
    import inspect
    from llmseg_amd.generate import GenerateMixin
    from llmseg_amd.sam_decoder import SamDecoderMixin
    sig = inspect.signature(GenerateMixin.generate)
    for name, default in (("do_sample", False), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("seed", None), ("uniforms", None), ("return_logprobs", False)):
        assert sig.parameters[name].default == default or (default is None and sig.parameters[name].default is None), name
    ev = inspect.signature(SamDecoderMixin.evaluate)
    for name in ("do_sample", "temperature", "top_k", "top_p", "seed", "uniforms"):
        assert name in ev.parameters, name
    ids = torch.zeros((1, 4), dtype=torch.int64)
    for kw in (dict(temperature=0.5), dict(top_k=5), dict(top_p=0.9), dict(seed=1), dict(uniforms=torch.zeros(1, 3)), dict(return_logprobs=True),
               dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=float("nan")), dict(do_sample=True, top_k=-1), dict(do_sample=True, top_k=1.5),
               dict(do_sample=True, top_p=0.0), dict(do_sample=True, top_p=1.5), dict(do_sample=True, seed=1, uniforms=torch.zeros(1, 3)),
               dict(do_sample=True, uniforms=torch.zeros(1, 4)), dict(do_sample=True, uniforms=torch.zeros(1, 3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            GenerateMixin.generate(None, None, ids, max_new_tokens=3, **kw)
