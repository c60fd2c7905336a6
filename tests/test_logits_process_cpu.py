"""CPU: logits processors.  The rule of tests/logits_process_checks.py against the four installed Hugging Face processors on bf16 inputs, bit for bit (the n-gram
pin of the issue included); the case table of llmseg_logits_process covers what it claims; the header, the binding and INTEGRATION.md agree on the symbol and bad
arguments are refused before any launch; generate() / evaluate() carry the new defaults and refuse bad arguments before any device work."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

from tests import logits_process_checks as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
INF = float("inf")
CASES = lc.cases()
SYM = "llmseg_logits_process"
ARGS = ["logits", "ldl", "N", "V", "hist", "ld_hist", "hist_len", "append", "repetition_penalty", "no_repeat_ngram", "ban_token", "suppress", "n_suppress", "stream"]


def _bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------------------- the rule against transformers
def _random_rows(seed, N, V, n):
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(N, V, generator=g)).to(BF)
    hist = torch.randint(0, min(V, 7), (N, n), generator=g)                 # a small alphabet: duplicates and repeated n-grams everywhere
    for r in range(N):                                                     # every class of value among the touched logits
        for k in range(min(V, 7)):
            logits[r, k] = lc.SPECIAL[(k + r) % 6] if k < 6 else 0.3
    return logits, hist


@pytest.mark.parametrize("theta", (0.7, 1.05, 1.3, 3.0, 1.0000001))
def test_penalty_is_the_installed_processor_bit_for_bit(theta):
    tf = pytest.importorskip("transformers")
    for seed, (N, V, n) in enumerate(((2, 50, 9), (3, 257, 40), (1, 4099, 300))):
        logits, hist = _random_rows(seed, N, V, n)
        hf = tf.RepetitionPenaltyLogitsProcessor(penalty=theta)(hist, logits.clone())
        ours = lc.rule_rows(logits, hist.tolist(), theta=theta)
        assert hf.dtype == BF and torch.equal(_bits(hf), _bits(ours)), (theta, N, V, n)
        assert theta == 1.0000001 or not torch.equal(_bits(ours), _bits(logits))      # (one fp32 ulp above 1 rounds back to the same bf16)


def test_ngram_pin_of_the_issue():
    tf = pytest.importorskip("transformers")
    V = 12
    for h, g, banned in lc.NGRAM_PIN:
        assert {t for t in lc.banned_by_ngram(h, g) if 0 <= t < V} == banned, (h, g)
        hf = tf.NoRepeatNGramLogitsProcessor(g)(torch.tensor([h]), torch.zeros((1, V), dtype=BF))
        assert set(torch.isinf(hf[0].float()).nonzero().flatten().tolist()) == banned, (h, g)


@pytest.mark.parametrize("g", (1, 2, 3, 4))
def test_ngram_ban_is_the_installed_processor(g):
    tf = pytest.importorskip("transformers")
    for seed, (N, V, n) in enumerate(((2, 50, 3), (3, 257, 40), (2, 4099, 300))):
        logits, hist = _random_rows(10 + seed, N, V, n)
        hf = tf.NoRepeatNGramLogitsProcessor(g)(hist, logits.clone())
        ours = lc.rule_rows(logits, hist.tolist(), g=g)
        assert torch.equal(_bits(hf), _bits(ours)), (g, N, V, n)


def test_min_length_suppress_and_the_whole_chain_are_the_installed_processors():
    tf = pytest.importorskip("transformers")
    logits, hist = _random_rows(20, 3, 257, 40)
    eos, prompt = 5, 30                                                    # 10 tokens emitted so far
    for m, ban in ((10, None), (11, eos), (40, eos)):
        hf = tf.MinNewTokensLengthLogitsProcessor(prompt, m, eos)(hist, logits.clone())
        assert torch.equal(_bits(hf), _bits(lc.rule_rows(logits, hist.tolist(), ban=ban))), m
    sup = [3, 200, 3, 256]
    hf = tf.SuppressTokensLogitsProcessor(sup)(hist, logits.clone())
    assert torch.equal(_bits(hf), _bits(lc.rule_rows(logits, hist.tolist(), suppress=sup)))
    chain = tf.LogitsProcessorList([tf.RepetitionPenaltyLogitsProcessor(penalty=1.3), tf.NoRepeatNGramLogitsProcessor(2),
                                    tf.MinNewTokensLengthLogitsProcessor(prompt, 11, eos), tf.SuppressTokensLogitsProcessor(sup)])
    hf = chain(hist, logits.clone())
    ours = lc.rule_rows(logits, hist.tolist(), theta=1.3, g=2, ban=eos, suppress=sup)
    assert torch.equal(_bits(hf), _bits(ours))


def test_rule_edge_values_and_out_of_range_history():
    l = torch.tensor([2.5, -1.75, 0.0, -0.0, INF, -INF, 1.0, 1.0], dtype=BF)
    out, touched = lc.rule(l, [0, 1, 2, 3, 4, 5, 5, 0, lc.IMAGE, 11], theta=2.0)
    assert _bits(out).tolist() == _bits(torch.tensor([1.25, -3.5, 0.0, -0.0, INF, -INF, 1.0, 1.0], dtype=BF)).tolist() and touched == {0, 1, 2, 3, 4, 5}
    # out-of-range values are skipped as targets, and still compare as values inside a window
    out, _ = lc.rule(l, [6, lc.IMAGE, 7, 3, 6, lc.IMAGE], g=3)
    assert torch.isinf(out.float()).nonzero().flatten().tolist() == [4, 5, 7]
    out, _ = lc.rule(l, [6, lc.IMAGE, 6], g=2)
    assert torch.equal(_bits(out), _bits(l))                               # the banned id is -200: nothing to write
    assert lc.banned_by_ngram([1, 2], 3) == set() and lc.banned_by_ngram([], 1) == set() and lc.banned_by_ngram([1, 2], 0) == set()


# ------------------------------------------------------------------------------------------------------------------------------ the table
def test_case_table_covers_what_it_claims():
    assert {c.V for c in CASES} == {33, 4099, 32003} and {c.N for c in CASES} == {1, 3, 8} and all(c.ldl_pad > 0 for c in CASES)
    assert {c.theta for c in CASES} == {0.5, 1.0, 1.2, 3.0} and {c.g for c in CASES} == {0, 1, 2, 3, 4}
    assert {c.append for c in CASES} == {True, False} and {c.ban_mode % 2 for c in CASES} == {0, 1} and {c.sup_mode for c in CASES} == {0, 1, 2}
    for c in CASES:
        if c.theta == 1.0:
            assert c.g > 0 or c.ban_mode % 2 == 0 or c.sup_mode > 0, f"{c.name}: theta = 1 with nothing else on"
    assert {c.g for c in CASES if c.kind in ("period", "same", "oob")} >= {1, 2, 3, 4}
    lens = set()
    for c in CASES:
        inp, ref = lc.inputs(c), lc.reference(c)
        assert len(set(inp["lens"])) == c.N, f"{c.name}: two rows of one length"
        lens |= {("cap" if n == c.cap else "g-1" if c.g and n == c.g - 1 else "g" if c.g and n == c.g else n) for n in inp["lens"]}
        if c.append:                                                       # a full row drops the append
            for r in range(c.N):
                assert ref["lens"][r] == min(inp["lens"][r] + 1, c.cap)
        assert int(inp["logits"][:c.N, :c.V].view(torch.int16).ne(ref["logits"][:c.N, :c.V].view(torch.int16)).sum()) > 0 or max(ref["lens"]) == 0, c.name
    assert lens >= {0, 1, "g-1", "g", 255, 256, 257, 1025, "cap"}, lens
    assert any(c.append and lc.inputs(c)["lens"][r] == c.cap for c in CASES for r in range(c.N)), "no full row meets an append"
    # the chunked-store hazard: one token at positions 0 and cap - 1 of a full history, penalised, not banned
    hazard = 0
    for c in (c for c in CASES if c.kind == "ends" and c.g != 1):
        inp, ref = lc.inputs(c), lc.reference(c)
        x, h = inp["alpha"][0], ref["hists"][0]
        assert c.cap == lc.CAP and len(h) == lc.CAP and h[0] == h[-1] == x and h.count(x) == 2 and c.theta != 1.0
        once = lc.penalise(inp["logits"][0, x:x + 1], c.theta)
        if ref["logits"][0, x] == once[0] and lc.penalise(once, c.theta)[0] != once[0]:
            hazard += 1
    assert hazard >= 2
    # -200 and an id >= V inside the history, inside a matching window, and as the banned id
    seen = set()
    for c in (c for c in CASES if c.kind in ("mix", "oob") and c.g >= 2):
        for h in lc.reference(c)["hists"]:
            n, g = len(h), c.g
            if n < g:
                continue
            for j in range(n - g + 1):
                if h[j:j + g - 1] == h[n - g + 1:]:
                    seen |= {("window", t) for t in h[j:j + g - 1] if not 0 <= t < c.V} | ({("banned", h[j + g - 1])} if not 0 <= h[j + g - 1] < c.V else set())
    assert {k for k, _ in seen} == {"window", "banned"} and {t < 0 for _, t in seen} == {True, False}


# -------------------------------------------------------------------------------------------------------------------- header, binding, library
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmseg_hip.h")).read(), flags=re.S)


def test_symbol_is_declared_bound_and_exported_with_the_headers_argument_order():
    from llmseg_amd import _lib, ops
    src = _header()
    assert re.search(r"\bint\s+%s\s*\(" % SYM, src), f"{SYM} is not declared in include/llmseg_hip.h"
    assert SYM in _lib.SIGNATURES, f"{SYM} is not bound in llmseg_amd/_lib.py"
    decl = re.search(r"%s\s*\((.*?)\)\s*;" % SYM, src, flags=re.S).group(1).split(",")
    assert [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", a)[-1] for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_float if "float" in a else C.c_int32 if "int32_t" in a else C.c_int64 for a in decl]
    assert _lib.SIGNATURES[SYM] == kinds
    assert int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION >= 20
    assert int(re.search(r"#define LLMSEG_LOGITS_HIST_CAP (\d+)", src).group(1)) == ops.LOGITS_HIST_CAP == lc.CAP
    lib = _lib.load()
    assert hasattr(lib, SYM) and lib.llmseg_version() == _lib.ABI_VERSION
    assert lib.llmseg_struct_size(6) == -1                                 # a plain argument list: no new argument struct
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"llmseg_version\(\) == %d\b" % _lib.ABI_VERSION, doc) and SYM in doc
    assert "logits.hip" in open(os.path.join(ROOT, "llmseg_amd", "csrc", "build.sh")).read()


def test_logits_process_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    ok = dict(logits=4096, ldl=40, N=2, V=33, hist=4096, ld_hist=64, hist_len=4096, append=4096, theta=1.2, g=2, ban=3, suppress=4096, n_suppress=2)
    bads = [dict(logits=None), dict(hist=None), dict(hist_len=None), dict(logits=4097), dict(hist=4100), dict(hist_len=4098), dict(append=4100), dict(suppress=4098),
            dict(N=0), dict(N=-1), dict(V=0), dict(V=1 << 31, ldl=1 << 32), dict(ldl=32), dict(ld_hist=0), dict(ld_hist=lc.CAP + 1), dict(theta=0.0), dict(theta=-1.0),
            dict(theta=INF), dict(theta=float("nan")), dict(g=-1), dict(ban=-2), dict(ban=33), dict(n_suppress=-1), dict(n_suppress=0), dict(suppress=None),
            dict(suppress=None, n_suppress=-1)]
    n0 = lib.llmseg_launch_count()
    for bad in bads:
        a = dict(ok, **bad)
        rc = lib.llmseg_logits_process(p(a["logits"]), a["ldl"], a["N"], a["V"], p(a["hist"]), a["ld_hist"], p(a["hist_len"]), p(a["append"]), a["theta"], a["g"], a["ban"],
                                       p(a["suppress"]), a["n_suppress"], None)
        assert rc == -1 and b"logits_process" in lib.llmseg_last_error(), bad
    assert lib.llmseg_launch_count() == n0


# -------------------------------------------------------------------------------------------------------------------- generate(), evaluate()
def test_generate_and_evaluate_signatures_carry_the_defaults():
    from llmseg_amd.generate import GenerateMixin
    from llmseg_amd.sam_decoder import SamDecoderMixin
    names = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")
    for fn in (GenerateMixin.generate, SamDecoderMixin.evaluate):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in names] == [1.0, 0, 0, None]
    ops_sig = inspect.signature(__import__("llmseg_amd.ops", fromlist=["ops"]).logits_process).parameters
    assert list(ops_sig) == ["logits", "hist", "hist_len", "append", "repetition_penalty", "no_repeat_ngram_size", "ban_token", "suppress"]
    assert [ops_sig[k].default for k in list(ops_sig)[3:]] == [None, 1.0, 0, None, None]


def test_generate_refuses_bad_controls_before_touching_a_device():
    """the checks come before prepare(): a stand-in for `self` that has a config and nothing else is enough"""
    from llmseg_amd.generate import GenerateMixin
    stub = types.SimpleNamespace(config=types.SimpleNamespace(llama=types.SimpleNamespace(vocab=100, head_dim=128)), _ragged_prompts=GenerateMixin._ragged_prompts)
    ids = torch.zeros((2, 6), dtype=torch.int64)
    ids[:, 1] = -200
    gen = lambda **kw: GenerateMixin.generate(stub, None, ids, **dict(dict(max_new_tokens=4), **kw))
    for bad in (0.0, -1.0, INF, float("nan"), "1.2", None, True):
        with pytest.raises(ValueError, match="repetition_penalty"):
            gen(repetition_penalty=bad, no_repeat_ngram_size=2)
    for name in ("no_repeat_ngram_size", "min_new_tokens"):
        for bad in (-1, 1.5, "2", None, True):
            with pytest.raises(ValueError, match=name):
                gen(**{name: bad, "repetition_penalty": 1.2})
    with pytest.raises(ValueError, match="min_new_tokens"):
        gen(min_new_tokens=2, eos_token_id=None)
    with pytest.raises(ValueError, match="min_new_tokens"):
        gen(min_new_tokens=5)
    for bad in ([], (), [100], [-1], [3, 1.5], [True], "ab", 7):
        with pytest.raises(ValueError, match="suppress_tokens"):
            gen(suppress_tokens=bad)
    with pytest.raises(ValueError, match="cap"):
        gen(repetition_penalty=1.2, max_new_tokens=lc.CAP - 5)
    with pytest.raises(ValueError, match="cap"):                           # the trimmed length Lm counts, not the padded one
        GenerateMixin.generate(stub, None, torch.cat([ids, torch.zeros((2, 8), dtype=torch.int64)], 1), max_new_tokens=lc.CAP - 8, no_repeat_ngram_size=2,
                               attention_mask=torch.arange(14)[None, :] < torch.tensor([9, 7])[:, None])
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1), dict(suppress_tokens=[3])):
        with pytest.raises(ValueError, match="num_beams"):
            gen(num_beams=2, **kw)
