"""GPU: logits processors.  llmseg_logits_process on every case of tests/logits_process_checks.py against the CPU rule, bit for bit (the processed rows, the
history and its lengths, bit-equal repeats, nothing written outside the affected logits, one launch); generate(repetition_penalty=, no_repeat_ngram_size=,
min_new_tokens=, suppress_tokens=) end to end on the tiny model: every step of a recorded run equals the rule on its own inputs and the pick reads the processed
logits, the properties each control promises, graph == eager, the quantised routes, evaluate() forwards the keywords, and a default call never reaches the kernel."""
import functools

import pytest
import torch

from tests import logits_process_checks as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
CASES = lc.cases()
GUARD_LEN = -9


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield


def _fault_guard(name, e):
    if "HIP error" in str(e) or "illegal memory access" in str(e):          # a device fault: nothing more may be started on this GPU
        pytest.exit(f"{name}: {e}", returncode=3)


def _guarded(name, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        _fault_guard(name, e)
        raise


def _bits(t):
    return t.view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------- the kernel
def _call(case, suppress_as_tensor):
    """one launch on fresh copies: logits with a decoy row and pad columns, the history between two guard rows -> (logits, hist, hist_len on the CPU, launches)"""
    from llmseg_amd import _lib, ops
    inp = lc.inputs(case)
    N, V = case.N, case.V
    logits = inp["logits"].to(DEV)
    hist = torch.full((N + 2, case.cap), lc.SENTINEL, dtype=torch.int64)
    hist[1:N + 1] = lc.hist_tensor(inp["hists"], case.cap)
    hist = hist.to(DEV)
    hist_len = torch.tensor([GUARD_LEN] + inp["lens"] + [GUARD_LEN], dtype=torch.int32, device=DEV)
    append = None if inp["append"] is None else torch.tensor(inp["append"], dtype=torch.int64, device=DEV)
    sup = inp["suppress"]
    if sup is not None and suppress_as_tensor:
        sup = torch.tensor(sup, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    n0 = _lib.load().llmseg_launch_count()
    ret = ops.logits_process(logits[:N, :V], hist[1:N + 1], hist_len[1:N + 1], append=append, repetition_penalty=inp["theta"], no_repeat_ngram_size=inp["g"],
                             ban_token=inp["ban"], suppress=sup)
    launches = _lib.load().llmseg_launch_count() - n0
    assert ret.data_ptr() == logits.data_ptr()
    torch.cuda.synchronize()
    return logits.cpu(), hist.cpu(), hist_len.cpu(), launches


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_equals_the_rule_bit_for_bit(case):
    inp, ref = lc.inputs(case), lc.reference(case)
    N, V = case.N, case.V
    la, ha, na, launches = _guarded(case.name, lambda: _call(case, False))
    lb, hb, nb, _ = _guarded(case.name, lambda: _call(case, True))
    assert launches == 1, f"{case.name}: {launches} launches"
    assert torch.equal(_bits(la[:N, :V]), _bits(ref["logits"][:N, :V])), f"{case.name}: rows {(_bits(la[:N, :V]) != _bits(ref['logits'][:N, :V])).any(1).nonzero().flatten().tolist()} differ from the rule"
    # every logit outside the affected set keeps its bits: the rest of each row, the pad columns, the decoy row
    keep = torch.ones(la.shape, dtype=torch.bool)
    for r in range(N):
        if ref["touched"][r]:
            keep[r, torch.tensor(sorted(ref["touched"][r]))] = False
    assert torch.equal(_bits(la)[keep], _bits(inp["logits"])[keep]), f"{case.name}: a store outside the affected logits"
    # the history: the appended token where the row had room, every other cell (the guard rows too) as it was
    want = torch.full((N + 2, case.cap), lc.SENTINEL, dtype=torch.int64)
    want[1:N + 1] = lc.hist_tensor(ref["hists"], case.cap)
    assert torch.equal(ha, want), f"{case.name}: history"
    assert na.tolist() == [GUARD_LEN] + ref["lens"] + [GUARD_LEN], f"{case.name}: hist_len {na.tolist()}"
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(ha, hb) and torch.equal(na, nb), f"{case.name}: a second call differs"


def test_single_row_with_a_row_stride_and_bad_arguments():
    from llmseg_amd import ops
    V = 97
    logits = torch.arange(3 * 128, dtype=F32).view(3, 128).to(DEV, BF)
    want = logits.cpu().clone()
    hist = torch.tensor([[5, 6, 5, 0, 0, 0]], dtype=torch.int64, device=DEV)
    hist_len = torch.tensor([3], dtype=torch.int32, device=DEV)
    _guarded("one row", lambda: ops.logits_process(logits[1:2, :V], hist, hist_len, repetition_penalty=2.0, ban_token=96, suppress=[0]))
    want[1, :V] = lc.rule(want[1, :V], [5, 6, 5], theta=2.0, ban=96, suppress=[0])[0]
    assert torch.equal(_bits(logits.cpu()), _bits(want)) and hist_len.tolist() == [3]
    for bad in (dict(repetition_penalty=0.0), dict(no_repeat_ngram_size=-1), dict(ban_token=V)):
        with pytest.raises(RuntimeError, match="logits_process"):
            ops.logits_process(logits[1:2, :V], hist, hist_len, **bad)
    with pytest.raises(AssertionError):
        ops.logits_process(logits[1:2, :V], hist, hist_len, suppress=[V])


# ---------------------------------------------------------------------------------------------------------------------------- generation
MAX_NEW = 8
LENS = (24, 17)
CONTROLS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
SAMPLING = dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.9)


def _model(sd, cfg, sam_decoder=False):
    from llmseg_amd import lisa as hip_lisa
    from tests import model_checks as mc
    hcfg = mc.to_hip_cfg(cfg)
    if sam_decoder:
        hcfg.sam_decoder = True
    m = hip_lisa.LISAForCausalLM(hcfg, device=DEV)
    missing, _ = m.load_state_dict(sd, strict=False)
    assert not missing, missing[:5]
    return m


@functools.lru_cache(maxsize=None)
def _tiny(lora_r=8):
    from oracle import cases
    from tests import model_checks as mc, w8_checks as wc
    cfg = cases.tiny_lisa_cfg(lora_r=lora_r)
    sd, _, _ = wc.generation_states(cfg)
    batch = mc._round_batch(cases.tiny_lisa_batch())
    return _model(sd, cfg), batch["images_clip"][:2].to(DEV), batch["input_ids"][:2].to(DEV)


@functools.lru_cache(maxsize=None)
def _free_run():
    """the uncontrolled greedy call every property below is measured against: (sequences, hidden)"""
    m, clip, ids = _tiny()
    return _guarded("free run", lambda: m.generate(clip, ids, max_new_tokens=MAX_NEW, eos_token_id=None))


class _Recorder:
    """wraps ops.logits_process: keeps each call's raw logits, its history before and after, its arguments and its processed logits"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, logits, hist, hist_len, append=None, repetition_penalty=1.0, no_repeat_ngram_size=0, ban_token=None, suppress=None):
        c = dict(raw=logits.clone(), hist=hist.clone(), len=hist_len.clone(), append=None if append is None else append.clone(), theta=repetition_penalty,
                 g=no_repeat_ngram_size, ban=ban_token, suppress=None if suppress is None else suppress.clone())
        out = self.real(logits, hist, hist_len, append=append, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, ban_token=ban_token,
                        suppress=suppress)
        c.update(out=logits.clone(), hist_after=hist.clone(), len_after=hist_len.clone(), ptr=logits.data_ptr())
        self.calls.append(c)
        return out


class _SampleRecorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, logits, *a, **kw):
        self.calls.append(dict(logits=logits.clone(), ptr=logits.data_ptr()))
        return self.real(logits, *a, **kw)


@pytest.mark.parametrize("sampled", (False, True), ids=("greedy", "sampled"))
@pytest.mark.parametrize("ragged", (False, True), ids=("plain", "attention_mask"))
def test_every_recorded_step_equals_the_rule_and_the_pick_reads_the_processed_logits(monkeypatch, ragged, sampled):
    from llmseg_amd import ops
    from llmseg_amd.generate import pad_prompts
    m, clip, ids = _tiny()
    mask = None
    if ragged:
        ids, mask = (t.to(DEV) for t in pad_prompts([ids[i, :n].clone() for i, n in enumerate(LENS)], 0))
    L = ids.shape[1]
    lens = LENS if ragged else (L, L)
    free = _free_run()[0]
    sup = [int(free[0, -MAX_NEW]), 3, int(free[0, -MAX_NEW])]                # (the first token of the free run, unless the ragged prompt changes it; a duplicate id)
    eos, MIN = int(free[1, -MAX_NEW + 1]), 5
    rec = _Recorder(ops.logits_process)
    monkeypatch.setattr(ops, "logits_process", rec)
    srec = _SampleRecorder(ops.sample_tokens)
    monkeypatch.setattr(ops, "sample_tokens", srec)
    kw = dict(max_new_tokens=MAX_NEW, attention_mask=mask, eos_token_id=eos, pad_token_id=1, min_new_tokens=MIN, suppress_tokens=sup, use_graph=False, **CONTROLS)
    if sampled:
        kw.update(seed=7, **SAMPLING)
    seq, hid = _guarded("recorded run", lambda: m.generate(clip, ids, **kw))
    n_new = seq.shape[1] - L
    assert MIN <= n_new <= MAX_NEW and len(rec.calls) == n_new and (len(srec.calls) == n_new if sampled else not srec.calls)
    prompts = [ids[r, :lens[r]].tolist() for r in range(2)]
    assert all(lc.IMAGE in p for p in prompts)
    unique = 0
    for s, c in enumerate(rec.calls):
        assert (c["append"] is None) == (s == 0) and c["theta"] == 1.3 and c["g"] == 2 and c["ban"] == (eos if s < MIN else None) and c["suppress"].tolist() == sup
        emitted = [seq[r, lens[r]:lens[r] + s].tolist() for r in range(2)]
        hists = [prompts[r] + emitted[r] for r in range(2)]                # every row's history is its own prompt followed by its own tokens
        assert c["len_after"].tolist() == [len(h) for h in hists]
        for r in range(2):
            assert c["hist_after"][r, :len(hists[r])].tolist() == hists[r], f"step {s} row {r}: history"
            if s:
                assert int(c["append"][r]) == emitted[r][-1] and int(c["len"][r]) == len(hists[r]) - 1
        want = lc.rule_rows(c["raw"].cpu(), hists, theta=1.3, g=2, ban=c["ban"], suppress=sup)
        assert torch.equal(_bits(c["out"].cpu()), _bits(want)), f"step {s}: the processed logits differ from the rule"
        assert not torch.equal(_bits(c["out"]), _bits(c["raw"]))
        done = [eos in emitted[r] for r in range(2)]
        if sampled:
            assert srec.calls[s]["ptr"] == c["ptr"] and torch.equal(_bits(srec.calls[s]["logits"]), _bits(c["out"])), f"step {s}: sample_tokens read other logits"
        else:
            # the tiny model's bf16 logits do tie at the top now and then: the token is then the one the same arg-max call names on the recorded rows, and
            # most picks must be decided by a unique maximum
            lg = c["out"].float()
            pick = lg.argmax(-1)
            unique += int(((lg == lg.max(-1, keepdim=True).values).sum(-1) == 1).sum())
            for r in range(2):
                assert int(seq[r, lens[r] + s]) == (1 if done[r] else int(pick[r])), f"step {s} row {r}: the token is not the arg-max of the processed row"
    assert sampled or unique >= n_new, f"only {unique} of {2 * n_new} arg-max picks were unique: the comparison needs another prompt"
    new =[seq[r, lens[r]:lens[r] + n_new].tolist() for r in range(2)]
    for r in range(2):
        assert eos not in new[r][:MIN] and not set(sup) & set(new[r])
    assert hid.shape[0] == 2


def _no_repeated_bigram(prompt, new):
    """no bigram that ends in the generated part occurs earlier in prompt + new"""
    full = prompt + new
    seen = {tuple(full[i:i + 2]) for i in range(len(prompt) - 1)}
    for i in range(len(prompt) - 1, len(full) - 1):
        if tuple(full[i:i + 2]) in seen:
            return False
        seen.add(tuple(full[i:i + 2]))
    return True


def _properties(m, clip, ids, name, **route):
    """the three properties on one route -> the controlled sequences"""
    L = ids.shape[1]
    kw = dict(max_new_tokens=MAX_NEW, **route)
    free, _ = _guarded(name + " free", lambda: m.generate(clip, ids, eos_token_id=None, **kw))
    # no_repeat_ngram_size = 2, on a prompt continuation that the penalty-free model repeats or not: the property must hold either way
    seq, _ = _guarded(name + " ngram", lambda: m.generate(clip, ids, eos_token_id=None, no_repeat_ngram_size=2, **kw))
    for r in range(2):
        assert _no_repeated_bigram(ids[r].tolist(), seq[r, L:].tolist()), f"{name} row {r}: a bigram occurs twice"
    # min_new_tokens: the eos is the free run's second token of row 0, so the uncontrolled call stops row 0 where that token first occurs (k = 1, or 0)
    eos, MIN = int(free[0, L + 1]), 5
    k = 0 if int(free[0, L]) == eos else 1
    short, _ = _guarded(name + " eos", lambda: m.generate(clip, ids, eos_token_id=eos, pad_token_id=1, **kw))
    assert int(short[0, L + k]) == eos and short[0, L:L + k].tolist() == free[0, L:L + k].tolist()
    held, _ = _guarded(name + " min", lambda: m.generate(clip, ids, eos_token_id=eos, pad_token_id=1, min_new_tokens=MIN, **kw))
    assert held.shape[1] >= L + MIN and not bool((held[:, L:L + MIN] == eos).any()), f"{name}: an eos before token {MIN}"
    assert held[0, L:L + k].tolist() == free[0, L:L + k].tolist() and int(held[0, L + k]) != eos, f"{name}: the first {MIN} tokens must differ where the uncontrolled call put the eos"
    # a suppressed token that the free run emits never appears
    sup = sorted({int(free[0, L]), int(free[1, L + 2])})
    quiet, _ = _guarded(name + " suppress", lambda: m.generate(clip, ids, eos_token_id=None, suppress_tokens=sup, **kw))
    assert not bool(torch.isin(quiet[:, L:], torch.tensor(sup, device=DEV)).any()), f"{name}: a suppressed token was emitted"
    return seq


def test_properties_on_the_default_route_and_graph_equals_eager():
    m, clip, ids = _tiny()
    _properties(m, clip, ids, "graph")
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None, suppress_tokens=[5, 9], **CONTROLS)
    a = _guarded("graph", lambda: m.generate(clip, ids, **kw))
    b = _guarded("graph again", lambda: m.generate(clip, ids, **kw))
    e = _guarded("eager", lambda: m.generate(clip, ids, use_graph=False, **kw))
    u = _guarded("unfused", lambda: m.generate(clip, ids, fuse_decode=False, **kw))
    for x, name in ((b, "a second call"), (e, "eager steps")):
        assert torch.equal(a[0], x[0]) and torch.equal(_bits(a[1]), _bits(x[1])), f"{name} differ"
    assert u[0].shape == a[0].shape and not bool(torch.isin(a[0][:, ids.shape[1]:], torch.tensor([5, 9], device=DEV)).any())


@pytest.mark.parametrize("route", (dict(weight_bits=8), dict(weight_format="mxfp4")), ids=("int8", "mxfp4"))
def test_properties_on_the_quantised_routes(route):
    m, clip, ids = _tiny()
    _properties(m, clip, ids, str(route), **route)


def test_controls_that_cannot_act_leave_the_default_call_bit_for_bit(monkeypatch):
    from llmseg_amd import ops
    m, clip, ids = _tiny()
    free = _free_run()
    rec = _Recorder(ops.logits_process)
    monkeypatch.setattr(ops, "logits_process", rec)
    big = ids.shape[1] + MAX_NEW + 1                                       # larger than any history of the call
    seq, hid = _guarded("g too large", lambda: m.generate(clip, ids, max_new_tokens=MAX_NEW, eos_token_id=None, repetition_penalty=1.0, no_repeat_ngram_size=big))
    assert len(rec.calls) == MAX_NEW and all(torch.equal(_bits(c["raw"]), _bits(c["out"])) for c in rec.calls)
    assert torch.equal(seq, free[0]) and torch.equal(_bits(hid), _bits(free[1]))


def test_a_default_call_never_reaches_the_kernel(monkeypatch):
    from llmseg_amd import ops
    m, clip, ids = _tiny()
    free = _free_run()

    def boom(*a, **kw):
        raise AssertionError("ops.logits_process called by a default generate()")
    monkeypatch.setattr(ops, "logits_process", boom)
    seq, hid = _guarded("default", lambda: m.generate(clip, ids, max_new_tokens=MAX_NEW, eos_token_id=None))
    assert torch.equal(seq, free[0]) and torch.equal(_bits(hid), _bits(free[1]))
    seq_s, _ = _guarded("default sampled", lambda: m.generate(clip, ids, max_new_tokens=3, eos_token_id=None, seed=1, **SAMPLING))
    assert seq_s.shape == (2, ids.shape[1] + 3)
    with pytest.raises(AssertionError, match="logits_process called"):
        m.generate(clip, ids, max_new_tokens=3, eos_token_id=None, no_repeat_ngram_size=2)


def test_evaluate_forwards_the_controls():
    from oracle import cases
    from tests import model_checks as mc, w8_checks as wc
    cfg = cases.tiny_lisa_cfg("sam")
    sd, _, _ = wc.generation_states(cfg)
    sd.update({k: v.to(BF).float() for k, v in cases.sam_decoder_state().items()})
    m = _model(sd, cfg, sam_decoder=True)
    batch = mc._round_batch(cases.tiny_lisa_batch(img_size=cfg.sam.img))
    clip, images, ids = batch["images_clip"][:2].to(DEV), batch["images"][:2].to(DEV), batch["input_ids"][:2].to(DEV)
    resize, orig = [(683, 1024), (1024, 768)], [(427, 640), (96, 72)]
    free, _ = _guarded("free", lambda: m.generate(clip, ids, max_new_tokens=4, eos_token_id=None))
    L = ids.shape[1]
    kw = dict(max_new_tokens=4, eos_token_id=int(free[0, L + 1]), min_new_tokens=3, suppress_tokens=[int(free[1, L])], **CONTROLS)
    seq, _ = _guarded("generate", lambda: m.generate(clip, ids, **kw))
    out, masks = _guarded("evaluate", lambda: m.evaluate(clip, images, ids, resize, orig, **kw))
    assert torch.equal(out, seq) and len(masks) == 2 and not torch.equal(seq[:, :free.shape[1]], free[:, :seq.shape[1]])
