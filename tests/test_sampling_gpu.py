"""GPU: sampling.  llmseg_sample_tokens on every case of tests/sampling_checks.py against the fp64 rule under the bounds tests/test_sampling_cpu.py validates (kept
sets, whole tie groups, probs, the token's CDF position, logprob, eos / pad bookkeeping, bit-equal repeats, nothing written outside the outputs); the distribution
of 4096 stratified draws; generate(do_sample=True) end to end on the tiny model: top_k=1 is the greedy call, seeds reproduce, graph == eager, every step of a
recorded run obeys the kernel assertions on its own logits, evaluate() forwards the keywords, bad arguments raise."""
import collections
import functools

import pytest
import torch

from tests import sampling_checks as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
CASES = sc.cases()
NAN = float("nan")
_WORST = collections.defaultdict(lambda: (0.0, ""))


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield
    print("\nworst error / bound")
    for k in sorted(_WORST):
        print(f"  {k:12s} {_WORST[k][0]:.3f}  at {_WORST[k][1]}")


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


def _call(logits, u, T, k, p, eos, pad, unfinished, ldp_pad=0):
    """one launch with every optional output, into buffers with a guard row and guard columns -> (out dict on the CPU, the guards are intact)"""
    from llmseg_amd import ops
    N, V = logits.shape
    nb = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    lb = torch.full((N + 1,), NAN, dtype=F32, device=DEV)
    kb = torch.full((N + 1,), -7, dtype=torch.int32, device=DEV)
    pb = torch.full((N + 1, V + ldp_pad), NAN, dtype=F32, device=DEV)
    uf = unfinished.to(DEV).clone()
    ops.sample_tokens(logits, T, k, p, u, eos_token_id=eos, pad_token_id=pad, unfinished=uf, next=nb[:N], logprob=lb[:N], kept=kb[:N], probs=pb[:N, :V])
    intact = bool(nb[N] == -7) and bool(torch.isnan(lb[N])) and bool(kb[N] == -7) and bool(torch.isnan(pb[N]).all()) and bool(torch.isnan(pb[:, V:]).all())
    return dict(next=nb[:N].cpu(), logprob=lb[:N].cpu(), kept=kb[:N].cpu(), probs=pb[:N, :V].cpu(), unfinished=uf.cpu()), intact


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_obeys_the_rule_within_its_bounds(case):
    inp = sc.inputs(case)
    N, V = case.N, case.V
    logits = inp["logits"].to(DEV)[:N, :V]                                  # rows of stride V + ldl_pad; row N and the pad columns are decoys
    u = inp["u"].to(DEV)[:N]
    a, intact_a = _guarded(case.name, lambda: _call(logits, u, case.T, case.k, case.p, inp["eos"], inp["pad"], inp["unfinished"], case.ldp_pad))
    b, intact_b = _guarded(case.name, lambda: _call(logits, u, case.T, case.k, case.p, inp["eos"], inp["pad"], inp["unfinished"], case.ldp_pad))
    assert intact_a and intact_b, f"{case.name}: a store outside the outputs"
    for key in a:
        assert torch.equal(a[key].view(torch.int32) if a[key].dtype == F32 else a[key], b[key].view(torch.int32) if b[key].dtype == F32 else b[key]), \
            f"{case.name}: {key} differs between two calls"
    r = sc.check(case, a)
    print(f"\n{case.name}: error / bound {r:.3f}")
    path = "general" if V > sc.REG_MAX else "registers"
    _WORST[path] = max(_WORST[path], (r, case.name))
    assert r <= 1.0, f"{case.name}: error / bound = {r:.3f}"


def test_optional_outputs_are_optional_and_do_not_change_the_token():
    from llmseg_amd import ops
    case = next(c for c in CASES if c.V == 4099 and c.N == 8)
    inp = sc.inputs(case)
    logits, u = inp["logits"].to(DEV)[:case.N, :case.V], inp["u"].to(DEV)[:case.N]
    full, _ = _guarded(case.name, lambda: _call(logits, u, case.T, case.k, case.p, None, 0, inp["unfinished"]))
    nxt, lp, kept, probs = _guarded(case.name, lambda: ops.sample_tokens(logits, case.T, case.k, case.p, u))
    assert lp is None and kept is None and probs is None and torch.equal(nxt.cpu(), full["next"])
    nxt, lp, kept, probs = _guarded(case.name, lambda: ops.sample_tokens(logits, case.T, case.k, case.p, u, want_logprob=True, want_kept=True, want_probs=True))
    assert torch.equal(nxt.cpu(), full["next"]) and torch.equal(lp.cpu(), full["logprob"]) and torch.equal(kept.cpu(), full["kept"]) and torch.equal(probs.cpu(), full["probs"])
    with pytest.raises(RuntimeError):
        ops.sample_tokens(logits, 0.0, 0, 1.0, u)
    with pytest.raises(RuntimeError):
        ops.sample_tokens(logits, 1.0, 0, 1.5, u)


def test_distribution_of_stratified_draws():
    """one row replicated over M rows with u = (j + 1/2) / M: every token's share of the draws is within 1 / M + delta_u of r_i"""
    from llmseg_amd import ops
    l, T, k, p, u, ref = sc.distribution_case()
    logits = l.to(DEV)[None, :].repeat(sc.DIST_M, 1)
    nxt, _, _, _ = _guarded("distribution", lambda: ops.sample_tokens(logits, T, k, p, u.to(DEV)))
    nxt = nxt.cpu()
    assert bool((nxt[1:] >= nxt[:-1]).all()), "ascending u must give ascending token ids"
    share = torch.bincount(nxt, minlength=sc.DIST_V).double() / sc.DIST_M
    err = (share - ref["r"]).abs().max().item()
    print(f"\ndistribution: worst |count / M - r| = {err:.3e} (bound {1.0 / sc.DIST_M + ref['b']['du']:.3e})")
    assert err <= 1.0 / sc.DIST_M + ref["b"]["du"]


# ---------------------------------------------------------------------------------------------------------------------------- generation
MAX_NEW = 6
SAMPLING = dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.9)
LENS = (24, 17)


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


class _Recorder:
    """wraps ops.sample_tokens: runs the real kernel with every optional output and keeps each call's inputs and outputs"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, logits, temperature, top_k, top_p, u, eos_token_id=None, pad_token_id=0, unfinished=None, want_logprob=False, **kw):
        assert not kw, kw
        before = unfinished.clone()
        nxt, lp, kept, probs = self.real(logits, temperature, top_k, top_p, u, eos_token_id=eos_token_id, pad_token_id=pad_token_id, unfinished=unfinished,
                                         want_logprob=True, want_kept=True, want_probs=True)
        self.calls.append(dict(logits=logits.clone(), args=(temperature, top_k, top_p), u=u.clone(), eos=eos_token_id, pad=pad_token_id, before=before,
                               out=dict(next=nxt.clone(), logprob=lp.clone(), kept=kept.clone(), probs=probs.clone(), unfinished=unfinished.clone())))
        return nxt, (lp if want_logprob else None), None, None


def test_top_k_1_is_the_greedy_call(monkeypatch):
    from llmseg_amd import ops
    m, clip, ids = _tiny()
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None)
    seq_g, hid_g = _guarded("greedy", lambda: m.generate(clip, ids, **kw))
    rec = _Recorder(ops.sample_tokens)
    monkeypatch.setattr(ops, "sample_tokens", rec)
    seq_s, hid_s = _guarded("top_k=1", lambda: m.generate(clip, ids, do_sample=True, top_k=1, seed=3, **kw))
    assert len(rec.calls) == MAX_NEW
    for c in rec.calls:                                                    # precondition: the arg-max is unique at every step, so K2 is one token
        lg = c["logits"].float()
        assert bool(((lg == lg.max(-1, keepdim=True).values).sum(-1) == 1).all()), "a tied arg-max: top_k=1 keeps both, the comparison needs another prompt"
        assert bool((c["out"]["kept"] == 1).all())
    assert torch.equal(seq_s, seq_g) and torch.equal(hid_s.view(torch.int16), hid_g.view(torch.int16))


def test_seed_reproduces_graph_equals_eager_and_seeds_differ():
    m, clip, ids = _tiny()
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None, return_logprobs=True, **SAMPLING)
    a = _guarded("seed 11", lambda: m.generate(clip, ids, seed=11, **kw))
    b = _guarded("seed 11 again", lambda: m.generate(clip, ids, seed=11, **kw))
    e = _guarded("seed 11 eager", lambda: m.generate(clip, ids, seed=11, use_graph=False, **kw))
    u = _guarded("seed 11 unfused", lambda: m.generate(clip, ids, seed=11, fuse_decode=False, **kw))
    w = _guarded("seed 11 int8", lambda: m.generate(clip, ids, seed=11, weight_bits=8, **kw))
    c = _guarded("seed 12", lambda: m.generate(clip, ids, seed=12, **kw))
    assert len(a) == 3 and a[2].shape == (2, MAX_NEW) and a[2].dtype == F32 and a[0].shape == (2, ids.shape[1] + MAX_NEW)
    for x, name in ((b, "a second call"), (e, "eager steps")):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1].view(torch.int16), x[1].view(torch.int16)) and torch.equal(a[2], x[2]), f"{name} differ"
    assert u[0].shape == a[0].shape and w[0].shape == a[0].shape and bool((a[2] <= 0).all())
    assert not torch.equal(a[0], c[0]), "another seed gave the same sequence"
    # uniforms= is the same stream the seed draws
    us = torch.rand((2, MAX_NEW), device=DEV, dtype=F32, generator=torch.Generator(device=DEV).manual_seed(11))
    kw2 = dict(kw)
    d = _guarded("uniforms", lambda: m.generate(clip, ids, uniforms=us, **kw2))
    assert torch.equal(a[0], d[0]) and torch.equal(a[2], d[2])


@pytest.mark.parametrize("ragged", (False, True), ids=("plain", "attention_mask"))
def test_every_recorded_step_obeys_the_kernel_assertions(monkeypatch, ragged):
    from llmseg_amd import ops
    from llmseg_amd.generate import pad_prompts
    m, clip, ids = _tiny()
    mask = None
    if ragged:
        ids, mask = (t.to(DEV) for t in pad_prompts([ids[i, :n].clone() for i, n in enumerate(LENS)], 0))
    L = ids.shape[1]
    # eos: a first run without an eos rule tells which token row 0 draws at its third step; the run under test then finishes row 0 there
    us = torch.rand((2, MAX_NEW), device=DEV, dtype=F32, generator=torch.Generator(device=DEV).manual_seed(5))
    kw = dict(max_new_tokens=MAX_NEW, use_graph=False, attention_mask=mask, uniforms=us, **SAMPLING)
    free, _ = _guarded("free run", lambda: m.generate(clip, ids, eos_token_id=None, **kw))
    eos = int(free[0, (LENS[0] if ragged else L) + 2])
    rec = _Recorder(ops.sample_tokens)
    monkeypatch.setattr(ops, "sample_tokens", rec)
    PAD = 1
    seq, hid, lps = _guarded("recorded run", lambda: m.generate(clip, ids, eos_token_id=eos, pad_token_id=PAD, return_logprobs=True, **kw))
    n_new = len(rec.calls)
    assert 3 <= n_new <= MAX_NEW and lps.shape == (2, n_new)
    T, k, p = SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"]
    worst = 0.0
    for s, c in enumerate(rec.calls):
        assert c["args"] == (T, k, p) and c["eos"] == eos and c["pad"] == PAD and torch.equal(c["u"], us[:, s])
        rows = sc.reference_rows(c["logits"].cpu(), T, k, p)
        for R in rows:
            assert torch.equal(R["lo"], R["hi"]), "a cumulative mass within delta_p of 1 - p: the step would be loosely checked (use another seed)"
        out = {key: v.cpu() for key, v in c["out"].items()}
        r = sc.check_rows(rows, p, c["u"].cpu(), c["before"].cpu(), eos, PAD, out)
        worst = max(worst, r)
        assert r <= 1.0, f"step {s}: error / bound = {r:.3f}"
        # what generate() returns is exactly what the kernel wrote
        assert torch.equal(lps[:, s], c["out"]["logprob"])
        for n in range(2):
            col = (LENS[n] if ragged else L) + s
            assert int(seq[n, col]) == int(c["out"]["next"][n])
    print(f"\nrecorded steps ({'ragged' if ragged else 'plain'}): worst error / bound {worst:.3f} over {n_new} steps")
    _WORST["generate"] = max(_WORST["generate"], (worst, "ragged" if ragged else "plain"))
    third = torch.stack([c["out"]["next"][0] for c in rec.calls]).cpu()
    assert int(third[2]) == eos and bool((third[3:] == PAD).all()), "row 0 must finish at its third token and emit pad afterwards"
    assert seq.shape == (2, L + n_new) and hid.shape[0] == 2


def test_evaluate_forwards_the_sampling_keywords():
    from oracle import cases
    from tests import model_checks as mc, w8_checks as wc
    cfg = cases.tiny_lisa_cfg("sam")
    sd, _, _ = wc.generation_states(cfg)
    sd.update({k: v.to(BF).float() for k, v in cases.sam_decoder_state().items()})
    m = _model(sd, cfg, sam_decoder=True)
    batch = mc._round_batch(cases.tiny_lisa_batch(img_size=cfg.sam.img))
    clip, images, ids = batch["images_clip"][:2].to(DEV), batch["images"][:2].to(DEV), batch["input_ids"][:2].to(DEV)
    resize, orig = [(683, 1024), (1024, 768)], [(427, 640), (96, 72)]
    seq_s, _ = _guarded("generate", lambda: m.generate(clip, ids, max_new_tokens=3, eos_token_id=None, seed=21, **SAMPLING))
    seq_g, _ = _guarded("greedy", lambda: m.generate(clip, ids, max_new_tokens=3, eos_token_id=None))
    ids_s, masks = _guarded("evaluate", lambda: m.evaluate(clip, images, ids, resize, orig, max_new_tokens=3, eos_token_id=None, seed=21, **SAMPLING))
    assert torch.equal(ids_s, seq_s) and len(masks) == 2
    ids_g, _ = _guarded("evaluate greedy", lambda: m.evaluate(clip, images, ids, resize, orig, max_new_tokens=3, eos_token_id=None))
    assert torch.equal(ids_g, seq_g)


def test_bad_sampling_arguments_raise():
    m, clip, ids = _tiny()
    kw = dict(max_new_tokens=3, eos_token_id=None)
    for bad in (dict(temperature=0.5), dict(top_k=5), dict(top_p=0.9), dict(seed=1), dict(return_logprobs=True), dict(uniforms=torch.zeros(2, 3, device=DEV)),
                dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=-1.0), dict(do_sample=True, top_k=-1), dict(do_sample=True, top_p=0.0),
                dict(do_sample=True, top_p=1.01), dict(do_sample=True, seed=1, uniforms=torch.zeros(2, 3, device=DEV)),
                dict(do_sample=True, uniforms=torch.zeros(2, 4, device=DEV))):
        with pytest.raises(ValueError):
            m.generate(clip, ids, **dict(kw, **bad))
    with pytest.raises(ValueError):
        m.generate(clip, ids, weight_bits=4, do_sample=True, **kw)
