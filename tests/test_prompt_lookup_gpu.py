"""GPU: prompt-lookup decoding.  llmseg_decode_attn_chunk on every case of tests/lookup_checks.py against the fp64 reference (Q successive one-row decode steps)
under the bounds tests/test_prompt_lookup_cpu.py validates, and its cache bit for bit against Q successive llmseg_decode_attn_rows steps; llmseg_lookup_draft and
llmseg_lookup_accept exactly against the restated rules; generate(prompt_lookup_num_tokens=) against the oracle's greedy loop on inputs whose every step is
decidable (full token equality), unforced and under forced drafts with the traces the restated loop predicts; ragged prompts with a row that finishes inside a
chunk; the quantised routes against their own yardsticks; graph replay against eager steps; the untouched plain routes; the rejections."""
import dataclasses
import functools
import math

import pytest
import torch

from tests import lookup_checks as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
CHUNK = lc.chunk_cases()
MAX_NEW = 6
# Seeds of the tiny model's weights (w8_checks.generation_states) and the image of every batch row, found on the CPU: the oracle's margin exceeds 2 x MARGIN on all
# MAX_NEW steps of rows 0 and 1.  DISTINCT: the rows emit six different tokens each (nothing to look up: the forced drafts carry the test).  REPEAT: the rows fall
# into repeating one token (margins >= 0.29), so the unforced lookup drafts for real and its drafts are accepted.
DISTINCT, REPEAT = 118, 121
IMAGES = {DISTINCT: [1, 0, 1], REPEAT: [1, 1, 1]}
LENS = (24, 17, 9)             # the ragged rows (tests/test_ragged_decode_gpu.py)
PAD = 0


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield


def _fault_guard(name, e):
    if "HIP error" in str(e) or "illegal memory access" in str(e):          # a device fault: nothing more may be started on this GPU
        pytest.exit(f"{name}: {e}", returncode=3)


def _guarded(name, fn):
    """fn() and a synchronisation; a device fault ends the session"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        _fault_guard(name, e)
        raise


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32 if t.dtype == F32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# 6 ---------------------------------------------------------------------------------------------------------------------------- the attention step
@pytest.mark.parametrize("case", CHUNK, ids=[c.name for c in CHUNK])
def test_decode_attn_chunk_parity_with_fp64_and_with_successive_steps(case):
    from llmseg_amd import _lib, ops
    from tests.test_backward_kernels_gpu import Out
    lib = _lib.load()
    inp, ref, bounds = lc.chunk_reference(case)
    N, H, Q, cap = case.N, case.heads, case.Q, lc.CAP
    D = H * lc.HD
    qkv, cos, sin = (inp[k].to(DEV) for k in ("qkv", "cos", "sin"))
    q0 = qkv.clone()
    o = {}
    for n in ("kc", "vc"):                                  # the caches and the output sit between guard regions
        o[n] = Out(N * cap, D, BF, NAN)
        o[n].w.copy_(inp[n].to(DEV).view(N * cap, D))
        o[n].before = o[n].buf.clone()
    o["out"] = Out(N * Q, D, BF, NAN)
    posd = torch.tensor(case.pos, dtype=torch.int32, device=DEV)
    nf = lc.chunk_scratch_floats(case)
    scratch = torch.full((nf,), NAN, dtype=F32, device=DEV) if nf else None
    cache = lambda n: o[n].w.view(N, cap, D)
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    _guarded(case.name, lambda: ops.decode_attn_chunk(qkv, cos, sin, cache("kc"), cache("vc"), posd, H, lc.HD, Q, out=o["out"].w, scale=inp["scale"], scratch=scratch))
    assert lib.llmseg_launch_count() - n0 == case.launches, f"{case.name}: {lib.llmseg_launch_count() - n0} launches, the table says {case.launches}"
    assert all(b.guard_untouched() for b in o.values()), f"{case.name}: a store outside the buffers (guard region changed)"
    assert _same(qkv, q0), "decode_attn_chunk wrote its qkv operand"
    assert torch.equal(posd.cpu(), torch.tensor(case.pos, dtype=torch.int32)), "the positions were written"
    got = {"out": o["out"].w.cpu(), "kc": cache("kc").cpu(), "vc": cache("vc").cpu()}
    r = lc.chunk_ratios(got, ref, bounds)
    print(f"\n{case.name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    # Q successive per-row steps on a copy of the input caches: the same bits in every cache element (the chunk's slots and all the untouched ones, NaN included)
    kc2, vc2, pos2 = inp["kc"].to(DEV).clone(), inp["vc"].to(DEV).clone(), posd.clone()
    nf1 = nf // Q
    scratch1 = torch.empty(nf1, dtype=F32, device=DEV) if nf1 else None
    out1 = torch.empty((N, D), dtype=BF, device=DEV)
    for j in range(Q):
        _guarded(case.name, lambda: ops.decode_attn(qkv[j::Q], cos, sin, kc2, vc2, pos2, H, lc.HD, out=out1, scale=inp["scale"], scratch=scratch1, per_row=True))
        pos2 += 1
    for k, c2 in (("kc", kc2), ("vc", vc2)):
        assert torch.equal(_bits(got[k]), _bits(c2.cpu())), f"{case.name}: {k} differs from the cache Q successive decode_attn steps leave"
        keep = torch.ones((N, cap), dtype=torch.bool)
        for n, p in enumerate(case.pos):
            keep[n, p:p + Q] = False
        assert torch.equal(_bits(got[k])[keep], _bits(inp[k])[keep]), f"{case.name}: {k} changed outside the chunk's own slots"
    assert r["vc"] == 0.0, r
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"


# 7 ---------------------------------------------------------------------------------------------------------------------- the draft and accept launches
def _draft_problem(rows, k, g, max_new, vocab, pad, forced=None):
    """rows: list of (hist, count, unfinished) -> device inputs and the restated outputs"""
    N, W = len(rows), max(len(h) for h, _, _ in rows) + 3
    hist = torch.full((N, W), -7, dtype=torch.int64)
    for n, (h, _, _) in enumerate(rows):
        hist[n, :len(h)] = torch.tensor(h, dtype=torch.int64)
    tok, dl = torch.full((N, k + 1), pad, dtype=torch.int64), torch.zeros((N,), dtype=torch.int32)
    for n, (h, c, u) in enumerate(rows):
        live = u and c < max_new
        limit = max_new - c - 1 if live else 0
        if forced is None:
            d = lc.draft(h, k, g, limit=limit, vocab=vocab)
        else:
            d = [int(t) for t in forced[n][c:c + k]][:max(0, min(k, limit))]
            d = d[:next((j for j, t in enumerate(d) if not 0 <= t < vocab), len(d))]
        tok[n, 0] = h[-1]
        tok[n, 1:1 + len(d)] = torch.tensor(d, dtype=torch.int64)
        dl[n] = len(d)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return hist.to(DEV), i32([len(h) for h, _, _ in rows]), i32([c for _, c, _ in rows]), i32([u for _, _, u in rows]), tok, dl


def _run_draft(rows, k, g, max_new, vocab, pad=PAD, forced=None):
    from llmseg_amd import ops
    hist, hl, cnt, unf, tok_w, dl_w = _draft_problem(rows, k, g, max_new, vocab, pad, forced)
    before = [t.clone() for t in (hist, hl, cnt, unf)]
    fd = None if forced is None else torch.tensor(forced, dtype=torch.int64, device=DEV)
    tok, dl = _guarded("lookup_draft", lambda: ops.lookup_draft(hist, hl, cnt, unf, k, g, max_new, vocab, pad, forced=fd))
    assert all(torch.equal(a, b) for a, b in zip(before, (hist, hl, cnt, unf))), "lookup_draft wrote an input"
    assert torch.equal(dl.cpu(), dl_w), (k, g, dl.cpu().tolist(), dl_w.tolist())
    assert torch.equal(tok.cpu(), tok_w), (k, g, tok.cpu().tolist(), tok_w.tolist())
    return dl_w


def test_lookup_draft_is_exact():
    for name, hist, k, g, want in lc.draft_hand_cases():
        dl = _run_draft([(hist, 0, 1)], k, g, 100, 32)
        assert int(dl[0]) == len(want), name
    groups = {}
    for i, (h, k, g) in enumerate(lc.draft_random_cases()):
        groups.setdefault((k, g), []).append((h, i % 5, 0 if i % 11 == 0 else 1))
    total = 0
    for (k, g), rows in groups.items():
        total += int(_run_draft(rows, k, g, 8, 6).sum())                      # max_new 8: the limit 8 - count - 1 cuts some drafts
        _run_draft(rows, k, g, 4, 6, pad=3)                                  # rows with count 4 are full
    assert total >= 200, total
    gen = torch.Generator().manual_seed(5)
    # the placeholder and ids beyond the vocabulary end a draft; one case at V = 32004 with ids up to V - 1
    rows = [([1, 2, 3, lc.IMAGE, 5, 1, 2], 0, 1), ([lc.IMAGE, 7, 4, lc.IMAGE], 0, 1), ([4, lc.IMAGE, 7, 4], 0, 1), ([1, 2, 3, 11, 1, 2], 1, 1)]
    _run_draft(rows, 5, 2, 50, 10)
    big = [(torch.cat([torch.tensor([1, lc.IMAGE]), torch.randint(31990, 32004, (60,), generator=gen)]).tolist(), n, 1) for n in range(6)]
    assert int(_run_draft(big, 7, 3, 40, 32004).sum()) >= 6
    assert int(_run_draft(big, 7, 3, 40, 32000).sum()) < int(_run_draft(big, 7, 3, 40, 32004).sum())
    long = [(torch.randint(0, 50, (4000,), generator=gen).tolist(), 3, 1), (torch.randint(0, 3, (4093,), generator=gen).tolist(), 0, 1)]      # more ids than threads
    _run_draft(long, 7, 4, 90, 50)
    forced = torch.randint(0, 12, (len(rows), 9), generator=gen).tolist()      # ids 10 and 11 lie outside the vocabulary of 10
    _run_draft(rows, 3, 2, 9, 10, forced=forced)
    _run_draft([(h, c + 5, u) for h, c, u in rows], 3, 2, 9, 10, forced=forced)


def _run_accept(rows, Q, logits, max_new, eos, first=False, strided=False):
    """rows: list of dict(tok, d, count, unfinished, pos, hist) -> runs the launch and compares every output and every buffer updated in place with the restatement"""
    from llmseg_amd import ops
    N, V = len(rows), logits.shape[1]
    W = max(len(r["hist"]) for r in rows) + Q + 1
    hist = torch.full((N, W), -7, dtype=torch.int64)
    for n, r in enumerate(rows):
        hist[n, :len(r["hist"])] = torch.tensor(r["hist"], dtype=torch.int64)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    hl, cnt, unf, pos = i32([len(r["hist"]) for r in rows]), i32([r["count"] for r in rows]), i32([r["unfinished"] for r in rows]), i32([r["pos"] for r in rows])
    tok, dl = torch.tensor([r["tok"] for r in rows], dtype=torch.int64), i32([r["d"] for r in rows])
    base, dump = torch.arange(N, dtype=torch.int64) * 1000 + 17, 10 ** 6
    lg = logits.to(BF)
    want = dict(hist=hist.clone(), hl=hl.clone(), cnt=cnt.clone(), unf=unf.clone(), pos=pos.clone(), map=torch.full((N * Q,), dump, dtype=torch.int64), rec=torch.zeros((4, N), dtype=torch.int32))
    for n, r in enumerate(rows):
        arg = [lc.argmax_row(lg[n * Q + j]) for j in range(Q)]
        res = lc.accept(r["tok"], r["d"] if r["unfinished"] and r["count"] < max_new else 0, arg, r["count"], r["unfinished"], max_new, eos, r["pos"], first=first)
        e = len(res["emitted"])
        want["hist"][n, len(r["hist"]):len(r["hist"]) + e] = torch.tensor(res["emitted"], dtype=torch.int64)
        want["hl"][n] += e
        want["cnt"][n], want["unf"][n], want["pos"][n] = res["count"], res["unfinished"], res["pos"]
        for j in range(res["stand"]):
            want["map"][n * Q + j] = base[n] + r["count"] + j
        want["rec"][:, n] = torch.tensor([res["unfinished"], res["count"], res["accepted"], r["d"] if r["unfinished"] and r["count"] < max_new else 0])
    dev = lambda t: t.to(DEV)
    hist, hl, cnt, unf, pos, tok, dl, base = map(dev, (hist, hl, cnt, unf, pos, tok, dl, base))
    lgd = lg.to(DEV)
    if strided:
        wide = torch.full((N * Q, V + 5), NAN, dtype=BF, device=DEV)
        wide[:, :V] = lgd
        lgd = wide[:, :V]
    hmap = torch.full((N * Q,), -1, dtype=torch.int64, device=DEV)
    l0 = lgd.clone()
    rec = _guarded("lookup_accept", lambda: ops.lookup_accept(lgd, None if first else tok, None if first else dl, hist, hl, pos, unf, cnt, max_new, eos_token_id=eos, first=first,
                                                              base=base, dump_row=dump, map=hmap))
    assert _same(lgd.contiguous(), l0.contiguous()), "lookup_accept wrote the logits"
    got = dict(hist=hist, hl=hl, cnt=cnt, unf=unf, pos=pos, map=hmap, rec=rec)
    for k, w in want.items():
        assert torch.equal(got[k].cpu(), w), (k, got[k].cpu().tolist(), w.tolist())
    return want


def test_lookup_accept_is_exact():
    for name, a, want in lc.accept_cases():                 # the hand-built tables, one row each
        Q = a["logits"].shape[0]
        row = dict(tok=a["tok"], d=a["d"], count=a["count"], unfinished=a["unfinished"], pos=a["pos"], hist=[3, 1, 4, 1, a["tok"][0]])
        w = _run_accept([row], Q, a["logits"], a["max_new"], a["eos"])
        assert int(w["rec"][2, 0]) == want["accepted"] and int(w["cnt"][0]) == want["count"] and int(w["pos"][0]) == want["pos"], name
    gen = torch.Generator().manual_seed(9)
    for V, Q, N, strided in ((16, 4, 7, False), (5, 8, 5, True), (300, 2, 9, False), (32004, 4, 3, True)):      # seeded tables; few distinct values: equal maxima abound
        for eos in (None, 2):
            logits = torch.randint(-3, 4, (N * Q, V), generator=gen).float() * 0.5
            if V > 100:
                logits[:, -1] = 1.5                            # the last id ties with earlier ones: the lowest index must win across the whole row
            arg = logits.to(BF).float().argmax(-1).view(N, Q)
            rows = []
            for n in range(N):
                d = int(torch.randint(0, Q, (1,), generator=gen))
                right = int(torch.randint(0, d + 1, (1,), generator=gen))      # the first `right` drafts are the arg-maxes
                tok = [1] + [int(arg[n, j]) if j < right else (int(arg[n, j]) + 1) % V for j in range(Q - 1)]
                rows.append(dict(tok=tok, d=d, count=n % 7, unfinished=0 if n == 3 else 1, pos=30 + n, hist=[0] * (2 + n)))
            _run_accept(rows, Q, logits, 6, eos, strided=strided)
    logits = torch.randn((4, 40), generator=gen)            # the pick after the prefill: Q = 1, no drafts, the position stays
    logits[1, 7] = logits[1, 30] = 9.0
    rows = [dict(tok=[0], d=0, count=0, unfinished=1, pos=20 + n, hist=[5, 6, 7][:1 + n % 3]) for n in range(4)]
    w = _run_accept(rows, 1, logits, 3, int(logits[2].to(BF).float().argmax()), first=True)
    assert w["pos"].tolist() == [20, 21, 22, 23] and w["cnt"].tolist() == [1, 1, 1, 1] and w["unf"].tolist() == [1, 1, 0, 1] and int(w["hist"][1, 2]) == 7


# ---------------------------------------------------------------------------------------------------------------------------------- generation
def _model(sd, cfg):
    from llmseg_amd import lisa as hip_lisa
    from tests import model_checks as mc
    m = hip_lisa.LISAForCausalLM(mc.to_hip_cfg(cfg), device=DEV)
    missing, _ = m.load_state_dict(sd, strict=False)
    assert not missing, missing[:5]
    return m


@functools.lru_cache(maxsize=None)
def _setup(seed=REPEAT):
    from oracle import cases
    from tests import model_checks as mc, mxfp4_checks as xc
    cfg = cases.tiny_lisa_cfg(lora_r=0)
    sd, sd_4, sd_8, _ = xc.generation_states_mxfp4(cfg, seed)
    batch = mc._round_batch(cases.tiny_lisa_batch())
    return dict(cfg=cfg, sd=sd, sd_q={8: sd_8, "mxfp4": sd_4}, m=_model(sd, cfg), clip=batch["images_clip"][IMAGES[seed]], ids=batch["input_ids"][:3])


@functools.lru_cache(maxsize=None)
def _oracle(seed, rows):
    """the oracle's greedy loop on the given rows of the batch, with its margins; shared, not written to"""
    from oracle import generate as ogen
    s = _setup(seed)
    idx = list(rows)
    margins = []
    with torch.no_grad():
        seq, hid = ogen.greedy_generate(s["sd"], s["cfg"], s["clip"][idx], s["ids"][idx], max_new_tokens=MAX_NEW, eos_token_id=None, margins=margins)
    return seq, hid, torch.stack(margins, 1)


def _teacher(seqs, V):
    """the device's own sequences as a forward for the restated loop: a greedy model's logits at a position of its own sequence point at the next token (what follows
    a rejected draft is never read)"""
    def forward(n, ids):
        own = seqs[n]
        out = torch.zeros((len(ids), V))
        for t in range(len(ids)):
            if t + 1 < len(own) and own[t + 1] >= 0 and ids[:t + 1] == own[:t + 1]:
                out[t, own[t + 1]] = 1.0
        return out
    return forward


@pytest.mark.parametrize("rows", ((0, 1), (0,)), ids=("N2", "N1"))
@pytest.mark.parametrize("k", (1, 3, 7))
def test_generate_equals_the_oracle_where_every_step_is_decidable(k, rows):
    _check_against_the_oracle(DISTINCT, k, rows)


@pytest.mark.parametrize("k", (1, 3))
def test_generate_unforced_drafts_are_accepted_on_a_repeating_continuation(k):
    traces = _check_against_the_oracle(REPEAT, k, (0, 1))
    assert sum(sum(t["accepted"]) for t in traces[None]) >= 2, traces[None]
    assert len(traces[None]) < MAX_NEW - 1, "accepted drafts must have saved steps"


def _check_against_the_oracle(seed, k, rows):
    from tests import generate_checks as gchk
    s = _setup(seed)
    seq_r, hid_r, mg = _oracle(seed, rows)
    print(f"\noracle margins {[['%.2f' % x for x in r] for r in mg.tolist()]}")
    assert float(mg.min()) > 2 * gchk.MARGIN, f"precondition: every step of every row must be decidable (smallest margin {float(mg.min()):.3f})"
    idx = list(rows)
    clip, ids = s["clip"][idx].to(DEV), s["ids"][idx].to(DEV)
    N, L = ids.shape
    cont = seq_r[:, L:]
    tol = 3e-2 * max(1.0, hid_r.abs().max().item())
    prompts = [r.tolist() for r in s["ids"][idx]]
    V = s["cfg"].llama.vocab
    traces = {}
    for kind in (None, "right", "mixed"):
        forced = None if kind is None else lc.forced_drafts(cont, kind, V)
        trace = traces[kind] = []
        seq, hid = _guarded("generate", lambda: s["m"].generate(clip, ids, max_new_tokens=MAX_NEW, eos_token_id=None, prompt_lookup_num_tokens=k, _lookup_forced=forced,
                                                                _lookup_trace=trace))
        seq, hid = seq.cpu(), hid.float().cpu()
        err = (hid - hid_r).abs().max().item() if hid.shape == hid_r.shape else NAN
        print(f"k={k} forced={kind}: steps {len(trace)}, accepted {[t['accepted'] for t in trace]}, hidden err {err:.3e} (tol {tol:.3e})")
        assert seq.shape == seq_r.shape and torch.equal(seq, seq_r), (kind, seq[:, L:].tolist(), seq_r[:, L:].tolist())
        assert hid.shape == hid_r.shape and err <= tol, (kind, err, tol)
        want = []
        lc.lookup_generate(_teacher([r.tolist() for r in seq], V), prompts, k, 2, MAX_NEW, forced=None if forced is None else forced.tolist(), trace=want, vocab=V)
        assert trace == want, (kind, trace, want)
        if kind == "right":                                    # every draft is accepted: k per step until max_new_tokens cuts the last chunk
            assert len(trace) == math.ceil((MAX_NEW - 1) / (k + 1))
            left = MAX_NEW - 1
            for t in trace:
                assert t["accepted"] == t["draft_len"] == [min(k, left - 1)] * N, (t, left)
                left -= min(k, left - 1) + 1
        if kind == "mixed":
            assert any(a < d for t in trace for a, d in zip(t["accepted"], t["draft_len"])), "a wrong draft must have been rejected"
    return traces


@functools.lru_cache(maxsize=None)
def _ragged_run(mode, n_rows, seed=REPEAT):
    """one generate(prompt_lookup_num_tokens=3) call on ragged (n_rows = 3) or single (n_rows = 1) prompts in the given weight mode and, per row, its yardstick's
    teacher-forced forward on the row alone; shared, not written to"""
    from llmseg_amd.generate import pad_prompts
    from oracle import lisa as olisa
    s = _setup(seed)
    osd = s["sd"] if mode is None else s["sd_q"][mode]
    lens = LENS[:n_rows] if n_rows == 3 else (LENS[0],)
    rows = [s["ids"][i, :n].clone() for i, n in enumerate(lens)]
    ids, mask = pad_prompts(rows, PAD)
    kw = {} if mode is None else dict(weight_bits=8) if mode == 8 else dict(weight_format="mxfp4")
    trace = []
    seq, hid = _guarded("generate", lambda: s["m"].generate(s["clip"][:n_rows].to(DEV), ids.to(DEV), max_new_tokens=MAX_NEW, eos_token_id=None, pad_token_id=PAD,
                                                            attention_mask=mask.to(DEV), prompt_lookup_num_tokens=3, _lookup_trace=trace, **kw))
    seq, hid = seq.cpu(), hid.cpu()
    oracle = []
    with torch.no_grad():
        for i, L in enumerate(lens):
            fed = seq[i:i + 1, :L + MAX_NEW - 1]                # teacher forcing: the row's prompt and the tokens the HIP path chose, all but the last
            _, lg, h = olisa.llava_forward(osd, s["cfg"], s["clip"][i:i + 1], torch.ones_like(fed, dtype=torch.bool), fed)
            oracle.append((lg[0].float(), h[0].float()))
    return dict(lens=lens, rows=rows, ids=ids, mask=mask, seq=seq, hid=hid, oracle=oracle, trace=trace, kw=kw)


def _check_against_yardstick(mode, n_rows, seed=REPEAT):
    """the margin rule as tests/test_ragged_decode_gpu.py and tests/test_w8_decode_gpu.py apply it: every chosen token within MARGIN of the yardstick's best logit at its
    position, every hidden state within the tolerance; the layouts exactly"""
    from tests import generate_checks as gchk
    s, run = _setup(seed), _ragged_run(mode, n_rows, seed)
    cfg, seq, hid, lens = s["cfg"], run["seq"], run["hid"].float(), run["lens"]
    Pn, Lm = cfg.n_img_tokens, max(lens)
    Tm = Lm - 1 + Pn
    tol = 3e-2 * max(1.0, max(h.abs().max().item() for _, h in run["oracle"]))
    assert seq.shape == (len(lens), Lm + MAX_NEW) and hid.shape == (len(lens), Tm + MAX_NEW - 1, cfg.llama.hidden)
    errs, gaps = [], []
    for i, L in enumerate(lens):
        T_i = L - 1 + Pn
        assert torch.equal(seq[i, :L], run["rows"][i]) and bool((seq[i, L + MAX_NEW:] == PAD).all()), f"row {i}: prompt, tokens, fill"
        assert bool((run["hid"][i, T_i + MAX_NEW - 1:].view(torch.int16) == 0).all()), f"row {i}: zeros after the row's last hidden state"
        lg, h = run["oracle"][i]
        errs.append((hid[i, :T_i + MAX_NEW - 1] - h).abs().max().item())
        steps = lg[T_i - 1:]
        gaps.append(steps.max(-1).values - steps.gather(-1, seq[i, L:L + MAX_NEW][:, None])[:, 0])
    gap = torch.stack(gaps)
    print(f"\nmode={mode} rows={n_rows}: steps {len(run['trace'])}, accepted {[t['accepted'] for t in run['trace']]}, hidden err {['%.3e' % e for e in errs]} (tol {tol:.3e}), "
          f"worst logit gap {gap.max().item():.3e} (MARGIN {gchk.MARGIN})")
    assert max(errs) <= tol, f"hidden states differ from the yardstick by {max(errs):.3e} > {tol:.3e}"
    assert bool((gap <= gchk.MARGIN).all()), f"a chosen token is {gap.max().item():.3e} below the yardstick's best logit"


# 9
def test_generate_ragged_prompts_and_a_row_that_finishes_inside_a_chunk():
    _check_against_yardstick(None, 3, DISTINCT)
    s, run = _setup(DISTINCT), _ragged_run(None, 3, DISTINCT)
    cfg, lens = s["cfg"], run["lens"]
    Pn, Lm = cfg.n_img_tokens, max(lens)
    base = torch.stack([run["seq"][i, L:L + MAX_NEW] for i, L in enumerate(lens)])
    ids, mask, pad = run["ids"].to(DEV), run["mask"].to(DEV), 7
    gen = lambda eos, trace: _guarded("generate", lambda: s["m"].generate(s["clip"].to(DEV), ids, max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=pad, attention_mask=mask,
                                                                          prompt_lookup_num_tokens=3, _lookup_forced=base.to(DEV), _lookup_trace=trace))
    # forced drafts = the unforced run's continuation, first without eos: the pick emits token 0 and the first step the accepted drafts and one more.  Then the same
    # call with an eos: the chunks are the same until a row finishes and rows do not influence each other, so every row must repeat its tokens and states bit for bit
    t_free, t_eos = [], []
    free, hid_free = (t.cpu() for t in gen(None, t_free))
    toks = torch.stack([free[i, L:L + MAX_NEW] for i, L in enumerate(lens)])
    # the eos: an ACCEPTED draft of the first step (token j <= a_r of row r, new to that row), so that the row finishes inside the chunk, what was accepted behind it
    # is dropped, and another row goes on
    pick = None
    for r in range(3):
        for j in range(1, t_free[0]["accepted"][r] + 1):
            e = int(toks[r, j])
            stops = [int((toks[i] == e).nonzero().flatten()[0]) + 1 if bool((toks[i] == e).any()) else MAX_NEW for i in range(3)]
            if pick is None and stops[r] == j + 1 and max(stops) > j + 1:
                pick = (r, j, e, stops)
    print(f"\ntokens without eos {toks.tolist()}, first step {t_free[0]}, pick {pick}")
    assert pick is not None, "precondition: some row's accepted draft must be usable as an eos while another row goes on"
    r, j, eos, stops = pick
    n_new = max(stops)
    seq, hid = (t.cpu() for t in gen(eos, t_eos))
    print(f"eos {eos}: with eos {[seq[i, L:].tolist() for i, L in enumerate(lens)]}, trace {t_eos}")
    assert seq.shape == (3, Lm + n_new) and hid.shape == (3, Lm - 1 + Pn + n_new - 1, cfg.llama.hidden)
    for i, L in enumerate(lens):
        c, T_i = stops[i], L - 1 + Pn
        assert torch.equal(seq[i, :L], run["rows"][i]) and torch.equal(seq[i, L:L + c], toks[i, :c]) and bool((seq[i, L + c:] == pad).all()), (i, seq[i, L:].tolist())
        assert _same(hid[i, :T_i + c - 1], hid_free[i, :T_i + c - 1]), f"row {i}: the prefill states and the state of every token it emitted but the last"
        assert bool((hid[i, T_i + c - 1:].view(torch.int16) == 0).all()), f"row {i}: zeros after the state of its last fed token"
    assert t_eos[0]["accepted"][r] == t_free[0]["accepted"][r] >= j, "the eos was an accepted draft"
    assert all(t["draft_len"][r] == 0 and t["accepted"][r] == 0 for t in t_eos[1:]) and len(t_eos) > 1, "a finished row drafts and accepts nothing while the others go on"


# 10
@pytest.mark.parametrize("n_rows", (1, 3), ids=("one_gemm_call", "chunked_rows"))
@pytest.mark.parametrize("mode", (8, "mxfp4"))
def test_generate_quantised_routes_against_their_yardsticks(mode, n_rows):
    _check_against_yardstick(mode, n_rows)


# 11
def test_graph_replay_equals_eager_steps_and_the_states_do_not_meet():
    s = _setup()
    m = s["m"]
    clip, ids = s["clip"][:2].to(DEV), s["ids"][:2].to(DEV)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None)
    gen = lambda **k: _guarded("generate", lambda: m.generate(clip, ids, **kw, **k))
    plain_a = gen()
    mixed = lc.forced_drafts(_oracle(REPEAT, (0, 1))[0][:, ids.shape[1]:], "mixed", s["cfg"].llama.vocab)      # several steps per call: the second one captures, later ones replay
    look_a = gen(prompt_lookup_num_tokens=1, _lookup_forced=mixed)
    key = next(k for k in m.__dict__["_decode_states"] if "lookup" in k)
    st = m.__dict__["_decode_states"][key]
    assert key[-2:] == ("lookup", 2) and st.q == 2 and st.x.shape[0] == 4 and st.k.shape[1] == 2, (key, st.x.shape, st.k.shape)
    graph = st.graph
    assert graph is not None, "the call has more than two steps: the step must have been captured"
    look_b = gen(prompt_lookup_num_tokens=1, _lookup_forced=mixed)
    assert m.__dict__["_decode_states"][key] is st and st.graph is graph, "a second call on the same state reuses the graph"
    eager = gen(prompt_lookup_num_tokens=1, _lookup_forced=mixed, use_graph=False)
    plain_b = gen()
    assert torch.equal(look_a[0], look_b[0]) and _same(look_a[1], look_b[1]), "two calls on one state differ"
    assert torch.equal(look_a[0], eager[0]) and _same(look_a[1], eager[1]), "eager steps and the replayed graph differ"
    assert torch.equal(plain_a[0], plain_b[0]) and _same(plain_a[1], plain_b[1]), "a plain call after a lookup call differs from one before it"
    assert all(("lookup" in k) == (v.q > 1) for k, v in m.__dict__["_decode_states"].items())


# 12
def test_rejections_and_untouched_defaults():
    from oracle import cases
    s = _setup()
    m = s["m"]
    clip, ids = s["clip"][:2].to(DEV), s["ids"][:2].to(DEV)
    kw = dict(max_new_tokens=3, eos_token_id=None)
    for bad, word in ((dict(do_sample=True), "do_sample"), (dict(num_beams=2), "num_beams"), (dict(repetition_penalty=1.3), "repetition_penalty"),
                      (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(min_new_tokens=1, eos_token_id=2), "min_new_tokens"), (dict(suppress_tokens=[5]), "suppress_tokens"),
                      (dict(kv_format="mxfp8"), "kv_format"), (dict(fuse_decode=False), "fuse_decode")):
        with pytest.raises(ValueError, match=word):
            m.generate(clip, ids, prompt_lookup_num_tokens=3, **{**kw, **bad})
    for k in (0, 8, 2.5, True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            m.generate(clip, ids, prompt_lookup_num_tokens=k, **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        m.generate(clip, ids, prompt_lookup_num_tokens=3, max_matching_ngram_size=0, **kw)
    with pytest.raises(ValueError, match="needs prompt_lookup_num_tokens"):
        m.generate(clip, ids, max_matching_ngram_size=3, **kw)
    with pytest.raises(ValueError, match="cap of"):
        m.generate(clip, ids, prompt_lookup_num_tokens=3, max_new_tokens=5000, eos_token_id=None)
    cfg64 = dataclasses.replace(s["cfg"], llama=dataclasses.replace(s["cfg"].llama, heads=4))                        # head_dim 64: the two-launch route
    m64 = _model({k: v.to(BF).float() for k, v in cases.tiny_lisa_state(cfg64).items()}, cfg64)
    with pytest.raises(ValueError, match="head_dim 128"):
        m64.generate(clip, ids, prompt_lookup_num_tokens=3, **kw)
    # the plain routes with the new arguments at their defaults: bit-identical to a call that does not name them
    from llmseg_amd.generate import pad_prompts
    rids, rmask = (t.to(DEV) for t in pad_prompts([s["ids"][i, :n].clone() for i, n in enumerate(LENS[:2])], PAD))
    for extra in (dict(), dict(weight_bits=8), dict(do_sample=True, seed=3, top_k=5), dict(num_beams=2)):
        a = _guarded("generate", lambda: m.generate(clip, ids, **kw, **extra))
        b = _guarded("generate", lambda: m.generate(clip, ids, prompt_lookup_num_tokens=None, max_matching_ngram_size=2, **kw, **extra))
        assert torch.equal(a[0], b[0]) and _same(a[1], b[1]), extra
    a = _guarded("generate", lambda: m.generate(clip, rids, attention_mask=rmask, **kw))
    b = _guarded("generate", lambda: m.generate(clip, rids, attention_mask=rmask, prompt_lookup_num_tokens=None, max_matching_ngram_size=2, **kw))
    assert torch.equal(a[0], b[0]) and _same(a[1], b[1])
