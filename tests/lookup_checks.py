"""Prompt-lookup decoding (generate(prompt_lookup_num_tokens=); llmseg_lookup_draft, llmseg_lookup_accept, llmseg_decode_attn_chunk): CPU restatements of the
draft rule, the accept rule and the loop around any deterministic forward; their case tables and mutants; and the fp64 reference, emulation and mutants of the
chunk attention step.  CPU only, no import of the HIP library.

The draft rule is Hugging Face's PromptLookupCandidateGenerator.get_candidates without a logits processor (tests/test_prompt_lookup_cpu.py pins `draft` against
the installed class).  Two deliberate differences, both stated in include/llmseg_hip.h: the installed class cuts a candidate in front of an eos id -- here an eos
may be drafted, because the accept rule itself ends the emission after the first eos, so an accepted eos finishes the row one step earlier and the tokens are the
same; and the installed class knows no ids outside the vocabulary, whereas a history here holds the <image> placeholder (-200), in front of which a draft is cut.
The installed class's `max_length` only ever acts through its early return (`max_length == input_length + 1`: no candidates when one token is left); here the
draft is cut to `limit` = max_new_tokens - emitted - 1 ids, which is 0 in that case.

The chunk attention step is not restated: its reference is tests/forward_kernel_checks.py::decode_compute applied Q times to one-row problems at pos_n + j on the
cache the earlier chunk tokens' stored bf16 rows produce, under that module's per-element bounds (bf16_bound on `out` and the new k rows, zero elsewhere)."""
import functools

import torch

from tests import forward_kernel_checks as fk
from tests.forward_kernel_checks import CAP, EMU_MAX, HD, MUT_MIN, Case, decode_compute, decode_splits, ratio      # noqa: F401  (re-exported)

BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")
IMAGE = -200


# ------------------------------------------------------------------------------------------------------------------------------ the draft rule
def draft(hist, k, g, limit=None, vocab=None, mut=None):
    """hist: list of ids -> the draft (a list of at most k ids).  g = max_matching_ngram_size; limit: at most this many ids (None: k); vocab: cut in front of the
    first id outside [0, vocab) (None: no cut).  mut = "latest_match": the latest window instead of the earliest."""
    n = len(hist)
    out = []
    for size in range(min(g, n - 1), 0, -1):
        tail = hist[n - size:]
        starts = [i for i in range(n - size + 1) if hist[i:i + size] == tail and i + size < n]      # a non-empty continuation: the tail itself is no match
        if starts:
            i = starts[-1] if mut == "latest_match" else starts[0]
            out = hist[i + size:i + size + k]
            break
    out = out[:k if limit is None else max(0, min(k, limit))]
    if vocab is not None:
        for j, t in enumerate(out):
            if not 0 <= t < vocab:
                return out[:j]
    return out


def hf_draft(hist, k, g):
    """the installed transformers' candidate generator on the same history (no eos, no logits processor, max_length out of reach)"""
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=k, max_matching_ngram_size=g, max_length=10 ** 6)
    ids = torch.tensor([hist], dtype=torch.int64)
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(hist):].tolist()


def draft_hand_cases():
    """(name, hist, k, g, expected)"""
    return [
        ("no_match", [1, 2, 3, 4, 5], 3, 2, []),
        ("match_only_at_the_tail", [7, 8, 9], 3, 2, []),                                # [8, 9] and [9] occur at the tail alone: no continuation
        ("single_token", [5], 3, 2, []),
        ("continuation_shorter_than_k", [1, 2, 3, 9, 1, 2], 5, 2, [3, 9, 1, 2]),
        ("continuation_of_one", [4, 7, 4], 5, 2, [7, 4]),
        ("two_matches_earliest_wins", [1, 2, 5, 6, 1, 2, 7, 8, 1, 2], 2, 2, [5, 6]),
        ("longer_ngram_preferred", [3, 2, 9, 9, 1, 2, 7, 7, 1, 2], 2, 2, [7, 7]),      # the 1-gram "2" matches earlier (-> 9 9); the 2-gram "1 2" is taken
        ("falls_back_to_shorter_ngram", [3, 2, 9, 9, 5, 2], 2, 2, [9, 9]),
        ("tail_overlaps_its_match", [6, 6, 6], 4, 2, [6]),                              # window [6, 6] at 0 continues with the last id only
        ("g3", [1, 2, 3, 4, 0, 2, 3, 5, 1, 2, 3], 3, 3, [4, 0, 2]),
    ]


def draft_random_cases(count=400, seed=11):
    """seeded histories over a vocabulary of 4 - 6 ids (matches abound), lengths 1 .. 40, g in {1, 2, 3}, k in {1 .. 7}"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(count):
        V = 4 + i % 3
        n = 1 + int(torch.randint(0, 40, (1,), generator=g))
        out.append((torch.randint(0, V, (n,), generator=g).tolist(), 1 + i % 7, 1 + (i // 7) % 3))
    return out


def check_draft(draft_fn):
    """-> the list of failures of `draft_fn` against the hand-built rows and against the installed class on the seeded histories"""
    bad = []
    for name, hist, k, g, want in draft_hand_cases():
        got, hf = draft_fn(hist, k, g), hf_draft(hist, k, g)
        if want != hf:
            bad.append(f"{name}: the table says {want}, the installed class {hf}")
        if got != want:
            bad.append(f"{name}: {got} != {want}")
    for hist, k, g in draft_random_cases():
        got, hf = draft_fn(hist, k, g), hf_draft(hist, k, g)
        if got != hf:
            bad.append(f"hist {hist} k {k} g {g}: {got} != {hf}")
    return bad


# ----------------------------------------------------------------------------------------------------------------------------- the accept rule
def argmax_row(row):
    """the lowest index among equal maxima (torch.argmax)"""
    return int(torch.as_tensor(row).float().argmax())


def accept(tok, d, arg, count, unfinished, max_new, eos, pos, first=False, mut=None):
    """One row.  tok: the fed tokens (tok[0] the last emitted one, tok[1 .. d] the draft); arg: the arg-max of every step row; count tokens emitted so far.
    -> dict(accepted, emitted = the list of tokens, count, unfinished, pos, stand = how many step rows hold the state of a token of the sequence)."""
    if not unfinished or count >= max_new:
        return dict(accepted=0, emitted=[], count=count, unfinished=unfinished, pos=pos, stand=0)
    a = 0
    while a < d and tok[1 + a] == arg[a]:
        a += 1
    if mut == "accepted_plus_one":
        a = min(a + 1, len(arg) - 1)
    elif mut == "accepted_minus_one":
        a = max(a - 1, 0)
    room = min(a if mut == "no_extra_token" else a + 1, max_new - count)
    out, fin = [], False
    while len(out) < room and not fin:
        out.append(arg[len(out)])
        fin = eos is not None and out[-1] == eos and mut != "eos_ignored"
    e = len(out)
    adv = 0 if first else (len(arg) if mut == "pos_by_Q" else e)
    return dict(accepted=a, emitted=out, count=count + e, unfinished=0 if fin else 1, pos=pos + adv, stand=0 if first else e)


def _table(rows, V=8):
    """logits [len(rows), V] with row j's maximum at rows[j] (a pair (a, b): two equal maxima at a and b)"""
    lg = (-0.25 * torch.arange(V, dtype=torch.float32)).repeat(len(rows), 1)      # (exact in bf16)
    for j, r in enumerate(rows):
        for t in (r if isinstance(r, tuple) else (r,)):
            lg[j, t] = 3.0
    return lg


def accept_cases():
    """(name, dict(tok, d, logits rows, count, unfinished, max_new, eos, pos), expected dict)"""
    c = []

    def add(name, tok, d, tops, count0, unfinished0, max_new, eos, pos0, **want):
        c.append((name, dict(tok=tok, d=d, logits=_table(tops), count=count0, unfinished=unfinished0, max_new=max_new, eos=eos, pos=pos0), want))
    add("all_accepted", [5, 1, 2, 3], 3, [1, 2, 3, 4], 2, 1, 20, 7, 40, accepted=3, emitted=[1, 2, 3, 4], count=6, unfinished=1, pos=44, stand=4)
    add("none_accepted", [5, 1, 2, 3], 3, [6, 2, 3, 4], 2, 1, 20, 7, 40, accepted=0, emitted=[6], count=3, unfinished=1, pos=41, stand=1)
    add("partial", [5, 1, 2, 3], 3, [1, 2, 6, 4], 2, 1, 20, 7, 40, accepted=2, emitted=[1, 2, 6], count=5, unfinished=1, pos=43, stand=3)
    add("short_draft", [5, 1, 0, 0], 1, [1, 0, 0, 0], 2, 1, 20, 7, 40, accepted=1, emitted=[1, 0], count=4, unfinished=1, pos=42, stand=2)      # the pad after the draft is no draft
    add("accepted_draft_is_eos", [5, 1, 7, 3], 3, [1, 7, 3, 4], 2, 1, 20, 7, 40, accepted=3, emitted=[1, 7], count=4, unfinished=0, pos=42, stand=2)
    add("extra_token_is_eos", [5, 1, 2, 3], 3, [1, 7, 3, 4], 2, 1, 20, 7, 40, accepted=1, emitted=[1, 7], count=4, unfinished=0, pos=42, stand=2)
    add("max_new_cut_mid_chunk", [5, 1, 2, 3], 3, [1, 2, 3, 4], 4, 1, 6, 7, 40, accepted=3, emitted=[1, 2], count=6, unfinished=1, pos=42, stand=2)
    add("finished_row", [5, 1, 2, 3], 3, [1, 2, 3, 4], 2, 0, 20, 7, 40, accepted=0, emitted=[], count=2, unfinished=0, pos=40, stand=0)
    add("full_row", [5, 1, 2, 3], 3, [1, 2, 3, 4], 6, 1, 6, 7, 40, accepted=0, emitted=[], count=6, unfinished=1, pos=40, stand=0)
    add("two_equal_maxima_lowest_wins", [5, 2, 3, 3], 3, [(2, 6), (4, 3), 1, 1], 2, 1, 20, 7, 40, accepted=2, emitted=[2, 3, 1], count=5, unfinished=1, pos=43, stand=3)
    add("no_eos", [5, 1, 7, 3], 3, [1, 7, 3, 4], 2, 1, 20, None, 40, accepted=3, emitted=[1, 7, 3, 4], count=6, unfinished=1, pos=44, stand=4)
    return c


def check_accept(accept_fn):
    bad = []
    for name, a, want in accept_cases():
        arg = [argmax_row(r) for r in a["logits"]]
        got = accept_fn(a["tok"], a["d"], arg, a["count"], a["unfinished"], a["max_new"], a["eos"], a["pos"])
        if got != want:
            bad.append(f"{name}: {got} != {want}")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------- the loop
def lookup_generate(forward, prompts, k, g, max_new, eos=None, pad=0, forced=None, trace=None, vocab=None, draft_fn=draft, accept_fn=accept):
    """The restated loop on rows that do not influence each other.  forward(n, ids: list) -> logits [len(ids), V] of row n (causal: row t depends on ids[:t + 1]).
    prompts: a list of id lists.  forced: [N][max_new] drafts instead of the lookup.  trace receives, per step, dict(draft_len, accepted) over the rows.
    -> (rows: prompt + emitted tokens, counts)."""
    N = len(prompts)
    seqs = [list(p) for p in prompts]
    st = [dict(count=0, unfinished=1, pos=0) for _ in range(N)]
    for n in range(N):
        r = accept_fn([], 0, [argmax_row(forward(n, seqs[n])[-1])], 0, 1, max_new, eos, 0, first=True)
        seqs[n] += r["emitted"]
        st[n].update(count=r["count"], unfinished=r["unfinished"])
    for _ in range(4 * max_new + 4):                            # (a mutant that emits nothing must not loop for ever)
        if not any(s["unfinished"] and s["count"] < max_new for s in st):
            break
        dl, ac = [], []
        for n in range(N):
            s = st[n]
            live = s["unfinished"] and s["count"] < max_new
            d = []
            if live:
                limit = max_new - s["count"] - 1
                if forced is not None:
                    d = [int(t) for t in forced[n][s["count"]:s["count"] + k]][:max(0, min(k, limit))]
                    if vocab is not None and any(not 0 <= t < vocab for t in d):
                        d = d[:next(j for j, t in enumerate(d) if not 0 <= t < vocab)]
                else:
                    d = draft_fn(seqs[n], k, g, limit=limit, vocab=vocab)
            if live:
                lg = forward(n, seqs[n] + d)[len(seqs[n]) - 1:]
                r = accept_fn([seqs[n][-1]] + d, len(d), [argmax_row(x) for x in lg], s["count"], 1, max_new, eos, s["pos"])
                seqs[n] += r["emitted"]
                s.update(count=r["count"], unfinished=r["unfinished"], pos=r["pos"])
                ac.append(r["accepted"])
            else:
                ac.append(0)
            dl.append(len(d))
        if trace is not None:
            trace.append(dict(draft_len=dl, accepted=ac))
    return seqs, [s["count"] for s in st]


def pack(prompts, seqs, counts, pad):
    """the result layout: row i = its prompt (right-padded to the longest), its count_i tokens, then pad -> int64 [N, Lm + n_new]"""
    Lm, n_new = max(len(p) for p in prompts), max(counts)
    out = torch.full((len(prompts), Lm + n_new), pad, dtype=torch.int64)
    for i, (p, s) in enumerate(zip(prompts, seqs)):
        out[i, :len(s)] = torch.tensor(s, dtype=torch.int64)
    return out


def toy_forward(seed, V=6, decay=0.6):
    """a seeded causal fp64 model over V ids: logits[t] = sum_{s <= t} decay^(t - s) * W[ids[s]] + B[ids[t]]; -> (batched forward for oracle.generate.greedy_generate,
    per-row forward for lookup_generate)"""
    g = torch.Generator().manual_seed(seed)
    W, Bm = torch.randn(V, V, generator=g, dtype=F64), torch.randn(V, V, generator=g, dtype=F64)

    def rows(ids):
        acc, out = torch.zeros(V, dtype=F64), []
        for t in ids:
            acc = acc * decay + W[t]
            out.append(acc + Bm[t])
        return torch.stack(out)

    def batched(ids):
        return torch.stack([rows(r.tolist()) for r in ids]), None
    return batched, lambda n, ids: rows(ids)


def invariance_cases():
    """(seed, N, L, k, g, eos, max_new) of the toy forward"""
    out = []
    for i, (k, g) in enumerate(((1, 1), (2, 2), (3, 2), (5, 3), (7, 2), (3, 1), (7, 3), (4, 2))):
        for eos in (None, 1, 4):
            for max_new in (1, 2, 9, 24):
                out.append((100 + i, 3, 5 + i % 3, k, g, eos, max_new))
    return out


def forced_drafts(cont, kind, V):
    """cont int64 [N, max_new]: the greedy continuation -> forced drafts that are all right, all wrong, or right at every second position"""
    if kind == "right":
        return cont.clone()
    wrong = (cont + 1) % V
    if kind == "wrong":
        return wrong
    return torch.where(torch.arange(cont.shape[1])[None, :] % 2 == 0, cont, wrong)


def check_invariance(draft_fn=draft, accept_fn=accept, cases=None):
    """the restated loop returns exactly oracle.generate.greedy_generate's sequences on the same forward, unforced and under forced drafts"""
    from oracle import generate as ogen
    bad = []
    for seed, N, L, k, g, eos, max_new in (invariance_cases() if cases is None else cases):
        batched, per_row = toy_forward(seed)
        gen = torch.Generator().manual_seed(seed)
        ids = torch.randint(0, 6, (N, L), generator=gen)
        want, _ = ogen.greedy_generate(None, None, None, ids, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=0, forward=batched)
        free, _ = ogen.greedy_generate(None, None, None, ids, max_new_tokens=max_new, eos_token_id=None, forward=batched)
        prompts = [r.tolist() for r in ids]
        for kind in (None, "right", "wrong", "mixed"):
            forced = None if kind is None else forced_drafts(free[:, L:], kind, 6).tolist()
            seqs, counts = lookup_generate(per_row, prompts, k, g, max_new, eos=eos, pad=0, forced=forced, draft_fn=draft_fn, accept_fn=accept_fn)
            got = pack(prompts, seqs, counts, 0)
            if got.shape != want.shape or not torch.equal(got, want):
                bad.append(f"seed {seed} k {k} g {g} eos {eos} max_new {max_new} forced {kind}: {got.tolist()} != {want.tolist()}")
    return bad


RULE_MUTANTS = ("latest_match", "accepted_plus_one", "accepted_minus_one", "no_extra_token", "eos_ignored", "pos_by_Q")


def mutant_failures(name):
    """-> the failures of checks 1 - 3 under the mutant (a subset of the invariance table: enough to catch every mutant that the loop can see)"""
    d = (lambda *a, **kw: draft(*a, mut=name, **kw)) if name == "latest_match" else draft
    a = accept if name == "latest_match" else (lambda *x, **kw: accept(*x, mut=name, **kw))
    return dict(draft=check_draft(d) if name == "latest_match" else [], accept=check_accept(a), invariance=check_invariance(d, a, cases=invariance_cases()[::5]))


# ------------------------------------------------------------------------------------------------------------------- chunk attention: cases
def chunk_cases():
    """Q in {1, 2, 5, 8} on three rows, one of which ends exactly at the capacity, on the 16-split route; Q = 8 across a 64-key trip (one workgroup per head walks
    the keys: no scratch); the 16-key group edge (pos 15 and 16); N * heads > 256: one split; a scratch that holds 5 of the 16 splits; scores up to +/-60"""
    out = []
    table = [(f"Q{Q}_N3_h2", dict(N=3, heads=2, Q=Q, pos=(0, 16, CAP - Q))) for Q in (1, 2, 5, 8)]
    table += [("Q8_N2_h2_noscratch_trip", dict(N=2, heads=2, Q=8, pos=(60, 0), scratch="none")), ("Q5_N2_h2_group_edge", dict(N=2, heads=2, Q=5, pos=(15, 16))),
              ("Q2_N5_h64", dict(N=5, heads=64, Q=2, pos=(3, 64, 65, CAP - 2, 17))), ("Q5_N1_h2_smallscratch", dict(N=1, heads=2, Q=5, pos=(CAP - 5,), scratch="small")),
              ("Q3_N2_h4_scores60", dict(N=2, heads=4, Q=3, pos=(CAP - 3, 40), qscale=25.0))]
    for name, kw in table:
        kw = {"scratch": "full", "qscale": 1.0, **kw}
        assert len(kw["pos"]) == kw["N"] and all(0 <= p and p + kw["Q"] <= CAP for p in kw["pos"])
        c = Case("decode_chunk", name, 0, **kw)
        c.launches = 2 if chunk_splits(c) > 1 else 1
        out.append(c)
    return out


def chunk_scratch_floats(case):
    """floats of scratch the case hands over: Q times what decode_attn's key split asks for ("full"), room for 5 splits ("small") or none"""
    nh = case.N * case.heads
    return {"full": nh * min(16, max(1, 256 // nh)) * 130 * case.Q, "small": nh * 5 * 130 * case.Q, "none": 0}[case.scratch]


def chunk_splits(case):
    return decode_splits(case.N, case.heads, chunk_scratch_floats(case) // case.Q)


def chunk_inputs(case):
    """ragged_decode_checks.inputs with Q step rows per sequence: the caches hold NaN beyond pos_n + Q - 1 and stale finite rows in the Q slots to be written"""
    g = fk._g(case)
    N, Q, D = case.N, case.Q, case.heads * HD
    qkv = torch.randn(N * Q, 3 * D, generator=g)
    qkv[:, :D] *= case.qscale
    ang = torch.rand(CAP, HD // 2, generator=g) * 6.28
    kc, vc = torch.randn(N, CAP, D, generator=g), torch.randn(N, CAP, D, generator=g)
    for n, p in enumerate(case.pos):
        kc[n, p + Q:], vc[n, p + Q:] = NAN, NAN
    return dict(qkv=qkv.to(BF), cos=ang.cos().float().contiguous(), sin=ang.sin().float().contiguous(), kc=kc.to(BF), vc=vc.to(BF), scale=HD ** -0.5)


def _chunk_row(case, inp, n, pos, mut=None, emu=None):
    """Q successive one-row decode_compute steps of sequence n from position `pos` -> (out [Q, D], kc, vc [1, CAP, D], exact masks)"""
    Q = case.Q
    cos, sin = inp["cos"], inp["sin"]
    if mut == "every_query_rotated_at_pos":
        cos, sin = cos.clone(), sin.clone()
        cos[pos:pos + Q], sin[pos:pos + Q] = cos[pos].clone(), sin[pos].clone()
    ref_k, ref_v = inp["kc"][n:n + 1].to(F64).clone(), inp["vc"][n:n + 1].to(F64).clone()      # what the step leaves: the new k rows unrounded (they take the bf16 bound)
    feed_k, feed_v = ref_k.clone(), ref_v.clone()                                             # what the next chunk token reads: the stored bf16 rows
    new = []
    for j in range(Q):
        one = Case("decode", f"{case.name}_row{n}_tok{j}", 0, N=1, heads=case.heads, pos=int(pos + j), scratch=case.scratch, qscale=case.qscale)
        sub = dict(inp, cos=cos, sin=sin, qkv=inp["qkv"][n * Q + j:n * Q + j + 1], kc=feed_k, vc=feed_v)
        step_mut = None
        if mut == "query_sees_next_chunk_key" and j + 1 < Q:   # slot pos + j + 1 already holds token j + 1's rows, and the key count takes it in
            nxt = Case("decode", "next", 0, N=1, heads=case.heads, pos=int(pos + j + 1), scratch=case.scratch, qscale=case.qscale)
            got_n, _ = decode_compute(nxt, dict(sub, qkv=inp["qkv"][n * Q + j + 1:n * Q + j + 2]), emu=emu)
            sub["kc"], sub["vc"] = feed_k.clone(), feed_v.clone()
            sub["kc"][:, pos + j + 1], sub["vc"][:, pos + j + 1] = got_n["kc"][:, pos + j + 1].to(BF).to(F64), got_n["vc"][:, pos + j + 1]
            step_mut = "key_pos_plus_1_included"
        got, exact = decode_compute(one, sub, mut=step_mut, emu=emu)
        new.append(got["out"])
        ref_k[:, pos + j], ref_v[:, pos + j] = got["kc"][:, pos + j], got["vc"][:, pos + j]
        if mut != "stale_slot_read":                           # (the mutant: later chunk tokens find the slots' old content)
            feed_k, feed_v = feed_k.clone(), feed_v.clone()
            feed_k[:, pos + j], feed_v[:, pos + j] = got["kc"][:, pos + j].to(BF).to(F64), got["vc"][:, pos + j]
    ek = torch.ones_like(ref_k, dtype=torch.bool)
    ek[:, pos:pos + Q] = False
    return dict(out=torch.cat(new, 0), kc=ref_k, vc=ref_v), dict(kc=ek, vc=torch.ones_like(ek))


OUTPUTS = ("out", "kc", "vc")


def chunk_compute(case, inp, positions=None, mut=None, emu=None):
    positions = case.pos if positions is None else positions
    rows = [_chunk_row(case, inp, n, positions[n], mut=mut, emu=emu) for n in range(case.N)]
    return {k: torch.cat([r[0][k] for r in rows], 0) for k in OUTPUTS}, {k: torch.cat([r[1][k] for r in rows], 0) for k in ("kc", "vc")}


@functools.lru_cache(maxsize=16)
def chunk_reference(case):
    """-> (inputs, fp64 reference {out [N * Q, D], kc, vc [N, CAP, D]}, per-element bounds); built once per case and shared: callers must not write to it"""
    inp = chunk_inputs(case)
    ref, exact = chunk_compute(case, inp)
    bounds = {}
    for k, r in ref.items():                                # the rule of forward_kernel_checks.reference for a bf16 output
        b = torch.where(r == 0, torch.zeros_like(r), torch.nan_to_num(fk.bf16_bound(r), nan=0.0))
        bounds[k] = torch.where(exact[k], torch.zeros_like(b), b) if k in exact else b
    return inp, ref, bounds


def chunk_ratios(got, ref, bounds):
    return {k: ratio(got[k], ref[k], bounds[k]) for k in OUTPUTS}


def chunk_emulation_ratios(case):
    inp, ref, bounds = chunk_reference(case)
    return chunk_ratios(chunk_compute(case, inp, emu=True)[0], ref, bounds)


def _swapped(pos):
    p = list(pos)
    for i in range(0, len(p) - 1, 2):
        p[i], p[i + 1] = p[i + 1], p[i]
    return tuple(p)


def chunk_mutant_names(case):
    m = []
    if case.Q >= 2:
        m.append("every_query_rotated_at_pos")
        if case.qscale == 1.0:                             # scores of sigma 25: the softmax is all but one-hot on some other key (forward_kernel_checks.decode_mutants)
            m += ["query_sees_next_chunk_key", "stale_slot_read"]
    if _swapped(case.pos) != tuple(case.pos) and all(p + case.Q <= CAP for p in _swapped(case.pos)):
        m.append("row_takes_neighbour_position")
    return m


def chunk_mutant(case, inp, name):
    if name == "row_takes_neighbour_position":
        return chunk_compute(case, inp, positions=_swapped(case.pos))[0]
    return chunk_compute(case, inp, mut=name)[0]


def chunk_mutant_ratios(case):
    inp, ref, bounds = chunk_reference(case)
    return {name: max(chunk_ratios(chunk_mutant(case, inp, name), ref, bounds).values()) for name in chunk_mutant_names(case)}
