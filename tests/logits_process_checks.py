"""Logits processors (llmseg_logits_process, generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=)): the rule of
include/llmseg_hip.h restated in plain torch on the CPU, and the case table of the kernel tests.  Every comparison built on this file is bit for bit: the rule is
exact arithmetic on bf16 / fp32 values, there is no tolerance anywhere.

The rule, per row: history h (a list of ints: the prompt ids as given, then every emitted token), logits l (bf16 [V]):
  1. every DISTINCT t of h with 0 <= t < V, once: l_t <- bf16(fl32(l_t) * fl32(theta)) if l_t < 0 else bf16(fl32(l_t) / fl32(theta));
  2. g >= 1 and len >= g: every j in [0, len - g] with h[j : j + g - 1] == h[len - g + 1 :] bans h[j + g - 1] (if in [0, V));
  3. ban_token gets -inf;  4. every id of the suppress list gets -inf.
"""
import collections
import functools

import torch

BF = torch.bfloat16
INF = float("inf")
CAP = 4096                           # == LLMSEG_LOGITS_HIST_CAP: the largest history a row may hold
IMAGE = -200                         # the <image> placeholder: stays in the history, skipped by the rule
SENTINEL = -7777                     # fills every history cell that holds no token


# ------------------------------------------------------------------------------------------------------------------------------ the rule
def penalise(l, theta):
    """the explicit formula on a bf16 tensor: fp32 product / true fp32 division, rounded to nearest even"""
    x = l.float()
    th = torch.tensor(float(theta), dtype=torch.float32)
    return torch.where(x < 0, x * th, x / th).to(BF)


def banned_by_ngram(h, g):
    """the tokens (any int, in range or not) that would complete an n-gram already in h"""
    n = len(h)
    if g < 1 or n < g:
        return set()
    tail = h[n - g + 1:]
    out = set()
    for j in range(n - g + 1):
        if h[j:j + g - 1] == tail:
            out.add(h[j + g - 1])
    return out


def rule(l, h, theta=1.0, g=0, ban=None, suppress=None):
    """l bf16 [V], h list of ints -> (processed bf16 [V], the set of ids the rule may have rewritten)"""
    V = l.numel()
    out = l.clone()
    touched = set()
    if theta != 1.0:
        ids = sorted({t for t in h if 0 <= t < V})
        if ids:
            idx = torch.tensor(ids, dtype=torch.int64)
            out[idx] = penalise(l[idx], theta)
        touched |= set(ids)
    neg = {t for t in banned_by_ngram(h, g) if 0 <= t < V}
    if ban is not None and ban >= 0:
        neg.add(int(ban))
    if suppress is not None:
        neg |= {int(t) for t in suppress}
    for t in neg:
        out[t] = -INF
    return out, touched | neg


def rule_rows(logits, hists, theta=1.0, g=0, ban=None, suppress=None):
    """logits bf16 [N, V], hists = one list per row -> processed bf16 [N, V]"""
    return torch.stack([rule(logits[n], hists[n], theta, g, ban, suppress)[0] for n in range(logits.shape[0])])


# ---------------------------------------------------------------------------------------------------------------------------- the table
Case = collections.namedtuple("Case", "name V N kind cap theta g append ban_mode sup_mode ldl_pad seed")
VS = (33, 4099, 32003)
NS = (1, 3, 8)
KINDS = ("mix", "same", "ends", "period", "oob")
THETAS = (0.5, 1.0, 1.2, 3.0)
GS = (1, 2, 3, 4, 0)
SPECIAL = (2.5, -1.75, 0.0, -0.0, INF, -INF)        # what the logits of the history's tokens are: every class the formula treats differently


def length_set(cap, g):
    """the history lengths (before an append) the rows of a case rotate through"""
    out = []
    for x in (0, 1, max(g - 1, 0), g, 255, 256, 257, 1025, cap, 64, 1024):      # (the last two: eight distinct lengths whatever g is)
        if x <= cap and x not in out:
            out.append(x)
    return out


def cases():
    out = []
    i = 0
    for V in VS:
        for N in NS:
            for kind in KINDS:
                theta = THETAS[i % 4]
                if kind == "ends":                             # the duplicate at both ends of a full history must be penalised: a penalty that is on
                    theta = (0.5, 1.2, 3.0)[i % 3]
                g = GS[(i // 5 + i) % 5]                       # (i % 5 is the kind: every kind meets every g)
                cap = CAP if kind == "ends" or (i // 5) % 3 != 1 else 1030
                append = i % 3 != 0
                ban_mode = (i // 3) % 4                        # 0: a token of the history, 2: V - 1, odd: none (-1)
                sup_mode = (i // 2) % 3                        # 0: none, 1: a list with a duplicate id, 2: a list that holds a penalised id
                if theta == 1.0 and g == 0 and ban_mode % 2 and sup_mode == 0:
                    sup_mode = 1                               # theta = 1 is tested with other controls on
                name = f"V{V}_N{N}_{kind}_cap{cap}_th{theta}_g{g}_{'app' if append else 'noapp'}_ban{ban_mode}_sup{sup_mode}"
                out.append(Case(name, V, N, kind, cap, theta, g, append, ban_mode, sup_mode, 5 + i % 3, 1000 + i))
                i += 1
    return out


def _alphabet(V, gen):
    """six distinct in-range ids: the two ends of the vocabulary and four others"""
    ids = {0, V - 1}
    while len(ids) < 6:
        ids.add(int(torch.randint(1, V - 1, (1,), generator=gen)))
    rest = sorted(ids - {0, V - 1})
    return [rest[0], 0, rest[1], V - 1, rest[2], rest[3]]


def _history(kind, n, alpha, V, g, gen):
    """n ids of the given kind"""
    oob = [IMAGE, V + 3]
    if n == 0:
        return []
    if kind == "same":
        return [alpha[0]] * n
    if kind == "period":                                       # overlapping matches, and the match that overlaps the suffix itself
        return [alpha[k % 3] for k in range(n)]
    if kind == "ends":                                         # alpha[0] at positions 0 and n - 1 only
        body = [alpha[1 + int(k)] for k in torch.randint(0, 5, (n,), generator=gen)]
        body[0] = body[-1] = alpha[0]
        return body
    pool = alpha + oob if kind == "mix" else [alpha[0], alpha[1]] + oob + oob      # "oob": half the history lies outside [0, V)
    h = [pool[int(k)] for k in torch.randint(0, len(pool), (n,), generator=gen)]
    if g >= 2 and n >= 2 * g:                                  # plant one match of the last g - 1 ids, so that every g of the table bans something
        p = int(torch.randint(0, n - 2 * g + 2, (1,), generator=gen))
        h[n - g + 1:] = h[p:p + g - 1]
    return h


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict: logits bf16 [N + 1, V + ldl_pad] (row N and the pad columns are decoys), hists (lists, before the append), append (list | None), lens, theta, g,
    ban (int | None), suppress (list | None)"""
    gen = torch.Generator().manual_seed(case.seed)
    V, N = case.V, case.N
    alpha = _alphabet(V, gen)
    logits = (3.0 * torch.randn(N + 1, V + case.ldl_pad, generator=gen)).to(BF)
    ls = [x for x in length_set(case.cap, case.g) if not (case.kind == "ends" and x == case.cap)]      # "ends": the full history is row 0's
    lens, hists, append = [], [], ([] if case.append else None)
    for r in range(N):
        n = ls[(case.seed + r) % len(ls)]
        if case.kind == "ends" and r == 0:                     # the full history: duplicates at 0 and cap - 1, the last one arriving as the append where there is one
            n = case.cap - 1 if case.append else case.cap
        h = _history(case.kind, n + (1 if case.kind == "ends" and r == 0 and case.append else 0), alpha, V, case.g, gen)
        if case.append:
            if case.kind == "ends" and r == 0:
                append.append(h.pop())
            elif case.kind in ("same", "period"):
                append.append(_history(case.kind, n + 1, alpha, V, case.g, gen)[-1])
            else:
                append.append((alpha + [IMAGE, V + 3])[int(torch.randint(0, 8, (1,), generator=gen))])
        lens.append(n)
        hists.append(h)
        for k, t in enumerate(alpha):
            logits[r, t] = SPECIAL[(k + r) % 6]
    if case.kind == "ends":
        logits[0, alpha[0]] = 2.5                              # penalised twice it would be 2.5 / theta^2: never the same bf16 as 2.5 / theta for the table's theta
    ban = alpha[2] if case.ban_mode == 0 else V - 1 if case.ban_mode == 2 else None
    free = [int(t) for t in torch.randint(0, V, (2,), generator=gen)]
    suppress = None if case.sup_mode == 0 else [free[0], free[1], free[0]] if case.sup_mode == 1 else [alpha[1], free[0]]
    return dict(logits=logits, hists=hists, append=append, lens=lens, theta=case.theta, g=case.g, ban=ban, suppress=suppress, alpha=alpha)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict: logits bf16 [N + 1, V + ldl_pad] after the call (decoys unchanged), hists after the append, lens after the append, touched = per row the ids the rule
    may have rewritten"""
    inp = inputs(case)
    V, N = case.V, case.N
    out = inp["logits"].clone()
    hists, lens, touched = [], [], []
    for r in range(N):
        h = list(inp["hists"][r])
        if inp["append"] is not None and len(h) < case.cap:    # a full row drops the append
            h.append(inp["append"][r])
        row, t = rule(inp["logits"][r, :V], h, inp["theta"], inp["g"], inp["ban"], inp["suppress"])
        out[r, :V] = row
        hists.append(h)
        lens.append(len(h))
        touched.append(t)
    return dict(logits=out, hists=hists, lens=lens, touched=touched)


def hist_tensor(hists, cap):
    """lists -> int64 [N, cap], SENTINEL where a row holds no token"""
    t = torch.full((len(hists), cap), SENTINEL, dtype=torch.int64)
    for r, h in enumerate(hists):
        t[r, :len(h)] = torch.tensor(h, dtype=torch.int64)
    return t


# the n-gram pin of the issue: (history, g, banned set), as the installed transformers gives them
NGRAM_PIN = ([([1, 2, 3, 1, 2, 3, 1, 2], 1, {1, 2, 3}), ([1, 2, 3, 1, 2, 3, 1, 2], 2, {3}), ([1, 2, 3, 1, 2, 3, 1, 2], 3, {3}), ([1, 2, 3, 1, 2, 3, 1, 2], 4, {3}),
              ([1, 2, 3, 1, 2, 3, 1, 2], 8, set()), ([1, 2, 3, 1, 2, 3, 1, 2], 9, set())] + [([4] * 8, g, {4}) for g in range(1, 9)] + [([4] * 8, 9, set())] +
             [([1, 2, 9, 9, 1, 2, 7, 1], 2, {2}), ([1, 2, 9, 9, 1, 2, 7, 1], 3, set())])
