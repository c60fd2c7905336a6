"""Beam search (llmseg_beam_step, generate(num_beams >= 2)): the rule restated on the CPU, an fp64 reference and an fp32 / integer emulation of
`llmseg_beam_step` on a case table, the per-score bound, and named mutants.  CPU only, no import of the HIP library.

The rule (per prompt; B beams; V >= 2 B):
  start      the live set is the prompt alone with score 0; the first pick reads ONE logits row, every later pick B rows.
  candidates (b, v) scores s_b + log_softmax(l_b)_v; the 2 B best are taken, score descending, equal scores by the smaller flat index b * V + v.
  walk       in rank order: an eos candidate of rank < B becomes a hypothesis (sum s, length g = step + 1, value s / g ** length_penalty), one of rank >= B
             is dropped, any other candidate becomes the next live beam until B are filled.  The pool keeps the B best hypotheses by value.
  done       the pool holds B hypotheses and (early_stopping, or the pool's worst value >= the step's best candidate score / (step + 1) ** length_penalty).
  end        every prompt done, or max_new_tokens picks made; a prompt that is not done adds its live beams (g = tokens generated); the result is the
             pool's best hypothesis.

The score bound.  llmseg_beam_step computes score = fl(s + fl(fl(l - l_max) - lse)) with lse = fp32(ln(S) - 40 ln 2), S the integer sum of
floor(expf(fl(l - l_max)) * 2^40).  Against exact arithmetic on the same bf16 logits and fp32 beam score:
  * three fp32 roundings, each at most half an ulp of its result: 2^-24 (|d| + |lp| + |score|), d = l - l_max, lp = d - lse;
  * the fp32 rounding of lse: 2^-24 |lse|;
  * ln(S): expf is accurate to one ulp (2^-23 relative on every term, hence on the sum), its argument was rounded (a relative error |d| 2^-24 of a term of
    weight exp(d) <= 1; x exp(-x) <= 0.37, so at most 2^-25 of the sum), and the floors remove less than V 2^-40 of a sum that is at least 1; a
    relative error of S is an absolute error of ln(S); the fp64 logarithm adds nothing visible.
bound = 2^-24 (|d| + |lse| + |lp| + |score|) + 2^-23 + 2^-25 + V 2^-40."""
import dataclasses
import functools
import math

import torch

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
FB = 40
LN2 = 0.69314718055994530942
SENTINEL = -7                     # what src_out holds before the call: entries the kernel must not write
LD_SRC = 24                       # row stride of the tables in the cases (the table rows are 20 wide: the slack must stay untouched)
W_SRC = 20
LOOP_MUTANTS = ("eos_rank_ge_B_kept", "length_without_eos", "ties_by_larger_index", "done_against_best_hypothesis")
TABLE_MUTANTS = ("src_row_from_own_slot", "new_key_owner_is_child_row", "prompt_keys_from_own_row")


# ------------------------------------------------------------------------------------------------------------------------------- the rule
def rank_candidates(cand, K, mut=None):
    """cand [beams_in, V] scores -> the flat indices of the K best, score descending, equal scores by the smaller flat index"""
    flat = cand.reshape(-1)
    if mut == "ties_by_larger_index":
        order = torch.sort(flat.flip(0), descending=True, stable=True).indices
        return (flat.numel() - 1 - order[:K]).tolist()
    return torch.sort(flat, descending=True, stable=True).indices[:K].tolist()


def walk(cand, B, eos, mut=None):
    """one pick on candidate scores [beams_in, V] -> dict(tokens, parents, scores: the B next live beams; fin: [(parent, score)] in rank order; best: the
    best candidate's score; ranked: [(b, v, score)] of the 2 B best; gap: the smallest difference between neighbours among the 2 B + 1 best)"""
    V = cand.shape[1]
    idx = rank_candidates(cand, min(2 * B + 1, cand.numel()), mut)
    flat = cand.reshape(-1)
    sc = [float(flat[i]) for i in idx]
    gap = min((sc[i] - sc[i + 1] for i in range(len(sc) - 1)), default=math.inf)
    tokens, parents, scores, fin, ranked = [], [], [], [], []
    for k, i in enumerate(idx[:2 * B]):
        b, v = divmod(i, V)
        ranked.append((b, v, sc[k]))
        if eos is not None and v == eos:
            if k < B or mut == "eos_rank_ge_B_kept":
                fin.append((b, sc[k]))
        elif len(tokens) < B:
            tokens.append(v)
            parents.append(b)
            scores.append(sc[k])
    return dict(tokens=tokens, parents=parents, scores=scores, fin=fin, best=sc[0], ranked=ranked, gap=gap)


class BeamPrompt:
    """the rule's state for one prompt: feed it the log-probabilities of its live beams, one pick at a time"""

    def __init__(self, B, eos, length_penalty=1.0, early_stopping=False, mut=None):
        self.B, self.eos, self.lp, self.early, self.mut = B, eos, float(length_penalty), early_stopping, mut
        self.seqs, self.scores = [[]], [0.0]
        self.pool = []                # (value, tokens)
        self.done = False
        self.steps = 0
        self.picks = []

    def _add(self, value, tokens):
        if len(self.pool) < self.B:
            self.pool.append((value, tokens))
        elif value > min(h[0] for h in self.pool):
            self.pool[min(range(len(self.pool)), key=lambda i: self.pool[i][0])] = (value, tokens)

    def step(self, logp):
        """logp fp64 [len(self.seqs), V]: log_softmax of each live beam's logits -> the pick (see `walk`)"""
        assert not self.done and logp.shape[0] == len(self.seqs)
        cand = torch.tensor(self.scores, dtype=F64)[:, None] + logp.to(F64)
        pick = walk(cand, self.B, self.eos, self.mut)
        g = self.steps + 1
        for b, s in pick["fin"]:
            glen = g - 1 if self.mut == "length_without_eos" else g
            self._add(s / max(glen, 1) ** self.lp, self.seqs[b] + [self.eos])
        self.seqs = [self.seqs[b] + [v] for b, v in zip(pick["parents"], pick["tokens"])]
        self.scores = pick["scores"]
        self.steps = g
        if len(self.pool) >= self.B:
            ref = max(h[0] for h in self.pool) if self.mut == "done_against_best_hypothesis" else min(h[0] for h in self.pool)
            self.done = self.early or ref >= pick["best"] / g ** self.lp
        self.picks.append(pick)
        return pick

    def result(self):
        """-> (value, tokens) of the best hypothesis; a prompt that is not done adds its live beams first"""
        pool = list(self.pool)
        if not self.done:
            saved, self.pool = self.pool, pool
            for s, toks in zip(self.scores, self.seqs):
                self._add(s / self.steps ** self.lp, toks)
            pool, self.pool = self.pool, saved
        return max(pool, key=lambda h: h[0])


def search(logits_fn, B, eos, max_new_tokens, length_penalty=1.0, early_stopping=False, mut=None):
    """the loop for ONE prompt: logits_fn(list of generated-token lists) -> fp32 / fp64 logits [len, V] of their next token -> (BeamPrompt, (value, tokens))"""
    p = BeamPrompt(B, eos, length_penalty, early_stopping, mut)
    while not p.done and p.steps < max_new_tokens:
        lg = logits_fn(p.seqs).to(F64)
        p.step(lg - torch.logsumexp(lg, -1, keepdim=True))
    return p, p.result()


# ----------------------------------------------------------------------------------------------------------------- llmseg_beam_step: cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    N: int
    B: int
    V: int
    beams_in: int                 # 1 or B
    eos: str = "none"             # none | rank0 | rankB-1 | rankB | every_beam
    shape: str = "mixed"          # mixed | identity | allsame | perm: what the parents of prompt 0 are
    done: tuple = ()              # prompts that are done
    neg_inf: bool = False
    ties: bool = False
    seed: int = 0


def cases():
    c = [
        Case("V2B_B2_first", 1, 2, 4, 1), Case("V2B_B3", 3, 3, 6, 3, eos="rank0"), Case("V2B1_B4", 1, 4, 9, 4, eos="rankB"), Case("V2B_B16", 1, 16, 32, 16),
        Case("V2B1_B16_first", 3, 16, 33, 1, eos="rankB-1"),
        Case("V1000_B2", 3, 2, 1000, 2, eos="rankB-1"), Case("V1000_B3_first", 3, 3, 1000, 1, eos="rank0"), Case("V1000_B4_everybeam", 1, 4, 1000, 4, eos="every_beam"),
        Case("V1000_B16", 1, 16, 1000, 16, eos="rankB"), Case("V1000_B4_identity", 3, 4, 1000, 4, shape="identity"),
        Case("V1000_B4_allsame", 1, 4, 1000, 4, shape="allsame"), Case("V1000_B4_perm", 3, 4, 1000, 4, shape="perm", eos="rankB"),
        Case("V1000_B3_done", 3, 3, 1000, 3, done=(1,), eos="rank0"), Case("V1000_B2_neginf", 1, 2, 1000, 2, neg_inf=True),
        Case("V9_B4_neginf", 3, 4, 9, 4, neg_inf=True), Case("V1000_B3_ties", 3, 3, 1000, 3, ties=True), Case("V1000_B4_ties_first", 1, 4, 1000, 1, ties=True, eos="rank0"),
        Case("V32000_B4", 1, 4, 32000, 4, eos="rankB-1"), Case("V32000_B16_perm", 1, 16, 32000, 16, shape="perm"), Case("V32000_B2_first", 3, 2, 32000, 1),
        Case("V32003_B3", 3, 3, 32003, 3, eos="rankB", done=(0,)), Case("V32003_B16_identity", 1, 16, 32003, 16, shape="identity", eos="every_beam"),
        Case("V32003_B4_first_neginf", 1, 4, 32003, 1, neg_inf=True, eos="rank0"),
    ]
    assert len({x.name for x in c}) == len(c)
    return c


def _raw_inputs(case):
    g = torch.Generator().manual_seed(1000 + case.seed + sum(map(ord, case.name)))
    N, B, V, bi = case.N, case.B, case.V, case.beams_in
    rows, R = N * bi, N * B
    K = min(2 * B + 2, V)
    logits = (torch.randn(rows, V, generator=g) * 1.5).clamp_(max=2.75)
    shaped = case.shape != "mixed"
    plant = []
    for r in range(rows):
        if V <= 64:                                          # every entry of the row distinct
            allv = 0.25 * torch.randperm(V, generator=g).double()
            logits[r] = allv.float()
            pos = allv.argsort(descending=True)[:K]
            vals = allv[pos].clone()
        else:                                                # K planted values above everything else of the row, the best first
            pos = torch.randperm(V, generator=g)[:K]
            if case.eos == "every_beam":                     # one token id is the best continuation of every beam
                pos = torch.cat([torch.tensor([V // 3]), pos[pos != V // 3][:K - 1]])
            vals = (3.0 + (0.0625 if shaped else 0.25) * torch.randperm(K, generator=g).double()).sort(descending=True).values
            if shaped:
                vals[0] = 12.0                               # one dominant candidate per beam
        if case.ties:                                        # the best two of the row are equal, and so are the next three
            vals[1] = vals[0]
            if K >= 5:
                vals[3] = vals[2]
                vals[4] = vals[2]
        logits[r, pos] = vals.float()
        plant.append(pos)
        if case.neg_inf:
            kill = torch.rand(V, generator=g) < (0.3 if V > 64 else 0.0)
            kill[pos[:2 * B]] = False
            if V <= 64:
                kill[pos[2 * B:]] = True                     # exactly 2 B finite logits are left
            logits[r, kill] = -math.inf
    logits = logits.to(BF)
    if bi == 1:
        scores = torch.zeros(rows)
    else:
        scores = -(torch.rand(N, B, generator=g) * 2.0)
        b = torch.arange(B).float()
        if case.shape == "identity":
            scores = (-0.25 * b)[None, :].expand(N, B) - torch.rand(N, 1, generator=g) + 0.03 * torch.rand(N, B, generator=g)
        elif case.shape == "perm":
            scores = (-0.25 * (B - 1 - b))[None, :].expand(N, B) - torch.rand(N, 1, generator=g) + 0.03 * torch.rand(N, B, generator=g)
        elif case.shape == "allsame":
            scores = torch.full((N, B), -100.0)
            scores[:, 1 % B] = -0.5
        scores = scores.reshape(-1).contiguous().float()
    done = torch.zeros(N, dtype=torch.int32)
    for n in case.done:
        done[n] = 1
    src_in = torch.randint(0, R, (R, LD_SRC), generator=g, dtype=torch.int32)
    pos_rows = torch.randint(1, W_SRC + 1, (R,), generator=g, dtype=torch.int32)
    pos_rows[0] = W_SRC
    if R > 1:
        pos_rows[1] = 1
    return dict(logits=logits, beam_scores=scores, done=done, src_in=src_in, pos_rows=pos_rows, pad=V - 1, plant=plant)


def exact_scores(inp, case):
    """fp64 candidate scores [N, beams_in, V] and the per-score bound of the module docstring"""
    l = inp["logits"].to(F64).view(case.N, case.beams_in, case.V)
    s = inp["beam_scores"].to(F64).view(case.N, case.beams_in, 1)
    lmax = l.max(-1, keepdim=True).values
    d = l - lmax
    lse = torch.log(torch.exp(d).sum(-1, keepdim=True))
    lp = d - lse
    score = s + lp
    bound = 2.0 ** -24 * (d.abs() + lse.abs() + lp.abs() + score.abs()) + 2.0 ** -23 + 2.0 ** -25 + case.V * 2.0 ** -40
    return score, torch.nan_to_num(bound, nan=0.0, posinf=0.0)


def emulated_scores(inp, case):
    """the kernel's arithmetic, step by step in fp32 and integers -> fp32 scores [N, beams_in, V]"""
    l = inp["logits"].to(F32).view(case.N, case.beams_in, case.V)
    s = inp["beam_scores"].to(F32).view(case.N, case.beams_in, 1)
    lmax = l.max(-1, keepdim=True).values
    d = l - lmax
    e = torch.exp(d)
    mass = torch.floor(e.to(F64) * 2.0 ** FB).to(torch.int64)
    S = mass.sum(-1, keepdim=True)
    lse = (torch.log(S.to(F64)) - FB * LN2).to(F32)
    return s + (d - lse)


def _step(case, inp, eos, cand, mut=None):
    """the outputs of llmseg_beam_step from candidate scores [N, beams_in, V] (fp64: the reference; fp32: the emulation)"""
    N, B, bi = case.N, case.B, case.beams_in
    R = N * B
    out = dict(next_token=torch.zeros(R, dtype=torch.int64), parent=torch.zeros(R, dtype=torch.int32), next_scores=torch.zeros(R, dtype=F64),
               step_best=torch.zeros(N, dtype=F64), fin_count=torch.zeros(N, dtype=torch.int32), fin_parent=torch.full((N, B), SENTINEL, dtype=torch.int32),
               fin_score=torch.zeros((N, B), dtype=F64), src_out=torch.full((R, LD_SRC), SENTINEL, dtype=torch.int32), gap=[math.inf] * N, ranked=[None] * N)
    for n in range(N):
        if int(inp["done"][n]):
            for i in range(B):
                j = min(i, bi - 1)
                out["next_token"][n * B + i], out["parent"][n * B + i] = inp["pad"], j
                out["next_scores"][n * B + i] = float(inp["beam_scores"][n * bi + j])
        else:
            pick = walk(cand[n].to(F64), B, eos, mut if mut in LOOP_MUTANTS else None)
            out["next_token"][n * B:(n + 1) * B] = torch.tensor(pick["tokens"])
            out["parent"][n * B:(n + 1) * B] = torch.tensor(pick["parents"], dtype=torch.int32)
            out["next_scores"][n * B:(n + 1) * B] = torch.tensor(pick["scores"], dtype=F64)
            out["step_best"][n] = pick["best"]
            out["fin_count"][n] = len(pick["fin"])
            for k, (b, s) in enumerate(pick["fin"][:B]):
                out["fin_parent"][n, k], out["fin_score"][n, k] = b, s
            out["gap"][n], out["ranked"][n] = pick["gap"], pick["ranked"]
        for i in range(B):
            r = n * B + i
            j = int(out["parent"][r])
            p = int(inp["pos_rows"][r])
            if bi == 1:
                out["src_out"][r, :p] = r if mut == "prompt_keys_from_own_row" else n * B
            else:
                out["src_out"][r, :p - 1] = inp["src_in"][r if mut == "src_row_from_own_slot" else n * B + j, :p - 1]
                out["src_out"][r, p - 1] = r if mut == "new_key_owner_is_child_row" else n * B + j
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (inputs with `eos` resolved, fp64 reference outputs, per-score bound [N, beams_in, V]); built once per case, callers must not write to it"""
    inp = _raw_inputs(case)
    score, bound = exact_scores(inp, case)
    eos = None
    if case.eos != "none":
        live = next(n for n in range(case.N) if n not in case.done)
        ranked = walk(score[live], case.B, None)["ranked"]
        if case.eos == "every_beam":
            eos = case.V // 3
        else:
            eos = ranked[{"rank0": 0, "rankB-1": case.B - 1, "rankB": case.B}[case.eos]][1]
    inp = dict(inp, eos=eos)
    return inp, _step(case, inp, eos, score), bound


def emulation(case, mut=None):
    inp, _, _ = reference(case)
    return _step(case, inp, inp["eos"], emulated_scores(inp, case), mut)


def mutant(case, mut):
    """the fp64 reference with one named defect"""
    inp, _, _ = reference(case)
    score, _ = exact_scores(inp, case)
    return _step(case, inp, inp["eos"], score, mut)


def bound_of(case, n, parent, token):
    return float(reference(case)[2][n, parent, token])


def compare(case, got, exact_only=False):
    """got (tensors on the CPU, llmseg_beam_step's outputs + src_out) against the fp64 reference -> (list of mismatches, worst score error / bound)"""
    inp, ref, bound = reference(case)
    N, B, bi = case.N, case.B, case.beams_in
    bad, worst = [], 0.0
    for k in ("next_token", "parent", "fin_count", "src_out"):
        if not torch.equal(got[k].to(ref[k].dtype).view_as(ref[k]), ref[k]):
            bad.append(k)
    for n in range(N):
        c = int(ref["fin_count"][n])
        if not torch.equal(got["fin_parent"].view(N, B)[n, :c].to(torch.int32), ref["fin_parent"][n, :c]):
            bad.append(f"fin_parent[{n}]")
        if int(inp["done"][n]):
            if not torch.equal(got["next_scores"].view(N, B)[n].to(F64), ref["next_scores"].view(N, B)[n]):
                bad.append(f"next_scores of the done prompt {n}")
            continue
        if exact_only:
            continue
        items = [(float(got["step_best"][n]), float(ref["step_best"][n]), ref["ranked"][n][0][:2])]
        for i in range(B):
            r = n * B + i
            items.append((float(got["next_scores"][r]), float(ref["next_scores"][r]), (int(ref["parent"][r]), int(ref["next_token"][r]))))
        for k in range(c):
            items.append((float(got["fin_score"].view(N, B)[n, k]), float(ref["fin_score"][n, k]), (int(ref["fin_parent"][n, k]), inp["eos"])))
        for g_, r_, (b, v) in items:
            bd = float(bound[n, b, v])
            ratio = abs(g_ - r_) / bd if bd > 0 else (0.0 if g_ == r_ else math.inf)
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                bad.append(f"score of ({n}, {b}, {v}): {g_!r} vs {r_!r}, bound {bd:.3e}")
    return bad, worst


def gap_condition(case):
    """-> (smallest NON-ZERO gap among the 2 B + 1 best fp64 scores of a live prompt) / (16 x the largest bound among them); zero gaps only in tie cases"""
    inp, ref, bound = reference(case)
    worst, zero = math.inf, 0
    for n in range(case.N):
        if int(inp["done"][n]):
            continue
        score, _ = exact_scores(inp, case)
        idx = rank_candidates(score[n], min(2 * case.B + 1, score[n].numel()))
        sc = [float(score[n].reshape(-1)[i]) for i in idx]
        bd = max(float(bound[n].reshape(-1)[i]) for i in idx)
        for a, b in zip(sc, sc[1:]):
            if not math.isfinite(a):
                continue
            if a == b:
                zero += 1
            elif math.isfinite(b):
                worst = min(worst, (a - b) / (16 * bd))
    return worst, zero
