"""Sampling (llmseg_amd/csrc/sample.hip, generate(do_sample=True)): an fp64 restatement of the public rule, hand-built rows, a case table, bounds derived from the
kernel's arithmetic, an fp32 / integer emulation of the kernel and named mutants the bounds must reject.  Everything here runs on the CPU (no import of the HIP
library); tests/test_sampling_cpu.py pins the restatement (against the installed transformers warpers and on hand-built rows), proves that the emulation stays at
<= EMU_MAX of the bounds and that every mutant exceeds them on several cases; tests/test_sampling_gpu.py holds the kernel to the same checks.

The rule, per row (include/llmseg_hip.h): z = l / T;  K1 = {z >= k-th largest z} (1 <= k < V; all ties kept; -inf never kept beside a larger logit);  q = softmax of z
over K1;  m_i = sum of q_j over {j in K1: z_j <= z_i};  K2 = {i in K1: m_i > 1 - p} (p < 1), K1 (p = 1);  r = q / sum_K2 q;  the token is the smallest i in K2, in
token-id order, with C_i = sum_{j <= i} r_j > u, the largest index of K2 if none;  logprob = ln r_token.

What the kernel rounds, with d_j = (l_j - l_max) / T <= 0 and e_j = exp(d_j):
    d^ = fl(fl(l_j - l_max) / fl(T)): three fp32 roundings, |d^ - d| <= 3 * 2^-24 |d|;   e^ = expf(d^) (<= 2 ulp);   mass_j = floor(e^ * 2^40), an integer.
    => |mass_j / 2^40 - e_j| <= err_j = e_j (|d_j| 2^-22 + 2^-22) + 2^-39.
    (3 * 2^-24 < 2^-22 and 2 ulp = 2^-23 < 2^-22; the floor loses < 2^-40 and ALWAYS loses it on a weight below 2^-40, a deterministic error that sits at the
    edge of its bound: the term is doubled so that the emulation stays at <= EMU_MAX of every bound, as the house rule for emulations asks.)
Every sum is an integer sum (exact), so with E(A) = sum_{j in A} err_j and S(A) = sum_{j in A} e_j a ratio of sums over subsets of A moves by <= 2 E(A) / S(A):
    delta_p = 2 E(K1) / S(K1) + 2^-24 + 2^-50      (a cumulative mass m_i against 1 - p; 2^-24: p itself is rounded to fp32; 2^-50: the threshold is formed in fp64)
    delta_u = 2 E(K2) / S(K2) + 2^-40 / S(K2) + 2^-50      (a CDF position C_i against u; the threshold u * S2 is floored to an integer)
    probs:   |r^_i - r_i| <= (err_i + r_i E(K2)) / S(K2) + 2^-23 r_i + 2^-60            (the fp32 store)
    logprob: |ln r^ - ln r| <= 1.01 (err_t / e_t + E(K2) / S(K2)) + 2^-23 max(1, |ln r|)    (where err_t / e_t <= 0.1)"""
import collections
import functools
import math

import torch

from tests.backward_kernel_checks import EMU_MAX, MUT_MIN  # noqa: F401  (re-exported to the two test files)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
INF = float("inf")
FB = 40                              # fixed-point bits of a mass (V <= 2^22)
REG_MAX = 32768                      # V <= REG_MAX: the row lives in registers; above: re-read from memory on every pass
U_MAX = 1.0 - 2.0 ** -24             # the largest fp32 below 1


# ------------------------------------------------------------------------------------------------------------------------------ the rule, fp64
def _canon(l):
    """bf16 row -> fp64 values with -0 folded into +0 (one tie group)"""
    return l.to(F64) + 0.0


def rule(l, T, k, p, shift=0.0):
    """fp64 restatement of the rule for one bf16 row -> dict(K1, K2 bool [V]; m, r, C fp64 [V]).  shift moves the top-p threshold: K2 = {m > 1 - p + shift}
    (p < 1 only; p = 1 keeps K1 whatever the shift)."""
    lv = _canon(l)
    V = lv.numel()
    z = lv / T
    K1 = torch.ones(V, dtype=torch.bool)
    if 1 <= k < V:
        K1 = z >= torch.topk(z, k).values[-1]
    if bool((z > -INF).any()):
        K1 = K1 & (z > -INF)
    e = torch.where(K1, torch.exp(z - z[K1].max()), torch.zeros_like(z))
    q = e / e.sum()
    order = torch.argsort(z)                                  # ascending z: ascending q
    zs, cs = z[order], torch.cumsum(q[order], 0)
    m = cs[torch.searchsorted(zs, z, right=True) - 1]          # cumulative mass up to and including the whole tie group of i
    K2 = K1 & (m > 1.0 - p + shift) if p < 1 else K1.clone()
    r = torch.where(K2, q, torch.zeros_like(q))
    r = r / r.sum()
    return dict(K1=K1, K2=K2, m=m, r=r, C=torch.cumsum(r, 0), e=e, d=(lv - lv[K1].max()) / T)


def draw(ref, u):
    """the token of the rule for the uniform u"""
    hit = (ref["C"] > u) & ref["K2"]
    return int(hit.nonzero()[0]) if bool(hit.any()) else int(ref["K2"].nonzero()[-1])


def bounds(ref):
    """-> dict(dp, du floats; probs fp64 [V]; logprob fp64 [V]) from the docstring's formulas, all computed from the fp64 reference alone"""
    e, d, K1, K2, r = ref["e"], ref["d"], ref["K1"], ref["K2"], ref["r"]
    err = e * (d.abs().nan_to_num(posinf=0.0) * 2.0 ** -22 + 2.0 ** -22) + 2.0 ** (1 - FB)
    E1, S1 = float(err[K1].sum()), float(e[K1].sum())
    E2, S2 = float(err[K2].sum()), float(e[K2].sum())
    lnr = torch.log(r)
    return dict(dp=2 * E1 / S1 + 2.0 ** -24 + 2.0 ** -50, du=2 * E2 / S2 + 2.0 ** -FB / S2 + 2.0 ** -50,
                probs=(err + r * E2) / S2 + 2.0 ** -23 * r + 2.0 ** -60,
                logprob=1.01 * (err / e + E2 / S2) + 2.0 ** -23 * lnr.abs().clamp(min=1.0))


# ------------------------------------------------------------------------------------------------------------------------------ hand-built rows
# (what the row shows, logits, T, k, p, the kept set K2 written out by hand)
HAND = (
    ("top-k keeps every tie at the k-th value", [1.0, 3.0, 2.0, 2.0, 0.0, 2.0], 1.0, 2, 1.0, [1, 2, 3, 5]),
    ("k = 1 with a tied maximum keeps both", [5.0, 1.0, 5.0], 1.0, 1, 1.0, [0, 2]),
    ("k >= V keeps everything", [0.5, -1.0, 2.0], 1.0, 3, 1.0, [0, 1, 2]),
    ("-inf is never kept beside a finite logit", [-INF, 0.0, -INF, 1.0], 1.0, 0, 1.0, [1, 3]),
    ("all equal: one tie group, kept whole at any p", [0.25] * 5, 1.0, 0, 1e-3, [0, 1, 2, 3, 4]),
    # the second group's m = (1 + e) / (1 + e + 2 e^8) = 6e-4 <= 1 - p
    ("p small keeps only the top group", [0.0, 8.0, 8.0, 1.0], 1.0, 0, 1e-6, [1, 2]),
    # z = (0, 0, 0, 1): the three equal tokens hold 3 / (3 + e) = 0.525 of the mass, 0.175 each; 1 - p = 0.2 falls INSIDE the group (HF drops one member,
    # whichever torch.sort puts first): the whole group stays
    ("a tie group straddling the p boundary is kept whole", [0.0, 0.0, 0.0, 16.0], 16.0, 0, 0.8, [0, 1, 2, 3]),
    # the same row with 1 - p = 0.6 above the group's 0.525: dropped whole
    ("a tie group below the p boundary is dropped whole", [0.0, 0.0, 0.0, 16.0], 16.0, 0, 0.4, [3]),
    # z = (100, 125, 50): m of token 0 is e^-25
    ("temperature first: T = 0.01 makes the maximum the only survivor of p = 0.99", [1.0, 1.25, 0.5], 0.01, 0, 0.99, [1]),
    # z = (1, 1, 0, -1 x 7), K1 = {0, 1, 2}: over K1 token 2 has m = 1 / (2 e + 1) = 0.155 <= 0.2 and goes; over the full row (top-p first) its m would be
    # (1 + 7 / e) / (2 e + 1 + 7 / e) = 0.397 and it would stay
    ("top-k then top-p: p acts on the softmax renormalised over K1", [4.0, 4.0, 0.0, -4.0, -4.0, -4.0, -4.0, -4.0, -4.0, -4.0], 4.0, 3, 0.8, [0, 1]),
    ("-0 and +0 are one tie group", [-0.0, 0.0, -3.0], 1.0, 1, 1.0, [0, 1]),
)


# ------------------------------------------------------------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "name idx V N T k p kinds ldl_pad ldp_pad eos")
KINDS = ("randn3", "all_equal", "dominant", "tie_k", "tie_p", "neg_inf", "big")
VS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 32003, REG_MAX - 1, REG_MAX, REG_MAX + 1)
NS = (1, 2, 8)
SEED_BUMP = {}                       # case name -> seed offset, where the default seed leaves a cumulative mass within delta_p of 1 - p (none needed)


def _settings(V):
    return ((1.0, 0, 1.0), (1.0, 1, 1.0), (1.0, V - 1, 0.9), (1.0, V + 5, 0.95), (0.01, 0, 0.9), (2.0, 50, 0.8), (1.0, 0, 1e-3), (0.7, 40, 0.95))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for vi, V in enumerate(VS):
        for j in range(3 if V < 30000 else 4):
            idx = len(out)
            T, k, p = _settings(V)[(3 * vi + j * 3 + (vi // 8)) % 8]
            N = NS[(vi + j) % 3]
            kinds = tuple(KINDS[(idx + n) % len(KINDS)] for n in range(N))
            pads = ((0, 0), (3, 5), (8, 0), (0, 1))[idx % 4]
            out.append(Case(f"V{V}_N{N}_T{T}_k{k}_p{p}_{kinds[0]}", idx, V, N, T, k, p, kinds, pads[0], pads[1], N >= 2 and idx % 3 != 2))
    return tuple(out)


def _row(kind, V, k, g):
    x = 3.0 * torch.randn(V, generator=g)
    if kind == "all_equal":
        x = torch.full((V,), 1.25)
    elif kind == "dominant":
        x[int(torch.randint(V, (1,), generator=g))] = 30.0
    elif kind == "tie_k":                                      # a tie group that straddles the k-th value (k on: ranks k-2 .. k+1; k off: ties everywhere)
        if 1 <= k < V:
            order = torch.argsort(x, descending=True)
            x[order[max(k - 2, 0):min(k + 2, V)]] = float(x[order[k - 1]])
        else:
            x = torch.round(x)
    elif kind == "tie_p":                                      # multiples of 1/2: every top-p boundary falls between or inside big tie groups
        x = torch.round(2.0 * x) / 2.0
    elif kind == "neg_inf":
        x[torch.rand(V, generator=g) < 0.35] = -INF
        x[int(torch.randint(V, (1,), generator=g))] = 0.5       # at least one finite logit
    elif kind == "big":
        x = (x * 3000.0).clamp(-1e4, 1e4)
    return x.to(BF)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict(logits bf16 [N + 1, V + ldl_pad] (row N and the pad columns: decoys the kernel must not read as data), u fp32 [N + 1], unfinished int64 [N], eos, pad)"""
    g = torch.Generator().manual_seed(1000 + case.idx + SEED_BUMP.get(case.name, 0))
    V, N = case.V, case.N
    buf = (3.0 * torch.randn(N + 1, V + case.ldl_pad, generator=g) + 40.0).to(BF)         # decoys far above every row: reading one changes the result
    for n, kind in enumerate(case.kinds):
        buf[n, :V] = _row(kind, V, case.k, g)
    u = torch.rand(N + 1, generator=g, dtype=F32).clamp(max=U_MAX)
    if case.idx % 5 == 0:
        u[0] = 0.0
    if case.idx % 5 == 1:
        u[N - 1] = U_MAX
    unfinished = torch.ones(N, dtype=torch.int64)
    eos, pad = None, 0
    if case.eos:
        unfinished[1::3] = 0
        eos = draw(rule(buf[0, :V], case.T, case.k, case.p), float(u[0]))                  # row 0 finishes at this step
        pad = V + 7
    return dict(logits=buf, u=u, unfinished=unfinished, eos=eos, pad=pad)


def reference_rows(logits, T, k, p):
    """logits bf16 [N, V] (CPU) -> per row: the fp64 rule, its bounds and the two kept sets at 1 - p -+ delta_p"""
    rows = []
    for l in logits:
        ref = rule(l, T, k, p)
        b = bounds(ref)
        rows.append(dict(ref, b=b, lo=rule(l, T, k, p, +b["dp"])["K2"], hi=rule(l, T, k, p, -b["dp"])["K2"], l=_canon(l)))
    return rows


@functools.lru_cache(maxsize=None)
def reference(case):
    """`reference_rows` of the case's rows (the two kept sets are equal, by the choice of seeds: test_sampling_cpu.py asserts it)"""
    return reference_rows(inputs(case)["logits"][:case.N, :case.V], case.T, case.k, case.p)


# ------------------------------------------------------------------------------------------------------------------------------------ the check
def check(case, out):
    """`check_rows` of the kernel's (or the emulation's, or a mutant's) outputs on `inputs(case)`"""
    inp = inputs(case)
    return check_rows(reference(case), case.p, inp["u"], inp["unfinished"], inp["eos"], inp["pad"], out)


def check_rows(rows, p, u_all, uf_in, eos, pad, out):
    """rows = `reference_rows` of the logits; u_all fp32 [>= N]; uf_in int64 [N] = `unfinished` before the call; eos None = no eos rule;
    out = dict(next int64 [N], logprob fp32 [N], kept int32 [N], probs fp32 [N, V], unfinished int64 [N] after the call)
    -> the worst error / bound over every assertion on the kernel; a violated exact assertion (kept sets between the two fp64 sets, whole tie groups, the
    token's range, eos / pad bookkeeping) counts as inf.  A padded row's token and logprob are checked for pad and 0."""
    inp = dict(eos=eos, pad=pad, u=u_all)
    worst = 0.0
    for n, R in enumerate(rows):
        V = R["r"].numel()
        tok = int(out["next"][n])
        padded = inp["eos"] is not None and int(uf_in[n]) == 0
        want_uf = int(uf_in[n]) if inp["eos"] is None else int(bool(uf_in[n]) and tok != inp["eos"])
        if int(out["unfinished"][n]) != want_uf or (padded and (tok != inp["pad"] or float(out["logprob"][n]) != 0.0)):
            return INF
        pr = out["probs"][n].to(F64)
        pk = pr > 0
        kept = int(out["kept"][n])
        if p < 1:
            if not (bool((R["lo"] <= pk).all()) and bool((pk <= R["hi"]).all()) and kept == int(pk.sum())):
                return INF
        elif not (bool((pk <= R["K2"]).all()) and kept == int(R["K2"].sum())):
            return INF
        if bool(torch.isin(R["l"][pk].unique(), R["l"][~pk].unique()).any()):      # a tie group split: one logit value on both sides
            return INF
        worst = max(worst, float(((pr - R["r"]).abs() / R["b"]["probs"]).max()))
        if padded:
            continue
        if not (0 <= tok < V) or not bool(R["hi"][tok]):
            return INF
        u = float(inp["u"][n])
        below = float(R["C"][tok - 1]) if tok > 0 else 0.0
        worst = max(worst, max(below - u, u - float(R["C"][tok]), 0.0) / R["b"]["du"])
        lnr = math.log(float(R["r"][tok])) if float(R["r"][tok]) > 0 else -INF
        lp = float(out["logprob"][n])
        if lnr == -INF or lp == -INF:
            worst = max(worst, 0.0 if lnr == lp else INF)
        else:
            worst = max(worst, abs(lp - lnr) / float(R["b"]["logprob"][tok]))
    return worst


# ------------------------------------------------------------------------------------------------------------------- emulation of the kernel, mutants
MUTANTS = ("topk_strict", "topp_before_topk", "temperature_ignored", "cdf_in_sorted_order", "tail_dropped", "u_row_plus_1", "ldl_ignored", "eos_ignored")


def mutant_names(case):
    """the mutants that compute something else on this case"""
    V, N = case.V, case.N
    names = []
    if 1 <= case.k < V:
        names.append("topk_strict")
        if case.p < 1:
            names.append("topp_before_topk")
    if case.T != 1.0 and V > 2:
        names.append("temperature_ignored")
    if V > 8:
        names += ["cdf_in_sorted_order", "tail_dropped"]
    if N >= 2 and V > 8:
        names.append("u_row_plus_1")
    if N >= 2 and case.ldl_pad:
        names.append("ldl_ignored")
    if case.eos:
        names.append("eos_ignored")
    return names


def _emulate_row(l, T, k, p, u, mutant=None):
    """one row in the kernel's own arithmetic: fp32 weights expf(fl(fl(l - l_max) / T)), integer masses floor(e 2^40), integer sums, integer threshold compares"""
    lf = l.to(F32) + 0.0
    V = lf.numel()
    T32 = torch.tensor(1.0 if mutant == "temperature_ignored" else T, dtype=F32)
    valid = torch.ones(V, dtype=torch.bool)
    if mutant == "tail_dropped":
        valid[(V - 1) // 8 * 8:] = False                       # the last partial (or whole) group of 8 is never read
    finite_above = bool((lf[valid] > -INF).any())
    lmax = lf[valid].max()
    e = torch.exp(((lf - lmax) / T32).to(F32))
    mass = torch.where((e > 0) & valid, torch.floor(e.to(F64) * 2.0 ** FB), torch.zeros(V, dtype=F64)).to(torch.int64)

    def top_p(K):
        if not p < 1:
            return K
        S = int(mass[K].sum())
        target = int(math.floor((1.0 - float(torch.tensor(p, dtype=F32))) * float(S)))
        order = torch.argsort(lf)
        ls, cs = lf[order], torch.cumsum(torch.where(K, mass, torch.zeros_like(mass))[order], 0)
        m = cs[torch.searchsorted(ls, lf, right=True) - 1]
        return K & (m > target) if S > 0 else K

    def top_k(K):
        if not 1 <= k < V:
            return K
        vals = torch.where(K, lf, torch.full_like(lf, -INF))
        kth = torch.topk(vals, k).values[-1]
        return K & ((lf > kth) if mutant == "topk_strict" else (lf >= kth))

    K = valid.clone()
    if finite_above:
        K &= lf > -INF
    K2 = top_k(top_p(K)) if mutant == "topp_before_topk" else top_p(top_k(K))
    km = torch.where(K2, mass, torch.zeros_like(mass))
    S2 = int(km.sum())
    rinv = 1.0 / float(S2) if S2 else 0.0
    tt = int(math.floor(float(u) * float(S2)))
    if mutant == "cdf_in_sorted_order":                        # the CDF walked from the most probable token down
        order = torch.argsort(lf, descending=True, stable=True)
        hit = (torch.cumsum(km[order], 0) > tt) & K2[order]
        tok = int(order[hit.nonzero()[0]]) if bool(hit.any()) else int(order[K2[order].nonzero()[-1]]) if bool(K2.any()) else V - 1
    else:
        hit = (torch.cumsum(km, 0) > tt) & K2
        tok = int(hit.nonzero()[0]) if bool(hit.any()) else int(K2.nonzero()[-1]) if bool(K2.any()) else V - 1
    probs = (km.to(F64) * rinv).to(F32)
    mt = float(mass[tok]) * rinv
    lp = math.log(mt) if mt > 0 else -INF
    return tok, torch.tensor(lp, dtype=F32), int(K2.sum()), probs


def emulate(case, mutant=None):
    """the kernel's outputs on `inputs(case)` from the emulation (mutant = None) or from one of MUTANTS"""
    inp = inputs(case)
    V, N = case.V, case.N
    flat = inp["logits"].reshape(-1)
    ldl = V + case.ldl_pad
    nxt, lps, kept, probs = [], [], [], []
    uf = inp["unfinished"].clone()
    for n in range(N):
        start = n * (V if mutant == "ldl_ignored" else ldl)
        u = inp["u"][n + 1 if mutant == "u_row_plus_1" else n]
        tok, lp, kc, pr = _emulate_row(flat[start:start + V], case.T, case.k, case.p, u, mutant)
        if inp["eos"] is not None and mutant != "eos_ignored":
            if int(uf[n]) == 0:
                tok, lp = inp["pad"], torch.tensor(0.0)
            uf[n] = int(bool(uf[n]) and tok != inp["eos"])
        nxt.append(tok)
        lps.append(lp)
        kept.append(kc)
        probs.append(pr)
    return dict(next=torch.tensor(nxt, dtype=torch.int64), logprob=torch.stack(lps).to(F32), kept=torch.tensor(kept, dtype=torch.int32), probs=torch.stack(probs),
                unfinished=uf)


# ------------------------------------------------------------------------------------------------------------------------ Hugging Face's warpers
def hf_filtered_softmax(l, T, k, p):
    """softmax of TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (the installed transformers) on one bf16 row, in fp32 as HF samples; fp32 [V]"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = l.to(F32)[None, :]
    ids = torch.zeros((1, 1), dtype=torch.int64)
    s = TemperatureLogitsWarper(float(T))(ids, s)
    if k > 0:
        s = TopKLogitsWarper(top_k=int(k))(ids, s)
    if p < 1:
        s = TopPLogitsWarper(top_p=float(p))(ids, s)
    return torch.softmax(s, -1)[0]


HF_V = (257, 1000, 4099, 32000)
HF_SETTINGS = ((1.0, 0, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.95), (0.01, 0, 0.9), (2.0, 0, 0.5), (2.0, 7, 0.99), (1.0, 1, 1.0), (0.3, 1000, 0.8),
               (1.5, 256, 0.3), (1.0, 0, 0.05), (0.9, 40, 0.9))
HF_TOL = 3e-6            # HF's softmaxes and cumulative sum run in fp32 over <= 32000 terms; the issue measured <= 3e-7 on these inputs


# ------------------------------------------------------------------------------------------------------------------------------ distribution
DIST_V, DIST_M = 257, 4096


@functools.lru_cache(maxsize=None)
def distribution_case():
    """one row (V = 257, T = 1.5, k = 100, p = 0.95) -> (logits bf16 [V], T, k, p, u fp32 [M] = (j + 1/2) / M, the fp64 reference with its bounds)"""
    g = torch.Generator().manual_seed(77)
    l = (3.0 * torch.randn(DIST_V, generator=g)).to(BF)
    T, k, p = 1.5, 100, 0.95
    u = ((torch.arange(DIST_M, dtype=F64) + 0.5) / DIST_M).to(F32)
    ref = rule(l, T, k, p)
    return l, T, k, p, u, dict(ref, b=bounds(ref))
