"""Fused attention forward / backward at ragged key masks and tile edges: fp64 references, a LOCAL tolerance, a bf16 emulation of
what the kernels round, and mutants (fp64 results of subtly wrong problems) that the tolerance must reject.

Everything here runs on the CPU (no import of the HIP library).  tests/test_attention_edges_cpu.py proves that the tolerance passes
the emulation with a 2x margin and rejects every applicable mutant by at least 2x on every case; tests/test_attention_edges_gpu.py
holds the kernels to the same rule.

Layout: q / k / v / dO are [B, H, N, hd]; key_mask is uint8 [B, Nk] (1 = attend); lse is the kernels' base-2 row statistic
log2 sum_valid exp(scale * s), [B, H, Nq].
"""
import functools
import math

import torch

BF = torch.bfloat16
F64 = torch.float64
INF = float("inf")

C_FWD = 5.0                   # forward o:  |got - ref| <= C_FWD * 2^-8 * (|ref| + sigma_row)
C_BWD = 8.0                   # dq, dk, dv: |got - ref| <= C_BWD * 2^-8 * (|ref| + sigma_row)  (dS rounding meets cancellation in the sums)
GRAD_FLOOR = 2.0 ** -8        # dq, dk, dv: added to sigma_row.  Rows whose exact gradient vanishes (a softmax over ONE key: dS = P (dP - D) = 0)
                              # come out of fp32 as ~1e-5 (dP and D round differently); masked keys' dk / dv rows are checked for exact zeros apart
SELF_K = 0.1                  # self attention: k_i += SELF_K * q_i, so the diagonal key (the one causal / tile-edge bugs move) carries weight
LSE_TOL = 2.0 ** -12          # lse: absolute (fp32 arithmetic on fp32 scores)
EMU_MAX = 0.5                 # the bf16 emulation must stay at <= half the bound
MUT_MIN = 2.0                 # every applicable mutant must exceed the bound by >= 2x

HDS = (32, 64, 128)           # what the backward supports
TS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 321)
BKV = 64                      # key tile of the forward kernel


# ----------------------------------------------------------------------------------------------------------------- the case table
class Case:
    def __init__(self, name, hd, B, H, Nq, Nk, causal, lens=None, nk_valid=None, bwd=True):
        self.name, self.hd, self.B, self.H, self.Nq, self.Nk = name, hd, B, H, Nq, Nk
        self.causal, self.lens, self.nk_valid, self.bwd = causal, lens, nk_valid, bwd

    def __repr__(self):
        return self.name

    def __eq__(self, o):
        return isinstance(o, Case) and self.name == o.name

    def __hash__(self):
        return hash(self.name)

    @property
    def scale(self):
        return self.hd ** -0.5

    @property
    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) % 100003

    @property
    def nk_eff(self):
        """the key count the kernel attends over (nk_dev below the capacity Nk)"""
        return self.Nk if self.nk_valid is None else self.nk_valid

    def key_mask(self):
        if self.lens is None:
            return None
        km = torch.zeros(self.B, self.Nk, dtype=torch.uint8)
        for b, L in enumerate(self.lens):
            km[b, :L] = 1
        return km


def ragged_lens(T):
    """>= 4 right-padded lengths covering 1, 63, 64, 65, 128, T - 1 and T (those in [1, T]); neighbours differ where T allows"""
    ls = []
    for L in (T, 1, 64, T - 1, 63, 128, 65):
        if 1 <= L <= T and L not in ls:
            ls.append(L)
    for L in (T // 2, T // 3, (3 * T) // 4):
        if len(ls) < 4 and L >= 1 and L not in ls:
            ls.append(L)
    n = len(ls)
    while len(ls) < 4:
        ls.append(ls[len(ls) % n])
    return ls


def cases():
    """The shared forward / backward table (every T x {plain, causal} x {no mask, ragged mask}, head_dim rotating so that every head_dim
    meets every mask form), the non-causal Nq != Nk backward shapes in both orders, and the forward's wide route (Nq >= 1024, non-causal,
    8 waves per workgroup) at 1024, 1025 and 4097 tokens (DINOv2-L at 896^2), with and without a key mask and once with nk_dev."""
    out = []
    for i, T in enumerate(TS):
        for j, (causal, masked) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            hd = HDS[(i + j) % 3]
            lens = ragged_lens(T) if masked else None
            name = f"T{T}_hd{hd}_{'causal' if causal else 'plain'}_{'mask' if masked else 'nomask'}"
            out.append(Case(name, hd, len(lens) if masked else 4, 2, T, T, causal, lens))
    for Nq, Nk, hd in ((70, 300, 64), (300, 70, 128)):
        for masked in (False, True):
            lens = [Nk, 1, 64, Nk - 1] if masked else None
            out.append(Case(f"cross{Nq}x{Nk}_hd{hd}_{'mask' if masked else 'nomask'}", hd, 4, 2, Nq, Nk, False, lens))
    for N, H, lens in ((1024, 2, None), (1025, 2, [1025, 1, 64, 1024]), (4097, 1, None), (4097, 1, [4097, 1, 2049, 4096])):
        out.append(Case(f"wide{N}_hd64_{'mask' if lens else 'nomask'}", 64, len(lens) if lens else 2, H, N, N, False, lens, bwd=False))
    out.append(Case("wide1025_hd64_mask_nkdev700", 64, 2, 2, 1025, 1025, False, [1025, 300], nk_valid=700, bwd=False))
    return out


def make_inputs(case):
    """q, k with std 1.5 (scores after scaling have std ~2: single keys matter; in self attention k_i leans towards q_i), v and dO with
    std 1; bf16"""
    g = torch.Generator().manual_seed(case.seed)
    B, H, hd = case.B, case.H, case.hd
    q = torch.randn(B, H, case.Nq, hd, generator=g) * 1.5
    k = torch.randn(B, H, case.Nk, hd, generator=g) * 1.5
    if case.Nq == case.Nk:
        k = k + SELF_K * q
    q, k = q.to(BF), k.to(BF)
    v = torch.randn(B, H, case.Nk, hd, generator=g).to(BF)
    do = torch.randn(B, H, case.Nq, hd, generator=g).to(BF)
    return q, k, v, do


# ------------------------------------------------------------------------------------------------------------------- references
def allowed_mask(B, Nq, Nk, causal, key_mask, nk_valid=None, diag=0, tile_cut=None):
    """bool [B, 1, Nq, Nk]: query i may attend key j.  diag moves the causal edge (key <= i + diag); keys >= tile_cut are dropped."""
    kj = torch.arange(Nk)
    a = (kj < (Nk if nk_valid is None else nk_valid))[None, None, None, :].expand(B, 1, Nq, Nk)
    if key_mask is not None:
        a = a & (key_mask != 0)[:, None, None, :]
    if causal:
        a = a & (kj[None, :] <= torch.arange(Nq)[:, None] + diag)[None, None]
    if tile_cut is not None:
        a = a & (kj < tile_cut)[None, None, None, :]
    return a


def _row_chunks(B, H, Nq, Nk):
    step = max(1, min(Nq, (1 << 24) // max(1, B * H * Nk)))
    return [(i, min(Nq, i + step)) for i in range(0, Nq, step)]


def _fwd(q, k, v, scale, allowed, emulate=False, drop_key=None):
    """fp64 masked softmax attention -> (o, lse2).  A row without a valid key gives o = 0 and lse = -inf.  emulate: P is rounded to
    bf16 before P.V (the normaliser sums the unrounded P) and o to bf16, as the forward kernel does.  drop_key: that key is left out of
    the normaliser (the lse mutant)."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    B, H, Nq, _ = q.shape
    o = torch.empty(B, H, Nq, v.shape[-1], dtype=F64)
    lse = torch.empty(B, H, Nq, dtype=F64)
    for i0, i1 in _row_chunks(B, H, Nq, k.shape[2]):
        s = ((q[:, :, i0:i1] @ k.transpose(-1, -2)) * scale).masked_fill(~allowed[:, :, i0:i1], -INF)
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = torch.exp(s - m)
        l = (p if drop_key is None else p.index_fill(-1, torch.tensor([drop_key]), 0.0)).sum(-1, keepdim=True)
        oc = ((p.to(BF).to(F64) if emulate else p) @ v) / l
        o[:, :, i0:i1] = torch.nan_to_num(oc, nan=0.0, posinf=0.0, neginf=0.0)
        lse[:, :, i0:i1] = ((m + torch.log(l)) / math.log(2.0)).squeeze(-1)
    if emulate:
        o, lse = o.to(BF).to(F64), lse.float().to(F64)
    return o, lse


def attn_ref(q, k, v, scale, causal, key_mask, Nk_valid=None):
    """fp64 forward reference -> (o, lse2), lse2 = log2 sum_valid exp(scale * s); masked keys get -inf"""
    return _fwd(q, k, v, scale, allowed_mask(q.shape[0], q.shape[2], k.shape[2], causal, key_mask, Nk_valid))


def attn_bwd_ref(q, k, v, scale, causal, key_mask, do, Nk_valid=None, o=None):
    """fp64 gradients (dq, dk, dv) of the masked softmax attention.  o = None: fp64 autograd.  o given (the bf16 forward output that the
    backward kernel is handed): the same gradients with D = rowsum(dO * o) taken from it, as the kernel's delta is -- the explicit
    backward, which equals the autograd one when o is the exact output (tests/test_attention_edges_cpu.py).  Without this, the bf16
    rounding of O alone moves D by ~2^-9 |dO| |O|, which swamps the gradient of rows whose softmax is saturated."""
    a = allowed_mask(q.shape[0], q.shape[2], k.shape[2], causal, key_mask, Nk_valid)
    if o is not None:
        return _bwd(q, k, v, do, scale, a, o)
    qq, kk, vv = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    s = ((qq @ kk.transpose(-1, -2)) * scale).masked_fill(~a, -INF)
    (torch.softmax(s, -1) @ vv).backward(do.to(F64))
    return qq.grad, kk.grad, vv.grad


def _bwd(q, k, v, do, scale, allowed, o_delta, emulate=False, delta_zero=False, allowed_dq=None, allowed_dkv=None):
    """explicit fp64 backward with the kernel's structure: P = exp(scale s - lse) on the forward's key set, D = rowsum(dO * O),
    dS = scale P (dP - D), dQ = dS K, dK = dS^T Q, dV = P^T dO.  allowed_dq / allowed_dkv: the key set that the dQ pass / the dK and dV
    passes apply (mutants).  emulate: P (for dV) and dS are rounded to bf16 before their products and the gradients to bf16."""
    q, k, v, do = q.to(F64), k.to(F64), v.to(F64), do.to(F64)
    s = (q @ k.transpose(-1, -2)) * scale
    sm = s.masked_fill(~allowed, -INF)
    m = sm.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    lse = m + torch.log(torch.exp(sm - m).sum(-1, keepdim=True))
    e = torch.exp(s - lse)
    D = torch.zeros_like(lse) if delta_zero else (do * o_delta.to(F64)).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    rnd = (lambda t: t.to(BF).to(F64)) if emulate else (lambda t: t)
    zero = torch.zeros((), dtype=F64)
    p_q = torch.where(allowed if allowed_dq is None else allowed_dq, e, zero)
    p_kv = torch.where(allowed if allowed_dkv is None else allowed_dkv, e, zero)
    dq = rnd(scale * p_q * (dP - D)) @ k
    dk = rnd(scale * p_kv * (dP - D)).transpose(-1, -2) @ q
    dv = rnd(p_kv).transpose(-1, -2) @ do
    return (rnd(dq), rnd(dk), rnd(dv)) if emulate else (dq, dk, dv)


# -------------------------------------------------------------------------------------------------------------------- tolerance
def ratio(got, ref, c=C_FWD, floor=0.0):
    """max over elements of |got - ref| / (c 2^-8 (|ref| + sigma_row + floor)), sigma_row = the RMS of that row of the reference (last
    dim): local, never normalised by the tensor-wide maximum.  With floor 0 a row whose reference is exactly zero must be exactly zero;
    NaN -> inf."""
    got, ref = got.to(F64), ref.to(F64)
    bound = c * 2.0 ** -8 * (ref.abs() + ref.pow(2).mean(-1, keepdim=True).sqrt() + floor)
    d = (got - ref).abs()
    r = torch.nan_to_num(torch.where(d == 0, torch.zeros_like(d), d / bound), nan=INF, posinf=INF)
    return float(r.max()) if r.numel() else 0.0


def lse_ratio(got, ref):
    """max |got - ref| / LSE_TOL (absolute); NaN -> inf"""
    d = (got.to(F64) - ref.to(F64)).abs()
    return float(torch.nan_to_num(d, nan=INF, posinf=INF).max()) / LSE_TOL if d.numel() else 0.0


def grad_ratios(got, ref):
    return {n: ratio(g, r, C_BWD, GRAD_FLOOR) for n, g, r in zip(("dq", "dk", "dv"), got, ref)}


# --------------------------------------------------------------------------------------------------------- reference / emulation / mutants
@functools.lru_cache(maxsize=2)
def reference(case):
    """(inputs (q, k, v, dO), forward reference (o, lse), backward reference (dq, dk, dv) or None)"""
    q, k, v, do = make_inputs(case)
    km = case.key_mask()
    fwd = attn_ref(q, k, v, case.scale, case.causal, km, case.nk_valid)
    bwd = attn_bwd_ref(q, k, v, case.scale, case.causal, km, do, case.nk_valid) if case.bwd else None
    return (q, k, v, do), fwd, bwd


def _allowed(case, key_mask="case", **kw):
    km = case.key_mask() if isinstance(key_mask, str) else key_mask
    return allowed_mask(case.B, case.Nq, case.Nk, case.causal, km, case.nk_valid, **kw)


def emulation_ratios(case):
    """tolerance ratios of the bf16 emulation against the fp64 reference: forward o, lse; backward dq, dk, dv"""
    (q, k, v, do), (ro, rl), rb = reference(case)
    a = _allowed(case)
    eo, el = _fwd(q, k, v, case.scale, a, emulate=True)
    r = {"fwd o": ratio(eo, ro), "fwd lse": lse_ratio(el, rl)}
    if rb is not None:      # the backward kernel is handed the forward's bf16 O: its reference takes D from that O
        rbo = attn_bwd_ref(q, k, v, case.scale, case.causal, case.key_mask(), do, case.nk_valid, o=eo)
        r.update({"bwd " + n: x for n, x in grad_ratios(_bwd(q, k, v, do, case.scale, a, eo, emulate=True), rbo).items()})
    return r


def _lens_shifted(case, d):
    """key mask with every sequence's valid length L -> L + d"""
    lens = case.lens if case.lens is not None else [case.Nk] * case.B
    km = torch.zeros(case.B, case.Nk, dtype=torch.uint8)
    for b, L in enumerate(lens):
        km[b, :max(0, min(case.Nk, min(L, case.nk_eff) + d))] = 1
    return km


def mutant_masks(case):
    """mutant name -> the key set (allowed mask) of that wrong problem, for the mutants that apply to this case"""
    km = case.key_mask()
    lens = [min(L, case.nk_eff) for L in (case.lens if case.lens is not None else [case.Nk] * case.B)]
    out = {"drop_last_valid_key": _allowed(case, _lens_shifted(case, -1))}
    if any(L < case.nk_eff for L in lens):
        out["admit_one_padded_key"] = _allowed(case, _lens_shifted(case, +1))
    if case.causal:
        out["causal_key_lt_q"] = _allowed(case, diag=-1)
        if case.Nk >= 2:
            out["causal_key_le_q+1"] = _allowed(case, diag=1)
    if case.nk_eff % BKV:
        out["last_partial_tile_ignored"] = _allowed(case, tile_cut=(case.nk_eff // BKV) * BKV)
    if km is not None and len(set(lens)) > 1:
        out["mask_of_b_on_b+1"] = _allowed(case, torch.roll(km, 1, 0))
    return out


def mutant_ratios(case):
    """mutant name -> its tolerance ratio against the fp64 reference (the worst over the outputs it corrupts)"""
    (q, k, v, do), (ro, rl), rb = reference(case)
    a = _allowed(case)
    out = {}
    for name, am in mutant_masks(case).items():
        mo, ml = _fwd(q, k, v, case.scale, am)
        out["fwd " + name] = max(ratio(mo, ro), lse_ratio(ml, rl))
        if rb is not None:
            out["bwd " + name] = max(grad_ratios(_bwd(q, k, v, do, case.scale, am, mo), rb).values())
    if rb is not None:
        out["bwd delta_zero"] = max(grad_ratios(_bwd(q, k, v, do, case.scale, a, ro, delta_zero=True), rb).values())
        if case.lens is not None and any(L < case.Nk for L in case.lens):
            free = _allowed(case, None)
            g = _bwd(q, k, v, do, case.scale, a, ro, allowed_dkv=free)
            out["bwd masked_keys_dk_dv_nonzero"] = max(ratio(g[1], rb[1], C_BWD, GRAD_FLOOR), ratio(g[2], rb[2], C_BWD, GRAD_FLOOR))
            g = _bwd(q, k, v, do, case.scale, a, ro, allowed_dq=free)
            out["bwd dq_ignores_key_mask"] = ratio(g[0], rb[0], C_BWD, GRAD_FLOOR)
    out["lse natural_log"] = lse_ratio(rl * math.log(2.0), rl)
    out["lse missing_key0_term"] = lse_ratio(_fwd(q, k, v, case.scale, a, drop_key=0)[1], rl)
    return out
