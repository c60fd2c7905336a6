"""The attention routes of SAM's image encoder (decomposed relative-position bias, 14 x 14 windows, the window gather, the 64-wide global
grid): fp64 references, the LOCAL tolerance of tests/attention_edge_checks.py (unchanged), a bf16 emulation of what the kernels round,
and mutants (fp64 results of subtly wrong problems) that the tolerance must reject.

Everything here runs on the CPU (no import of the HIP library).  tests/test_attention_relpos_cpu.py proves that the tolerance passes the
emulation with a 2x margin and rejects every applicable mutant by at least 2x on every case; tests/test_attention_relpos_gpu.py holds the
kernels to the same rule, route by route (the dispatch conditions are listed in profiles/attn_relpos_parity.md).

    o = softmax(scale * q k^T + bias) v,   bias(q, k) = Gh[q][qh - kh + gh - 1] + Gw[q][qw - kw + gw - 1]   (the bias is NOT scaled)
    lse = log2 sum_k exp(scale * s + bias)

Table routes ("tab", "gather": rel_tab_*): Gh = q . Rh^T and Gw = q . Rw^T in fp64 from the bf16 q and the bf16 tables.  Array routes ("arr":
rel_h / rel_w): the same products rounded once to fp32, handed to the kernel as [heads][batch * Nq][rel_ld] with every column the API gives
no meaning (>= 2 gh - 1 of rel_h, >= 2 gw - 1 of rel_w) set to NaN.

Layout: q / k / v / o are [B, H, N, hd]; an ITEM is (b, h) with the heads fastest (what the window kernels' persistent loop walks).
"""
import functools
import math

import torch

from tests.attention_edge_checks import BF, C_FWD, EMU_MAX, F64, INF, LSE_TOL, MUT_MIN, SELF_K, lse_ratio, ratio   # noqa: F401  (re-exported)

WS = 14                       # SAM's window
TAB_STD = 0.1                 # rel-pos tables: q (std 1.5) . R over head_dim 80 gives a bias of std ~2 in logit units: single keys decide rows
REL_LD_EXTRA = 5              # rel_ld = 2 max(gh, gw) - 1 + this (>= 4 NaN columns behind the longest row)


# ----------------------------------------------------------------------------------------------------------------- the case table
class Case:
    """kind "tab": B windows of 14 x 14 through rel_tab_*; "gather": `images` images on a g x g grid, windows gathered inside the kernel
    (B = images * ceil(g / 14)^2); "arr": a gh x gw grid through rel_h / rel_w"""

    def __init__(self, name, kind, hd, B, H, gh, gw, g=0, images=0, lse=False):
        self.name, self.kind, self.hd, self.B, self.H, self.gh, self.gw = name, kind, hd, B, H, gh, gw
        self.g, self.images, self.lse = g, images, lse

    def __repr__(self):
        return self.name

    def __eq__(self, o):
        return isinstance(o, Case) and self.name == o.name

    def __hash__(self):
        return hash(self.name)

    @property
    def N(self):
        return self.gh * self.gw

    @property
    def scale(self):
        return self.hd ** -0.5

    @property
    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) % 100003

    @property
    def nw(self):
        return (self.g + WS - 1) // WS

    @property
    def rel_ld(self):
        return 2 * max(self.gh, self.gw) - 1 + REL_LD_EXTRA


def _tab(name, B, H):
    return Case(name, "tab", 80, B, H, WS, WS)


def _gather(name, g, images, H):
    nw = (g + WS - 1) // WS
    return Case(name, "gather", 80, images * nw * nw, H, WS, WS, g=g, images=images)


def _arr(name, hd, B, H, gh, gw, lse=False):
    return Case(name, "arr", hd, B, H, gh, gw, lse=lse)


def cases():
    """the smallest shapes that reach each route of launch_hd (csrc/attention.hip); lse = True: the case is ALSO run with lse requested"""
    return [
        _tab("win_b3_h2", 3, 2), _tab("win_b5_h8", 5, 8), _tab("win_b33_h8", 33, 8),
        _gather("gather_g15", 15, 2, 2), _gather("gather_g27", 27, 2, 2), _gather("gather_g28", 28, 2, 2), _gather("gather_g29", 29, 2, 2),
        _gather("gather_g15_i3_h8", 15, 3, 8),
        _arr("rel14_hd80", 80, 3, 2, 14, 14), _arr("rel14_hd64", 64, 3, 2, 14, 14),
        _arr("rel9x21_hd80", 80, 2, 2, 9, 21), _arr("rel21x9_hd80", 80, 2, 2, 21, 9), _arr("rel2x65_hd32", 32, 2, 2, 2, 65),
        _arr("rel5x64_hd80", 80, 2, 2, 5, 64), _arr("rel5x64_hd64", 64, 2, 2, 5, 64),
        _arr("rel17x64_hd80", 80, 1, 3, 17, 64), _arr("rel16x64_hd64", 64, 1, 3, 16, 64),
        _arr("rel16x64_hd80", 80, 1, 3, 16, 64, lse=True), _arr("rel16x64_hd80_b3_h3", 80, 3, 3, 16, 64),
        _arr("rel20x64_hd80", 80, 1, 2, 20, 64),
        _arr("rel68x64_hd80", 80, 1, 1, 68, 64),      # 4352 = 17 x 256 tokens, gh even but > 64: every condition of attn_glob80_dma_kernel but the height of its LDS bias table
    ]


TAB_LSE_CASE = "win_b3_h2"     # the table case that is also run with lse requested (attn_fwd_kernel<80, 4>)


def has_lse(case):
    return case.lse or case.name == TAB_LSE_CASE


# --------------------------------------------------------------------------------------------------------------------- inputs
def window_source(g, images):
    """int64 [images * nw^2, 196]: the token row (image * g^2 + y * g + x) that row (iy, ix) of window (wy, wx) holds, -1 = padding"""
    nw = (g + WS - 1) // WS
    wy, wx, iy, ix = torch.meshgrid(torch.arange(nw), torch.arange(nw), torch.arange(WS), torch.arange(WS), indexing="ij")
    ty, tx = WS * wy + iy, WS * wx + ix
    row = torch.where((ty < g) & (tx < g), ty * g + tx, torch.full_like(ty, -1)).reshape(nw * nw, WS * WS)
    return torch.cat([torch.where(row >= 0, row + i * g * g, row) for i in range(images)])


def materialise(tok, pad, src):
    """tok [rows, H, hd], pad [H, hd], src [B, 196] -> the padded windows [B, H, 196, hd]"""
    w = torch.where((src >= 0)[:, :, None, None], tok[src.clamp(min=0)], pad[None, None])
    return w.permute(0, 2, 1, 3).contiguous()


def make_problem(case):
    """dict: q, k, v [B, H, N, hd] bf16 (q, k with std 1.5 and k += 0.1 q, v with std 1), Rh [2 gh - 1, hd] / Rw [2 gw - 1, hd] bf16 tables;
    gather cases also: tok_q / tok_k / tok_v [images * g^2, H, hd], pad_q / pad_k / pad_v [H, hd] (drawn like token rows), src [B, 196]"""
    gen = torch.Generator().manual_seed(case.seed)
    H, hd = case.H, case.hd

    def qkv(*lead):
        q = torch.randn(*lead, H, hd, generator=gen) * 1.5
        k = torch.randn(*lead, H, hd, generator=gen) * 1.5 + SELF_K * q
        return q.to(BF), k.to(BF), torch.randn(*lead, H, hd, generator=gen).to(BF)
    P = {}
    if case.kind == "gather":
        P["tok_q"], P["tok_k"], P["tok_v"] = qkv(case.images * case.g * case.g)
        P["pad_q"], P["pad_k"], P["pad_v"] = qkv()
        P["src"] = window_source(case.g, case.images)
        for n in "qkv":
            P[n] = materialise(P["tok_" + n], P["pad_" + n], P["src"])
    else:
        P["q"], P["k"], P["v"] = (t.permute(0, 2, 1, 3).contiguous() for t in qkv(case.B, case.N))
    P["Rh"] = (torch.randn(2 * case.gh - 1, hd, generator=gen) * TAB_STD).to(BF)
    P["Rw"] = (torch.randn(2 * case.gw - 1, hd, generator=gen) * TAB_STD).to(BF)
    return P


def real_rows(case, P):
    """bool [B, N]: the query is a real token (all of them except the padding of the gathered windows)"""
    return P["src"] >= 0 if case.kind == "gather" else torch.ones(case.B, case.N, dtype=torch.bool)


def rel_products(case, q, Rh, Rw, fp32=None):
    """Gh [B, H, N, 2 gh - 1], Gw [B, H, N, 2 gw - 1] in fp64; array routes (or fp32 = True): rounded once to fp32"""
    Gh, Gw = q.to(F64) @ Rh.to(F64).t(), q.to(F64) @ Rw.to(F64).t()
    if case.kind == "arr" if fp32 is None else fp32:
        Gh, Gw = Gh.float().to(F64), Gw.float().to(F64)
    return Gh, Gw


def rel_arrays(case, Gh, Gw):
    """the kernel's rel_h / rel_w: fp32 [H][B * N][rel_ld], meaningless columns NaN"""
    out = []
    for G in (Gh, Gw):
        a = torch.full((case.H, case.B * case.N, case.rel_ld), float("nan"))
        a[:, :, :G.shape[-1]] = G.float().transpose(0, 1).reshape(case.H, case.B * case.N, -1)
        out.append(a)
    return out


def kernel_tables(P):
    """the kernel's rel_tab_h / rel_tab_w: bf16 [32][hd], rows >= 27 zero"""
    out = []
    for R in (P["Rh"], P["Rw"]):
        t = torch.zeros(32, R.shape[1], dtype=BF)
        t[:R.shape[0]] = R
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------------------------- references
def grid_coords(gh, gw):
    n = torch.arange(gh * gw)
    return n // gw, n % gw


def rel_index(gh, gw, kh=None, kw=None):
    """ih, iw [N, Nk]: the Gh / Gw column of (query, key); kh / kw = the key coordinates the (possibly wrong) problem uses"""
    qh, qw = grid_coords(gh, gw)
    kh, kw = qh if kh is None else kh, qw if kw is None else kw
    return qh[:, None] - kh[None, :] + gh - 1, qw[:, None] - kw[None, :] + gw - 1


def attend(q, k, v, scale, Gh, Gw, ih, iw, bias_mul=1.0, drop_key=None, emulate=False):
    """fp64 softmax(scale q k^T + bias_mul * (Gh[q][ih] + Gw[q][iw])) v -> (o [B, H, N, hd], lse2 [B, H, N]).  emulate: P is rounded to bf16 before
    P.V (the normaliser sums the unrounded P), o to bf16 and lse to fp32, as the kernels do."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    B, H, N, _ = q.shape
    o = torch.empty(B, H, N, v.shape[-1], dtype=F64)
    lse = torch.empty(B, H, N, dtype=F64)
    qi = torch.arange(N)[:, None]
    for b in range(B):
        s = (q[b] @ k[b].transpose(-1, -2)) * scale
        if bias_mul != 0.0:
            s = s + bias_mul * (Gh[b][:, qi, ih] + Gw[b][:, qi, iw])
        if drop_key is not None:
            s[..., drop_key] = -INF
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        o[b] = ((p.to(BF).to(F64) if emulate else p) @ v[b]) / l
        lse[b] = ((m + torch.log(l)) / math.log(2.0)).squeeze(-1)
    if emulate:
        o, lse = o.to(BF).to(F64), lse.float().to(F64)
    return o, lse


def solve(case, P, emulate=False, **kw):
    """the case's problem, with whatever a mutant changes passed as a keyword (q, k, v, Gh, Gw, ih, iw, bias_mul, drop_key)"""
    q = kw.pop("q", P["q"])
    if "Gh" not in kw:
        kw["Gh"], kw["Gw"] = rel_products(case, q, P["Rh"], P["Rw"], fp32=True if emulate else None)
    if "ih" not in kw:
        kw["ih"], kw["iw"] = rel_index(case.gh, case.gw)
    return attend(q, kw.pop("k", P["k"]), kw.pop("v", P["v"]), case.scale, emulate=emulate, **kw)


@functools.lru_cache(maxsize=4)
def reference(case):
    """(problem dict, (o, lse) fp64, (Gh, Gw) as the reference used them)"""
    P = make_problem(case)
    Gh, Gw = rel_products(case, P["q"], P["Rh"], P["Rw"])
    return P, solve(case, P, Gh=Gh, Gw=Gw), (Gh, Gw)


def rows_ratio(case, P, got, ref):
    """edge_checks.ratio of o [B, H, N, hd] over the real query rows"""
    keep = real_rows(case, P)
    if bool(keep.all()):
        return ratio(got, ref)
    return ratio(got.transpose(1, 2)[keep], ref.transpose(1, 2)[keep])


def rows_lse_ratio(case, P, got, ref):
    keep = real_rows(case, P)
    return lse_ratio(got.transpose(1, 2)[keep], ref.transpose(1, 2)[keep])


# --------------------------------------------------------------------------------------------------------- emulation / mutants
def emulation_ratios(case):
    P, (ro, rl), _ = reference(case)
    eo, el = solve(case, P, emulate=True)
    r = {"o": rows_ratio(case, P, eo, ro)}
    if has_lse(case):
        r["lse"] = rows_lse_ratio(case, P, el, rl)
    return r


def _items(t, case):
    """[B, H, ...] -> [B * H, ...] (item order: heads fastest)"""
    return t.reshape(case.B * case.H, *t.shape[2:])


def _roll_items(t, case, by):
    return torch.roll(_items(t, case), by, 0).reshape(t.shape)


def mutant_outputs(case):
    """mutant name -> its fp64 (o, lse), for the mutants that change this case's problem"""
    P, (ro, rl), (Gh, Gw) = reference(case)
    gh, gw, B, H, N = case.gh, case.gw, case.B, case.H, case.N
    qh, qw = grid_coords(gh, gw)
    ih, iw = rel_index(gh, gw)
    out = {}
    # ---- bias indexing
    if gh == gw:
        out["rel_h_w_swapped"] = solve(case, P, Gh=Gw, Gw=Gh)
    out["h_index_plus_one"] = solve(case, P, Gh=Gh, Gw=Gw, ih=(ih + 1).clamp(max=2 * gh - 2), iw=iw)
    out["h_index_sign_flipped"] = solve(case, P, Gh=Gh, Gw=Gw, ih=2 * (gh - 1) - ih, iw=iw)
    kh = torch.where(qh == gh - 1, qh - 1, qh)
    out["last_key_row_takes_previous_row"] = solve(case, P, Gh=Gh, Gw=Gw, ih=rel_index(gh, gw, kh=kh)[0], iw=iw)
    kh = torch.where((qw < 4) & (qh > 0), qh - 1, qh)
    out["first_columns_keep_previous_row"] = solve(case, P, Gh=Gh, Gw=Gw, ih=rel_index(gh, gw, kh=kh)[0], iw=iw)
    kw = qw.clone()
    kw[N - 1] -= 1
    out["one_key_w_entry_off"] = solve(case, P, Gh=Gh, Gw=Gw, ih=ih, iw=rel_index(gh, gw, kw=kw)[1])
    out["bias_scaled_by_scale"] = solve(case, P, Gh=Gh, Gw=Gw, bias_mul=case.scale)
    out["no_bias"] = solve(case, P, Gh=Gh, Gw=Gw, bias_mul=0.0)
    if B > 1 and H > 1:       # the rel row of (b, h) read at [b][h] of an [H][B] array
        at = torch.arange(B)[:, None] * H + torch.arange(H)[None, :]
        hh, bb = at // B, at % B
        out["rel_rows_batch_major"] = solve(case, P, Gh=Gh[bb, hh], Gw=Gw[bb, hh])
    # ---- key set
    out["drop_last_key"] = solve(case, P, Gh=Gh, Gw=Gw, drop_key=N - 1)
    if case.kind in ("tab", "gather"):      # the V image's filler rows are copies of row 195
        dup = lambda t: torch.cat([t, t[:, :, -1:]], 2)
        out["admit_key_196_as_copy_of_195"] = solve(case, P, Gh=Gh, Gw=Gw, k=dup(P["k"]), v=dup(P["v"]), ih=torch.cat([ih, ih[:, -1:]], 1),
                                                    iw=torch.cat([iw, iw[:, -1:]], 1))
    # ---- window gather
    if case.kind == "gather":
        if bool((P["src"] < 0).any()):
            W = {n: materialise(P["tok_" + n], torch.zeros_like(P["pad_" + n]), P["src"]) for n in "qkv"}
            out["padded_token_is_zero"] = solve(case, P, **W)
            if H > 1:
                W = {n: materialise(P["tok_" + n], P["pad_" + n][:1].expand(H, -1), P["src"]) for n in "qkv"}
                out["pad_row_of_head_0_for_every_head"] = solve(case, P, **W)
        if case.nw > 1:
            tr = lambda t: t.reshape(case.images, case.nw, case.nw, *t.shape[1:]).transpose(1, 2).reshape(t.shape)
            out["window_origin_transposed"] = (tr(ro), tr(rl))
    # ---- persistent loop / mapping
    if B * H > 1:
        pk, pv = _roll_items(P["k"], case, 1), _roll_items(P["v"], case, 1)
        out["stale_kv_of_previous_item"] = solve(case, P, Gh=Gh, Gw=Gw, k=pk, v=pv)
        out["stale_v_only"] = solve(case, P, Gh=Gh, Gw=Gw, v=pv)
        out["heads_rolled"] = (_roll_items(ro, case, -1), _roll_items(rl, case, -1))
    return out


def mutant_ratios(case):
    """mutant name -> the tolerance ratio of its o against the fp64 reference (lse is not counted: most routes do not write it); cases that
    are run with lse also get "lse <mutant>" for the mutants that move the normaliser"""
    P, (ro, rl), _ = reference(case)
    out = {}
    for name, (mo, ml) in mutant_outputs(case).items():
        out[name] = rows_ratio(case, P, mo, ro)
        if has_lse(case) and name in ("no_bias", "bias_scaled_by_scale", "drop_last_key", "h_index_plus_one", "heads_rolled"):
            out["lse " + name] = rows_lse_ratio(case, P, ml, rl)
    if has_lse(case):
        out["lse natural_log"] = rows_lse_ratio(case, P, rl * math.log(2.0), rl)
    return out


ALL_MUTANTS = {"rel_h_w_swapped", "h_index_plus_one", "h_index_sign_flipped", "last_key_row_takes_previous_row", "first_columns_keep_previous_row",
               "one_key_w_entry_off", "bias_scaled_by_scale", "no_bias", "rel_rows_batch_major", "drop_last_key", "admit_key_196_as_copy_of_195",
               "padded_token_is_zero", "pad_row_of_head_0_for_every_head", "window_origin_transposed", "stale_kv_of_previous_item", "stale_v_only",
               "heads_rolled"}
