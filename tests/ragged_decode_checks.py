"""decode_attn with one position per sequence (llmseg_decode_attn_rows; generate(attention_mask=) runs on it): a case table, inputs, fp64 references,
emulations and mutants.  CPU only, no import of the HIP library.

The arithmetic is not restated here: the reference of a ragged case is tests/forward_kernel_checks.py::decode_compute applied row by row to one-row
slices (a sequence at position pos_n is the scalar problem N = 1, pos = pos_n), the emulation is its emulation, and the bounds are the per-element
bounds its outputs take there (bf16_bound on `out` and on the new k row, zero on every other cache element).  Inputs follow decode_inputs with the
sentinel placed per row: the caches hold NaN beyond EACH ROW'S OWN position, so a row that reads a key it does not own returns NaN, and slot pos_n
holds a stale finite row, so a row that attends to the slot's old content instead of the appended token returns a finite wrong number.

Mutants are fp64 results of the ways a per-row position can go wrong (a row that takes another row's position for all or for part of what follows
from it); tests/test_ragged_decode_cpu.py proves that the bounds reject each by MUT_MIN on every case it applies to."""
import functools

import torch

from tests import forward_kernel_checks as fk
from tests.forward_kernel_checks import CAP, EMU_MAX, HD, MUT_MIN, Case, decode_compute, decode_scratch_floats, decode_splits, ratio      # noqa: F401  (re-exported)

BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")
OUTPUTS = ("out", "kc", "vc")          # `qkv` of decode_compute is rope_kv_append's in-place operand: decode_attn leaves its qkv alone


def cases():
    """(the split count follows decode_splits) one key / 17 keys with 14 empty splits / the full cache in one launch; two rows on the 16-split route; 8 splits;
    N * heads > 256: one split; no scratch; a scratch that holds 5 of the 16 splits; scores up to +/-60"""
    out = []
    for name, kw in (("N3_h2", dict(N=3, heads=2, pos=(0, 16, 129))), ("N2_h2", dict(N=2, heads=2, pos=(15, 31))), ("N4_h8", dict(N=4, heads=8, pos=(7, 8, 63, 129))),
                     ("N5_h64", dict(N=5, heads=64, pos=(3, 64, 65, 128, 17))), ("N2_h2_noscratch", dict(N=2, heads=2, pos=(129, 0), scratch="none")),
                     ("N1_h2_smallscratch", dict(N=1, heads=2, pos=(129,), scratch="small")), ("N2_h4_scores60", dict(N=2, heads=4, pos=(129, 40), qscale=25.0))):
        kw = {"scratch": "full", "qscale": 1.0, **kw}
        assert len(kw["pos"]) == kw["N"] and all(0 <= p < CAP for p in kw["pos"])
        c = Case("decode_rows", name, 0, **kw)
        c.launches = 2 if splits(c) > 1 else 1                     # decode_attn (+ its merge)
        out.append(c)
    return out


def splits(case):
    return decode_splits(case.N, case.heads, decode_scratch_floats(case))


def inputs(case):
    g = fk._g(case)
    N, D = case.N, case.heads * HD
    qkv = torch.randn(N, 3 * D, generator=g)
    qkv[:, :D] *= case.qscale
    ang = torch.rand(CAP, HD // 2, generator=g) * 6.28
    kc, vc = torch.randn(N, CAP, D, generator=g), torch.randn(N, CAP, D, generator=g)
    for n, p in enumerate(case.pos):                       # beyond the row's own position: NaN (never read); slot pos_n holds a stale finite row
        kc[n, p + 1:], vc[n, p + 1:] = NAN, NAN
    return dict(qkv=qkv.to(BF), cos=ang.cos().float().contiguous(), sin=ang.sin().float().contiguous(), kc=kc.to(BF), vc=vc.to(BF), scale=HD ** -0.5)


def _row(case, inp, n, pos, mut=None, emu=None):
    """decode_compute on sequence n alone at position `pos` -> (outputs, exact masks), each with a leading dimension of one row"""
    one = Case("decode", f"{case.name}_row{n}", 0, N=1, heads=case.heads, pos=int(pos), scratch=case.scratch, qscale=case.qscale)
    sub = dict(inp, qkv=inp["qkv"][n:n + 1], kc=inp["kc"][n:n + 1], vc=inp["vc"][n:n + 1])
    return decode_compute(one, sub, mut=mut, emu=emu)


def compute(case, inp, positions=None, muts=None, emu=None):
    """row n at positions[n] (default: its own) with the decode_compute mutant muts[n] (default: none) -> ({out, kc, vc}, exact masks of kc and vc)"""
    positions = case.pos if positions is None else positions
    rows = [_row(case, inp, n, positions[n], mut=None if muts is None else muts[n], emu=emu) for n in range(case.N)]
    got = {k: torch.cat([r[0][k] for r in rows], 0) for k in OUTPUTS}
    exact = {k: torch.cat([r[1]["exact:" + k] for r in rows], 0) for k in ("kc", "vc")}
    return got, exact


@functools.lru_cache(maxsize=8)
def reference(case):
    """-> (inputs, fp64 reference {out [N, D], kc, vc [N, CAP, D]}, per-element bounds); built once per case and shared: callers must not write to it"""
    inp = inputs(case)
    ref, exact = compute(case, inp)
    bounds = {}
    for k, r in ref.items():                                # the rule of forward_kernel_checks.reference for a bf16 output
        b = torch.where(r == 0, torch.zeros_like(r), torch.nan_to_num(fk.bf16_bound(r), nan=0.0))
        bounds[k] = torch.where(exact[k], torch.zeros_like(b), b) if k in exact else b
    return inp, ref, bounds


def ratios(got, ref, bounds):
    return {k: ratio(got[k], ref[k], bounds[k]) for k in OUTPUTS}


def emulation_ratios(case):
    inp, ref, bounds = reference(case)
    got, _ = compute(case, inp, emu=True)
    return ratios(got, ref, bounds)


def _swapped(pos):
    p = list(pos)
    for i in range(0, len(p) - 1, 2):
        p[i], p[i + 1] = p[i + 1], p[i]
    return tuple(p)


def mutant_names(case):
    pos = case.pos
    m = []
    if any(p != pos[0] for p in pos):
        m += ["row0_pos_for_every_row", "longest_pos_for_every_row", "rope_at_row_pos_keys_of_longest_row"]      # (some row is shorter than the longest)
    if _swapped(pos) != tuple(pos):
        m.append("neighbour_rows_swap_positions")
    if any(p + 1 < CAP for p in pos):
        m.append("append_at_row_pos_plus_1")
    if case.qscale == 1.0:                                 # scores of sigma 25: the softmax is all but one-hot on some other key (forward_kernel_checks.decode_mutants)
        m += ["key_pos_excluded_per_row", "stale_cache_row_used_for_pos_per_row"]
    return m


def mutant(case, inp, name):
    N, pos = case.N, case.pos
    if name == "row0_pos_for_every_row":
        return compute(case, inp, positions=(pos[0],) * N)[0]
    if name == "longest_pos_for_every_row":
        return compute(case, inp, positions=(max(pos),) * N)[0]
    if name == "neighbour_rows_swap_positions":
        return compute(case, inp, positions=_swapped(pos))[0]
    if name == "rope_at_row_pos_keys_of_longest_row":
        # angle and cache slot are the row's own, so the caches are right; the key range 0 .. max(pos) of a shorter row takes in slots beyond its
        # position, which hold NaN: one NaN score makes the running max, and with it every weight and every element of the row's output, NaN
        got = compute(case, inp)[0]
        for n in range(N):
            if pos[n] < max(pos):
                assert bool(torch.isnan(inp["kc"][n, pos[n] + 1:max(pos) + 1].float()).all())
                got["out"][n] = NAN
        return got
    per_row = {"append_at_row_pos_plus_1": "k_written_at_pos_plus_1", "key_pos_excluded_per_row": "key_pos_excluded",
               "stale_cache_row_used_for_pos_per_row": "stale_cache_row_used_for_pos"}[name]
    muts = [per_row if (name != "append_at_row_pos_plus_1" or p + 1 < CAP) else None for p in pos]
    return compute(case, inp, muts=muts)[0]


def mutant_ratios(case):
    """mutant -> its worst tolerance ratio over the outputs against the fp64 reference"""
    inp, ref, bounds = reference(case)
    return {name: max(ratios(mutant(case, inp, name), ref, bounds).values()) for name in mutant_names(case)}
