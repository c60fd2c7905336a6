"""CPU: the tolerances of tests/test_head_f32_gpu.py have teeth.  On every case of the shared table the fp32 emulation of what the fp32 head kernels
(llmseg_amd/csrc/head_f32.hip) round passes with a 2x margin, and every applicable mutant (an fp64 result of a subtly wrong problem) fails by at least
2x.  The table is held to the edges it was written for; two wrong emulations (a one-pass variance, a softmax without its maximum) are rejected; the
composed head's bound (4 x the fp32 oracle's own deviation from fp64) rejects three wrong heads; the restated inference tail reproduces the oracle's
model_forward; the four entry points refuse bad arguments before any launch.  Run with -s to see each case's ratios and the per-mutant summary."""
import ctypes as C
import time

import pytest
import torch

from tests import head_f32_checks as hk

CASES = hk.cases()
_SEEN = {}
_T0 = time.time()

# every mutant that must apply somewhere in the table, per entry point
MUTANTS = {
    "linear": {"k_tail_dropped", "last_row_dropped", "last_col_dropped", "alpha_on_bias", "residual_before_act", "bias_indexed_by_row", "layout_swapped", "ldx_taken_as_K",
               "ldr_taken_as_N", "tanh_gelu", "quickgelu_constant_1"},
    "layernorm": {"eps_dropped", "unbiased_variance", "last_lane_group_dropped", "last_row_dropped", "bias_dropped"},
    "attn": {"last_key_dropped", "last_stage_dropped", "stage_padding_counted", "scale_missing", "batch_reads_batch0_keys", "heads_permuted", "v_read_from_k_columns"},
    "cosine": {"target_norm_missing", "last_row_dropped", "last_lane_group_dropped"},
}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\nratio to the bound over the table (mutants: weakest, must be >= %g; emulation: worst, must be <= %g)" % (hk.MUT_MIN, hk.EMU_MAX))
        for n in sorted(_SEEN):
            emu = " emulation " in n
            r, where = (max if emu else min)(_SEEN[n])
            print(f"  {n:55s} {r:12.3f}  at {where}  ({len(_SEEN[n])} cases)")
    print(f"tests/test_head_f32_cpu.py: {time.time() - _T0:.1f} s")


def _case(name):
    return next(c for c in CASES if c.name == name)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_mutants_fail(case):
    emu = hk.emulation_ratios(case)
    mut = hk.mutant_ratios(case)
    for n, r in emu.items():
        _SEEN.setdefault(f"{case.op} emulation {n}", []).append((r, case.name))
    for n, r in mut.items():
        _SEEN.setdefault(f"{case.op} {n}", []).append((r, case.name))
    print(f"\n{case.name}: emulation " + " ".join(f"{n}={r:.3f}" for n, r in emu.items()) +
          " | mutants " + " ".join(f"{n}={r:.3g}" for n, r in sorted(mut.items(), key=lambda x: x[1])))
    assert all(r <= hk.EMU_MAX for r in emu.values()), f"an emulation exceeds {hk.EMU_MAX} of the bound: {emu}"
    assert mut, "no mutant applies to this case"
    weak = {n: r for n, r in mut.items() if not r >= hk.MUT_MIN}
    assert not weak, f"mutants the tolerance does not reject by {hk.MUT_MIN}x: {weak}"


def test_every_mutant_applies_somewhere():
    """every mutant of the list applies to at least one case of its entry point, and no case is left without one"""
    seen = {}
    for c in CASES:
        names = hk.mutant_names(c)
        assert names, c
        seen.setdefault(c.op, set()).update(names)
    assert seen == MUTANTS, {op: (seen.get(op, set()) ^ MUTANTS.get(op, set())) for op in set(seen) | set(MUTANTS) if seen.get(op) != MUTANTS.get(op)}


def test_table_reaches_both_sides_of_every_edge():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names) and all(c.launches == 1 for c in CASES)
    lin = [c for c in CASES if c.op == "linear"]
    # 64 x 64 tiles: below, at, above one tile and more than two; the K step of 16 likewise; each in both weight layouts
    for kn in (0, 1):
        sub = [c for c in lin if c.kn == kn]
        assert any(c.M > hk.LT and c.M % hk.LT for c in sub) and any(c.N > hk.LT and c.N % hk.LT for c in sub) and any(c.M < hk.LT for c in sub) and any(c.N < hk.LT for c in sub), kn
        assert any(c.K > hk.LK and c.K % hk.LK for c in sub) and any(c.K % hk.LK == 0 for c in sub) and any(c.K < hk.LK for c in sub), kn
    assert {c.M for c in lin} >= {1, 63, 64, 65, 130} and {c.N for c in lin} >= {1, 63, 64, 65, 130} and {c.K for c in lin} >= {1, 15, 16, 17, 50}
    assert any(c.M > hk.LT and c.N > hk.LT and c.K > hk.LK and c.K % hk.LK for c in lin)
    acts = [c for c in lin if (c.M, c.N, c.K) == (33, 65, 17) and c.wide]
    assert {c.act for c in acts} == set(hk.ACTS) and {hk.ACTS[a] for a in hk.ACTS} == set(range(6))
    for c in acts:                                              # pre-activations reach the saturated ends
        inp, ref, _ = hk.reference(c)
        if c.act == "none" and not c.res:
            assert float(ref["y"].nan_to_num().abs().max()) >= 11.0
    assert any(c.alpha == 0.5 and c.bias and c.res for c in lin)
    assert any(c.ldx == 5 for c in lin) and any(c.ldr == 3 and c.res for c in lin) and any(c.ldy == 3 for c in lin)
    assert {(c.kn, c.wslice) for c in lin if c.wslice} == {(0, "row"), (0, "col"), (1, "row"), (1, "col")}
    for kn in (0, 1):                                          # every leading dimension at once, per layout
        assert any(c.kn == kn and c.ldx and c.ldr and c.ldy and c.wslice for c in lin)
    assert {(c.M, c.N, c.K, c.kn, c.act, c.res) for c in lin} >= {(3, 256, 4096, 0, "relu", 0), (130, 768, 256, 0, "none", 0), (130, 2048, 256, 0, "relu", 0),
                                                                (130, 256, 2048, 0, "none", 1), (20, 256, 4096, 1, "none", 0)}
    for c in lin:                                              # the slack of every strided operand is there, and is finite
        inp = hk.reference(c)[0]
        assert inp["x"].shape == (c.M, c.K + c.ldx) and bool(torch.isfinite(inp["x"]).all()) and bool(torch.isfinite(inp["wbuf"].float()).all())
        assert hk.weight_view(c, inp).shape == ((c.K, c.N) if c.kn else (c.N, c.K)) and inp["wbuf"].stride(0) == hk.weight_view(c, inp).shape[1] + (6 if c.wslice else 0)
    ln = [c for c in CASES if c.op == "layernorm"]
    assert {c.rows for c in ln} == {1, 3, 4, 5, 130} and {c.D for c in ln} == {1, 8, 63, 64, 65, 100, 256} and {c.bias for c in ln} == {0, 1}
    assert {c.kind for c in ln} == {"", "const", "offset"} and any(c.kind == "offset" and c.D == 256 for c in ln)
    at = [c for c in CASES if c.op == "attn"]
    assert {(c.B, c.H, c.Nq, c.Nk, c.hd) for c in at} >= {(1, 1, 1, 1, 32), (2, 8, 1, 65, 32), (3, 8, 130, 130, 32), (1, 2, 127, 63, 64), (1, 2, 128, 64, 64),
                                                           (2, 2, 129, 65, 64), (1, 8, 64, 130, 32)}
    assert _case("attn-B2_H8_q1_k65_hd32_cross").layout == "kv" and _case("attn-B3_H8_q130_k130_hd32_self").layout == "qkv"
    c = _case("attn-B1_H8_q64_k130_hd32_scale_ldo")
    assert c.ldo > 0 and abs(hk.attn_scale(c) - c.hd ** -0.5) > 0.05
    assert {c.peak for c in at if c.Nk == 130} >= {"first", "last"}
    # the partial last key stage and query workgroup from both sides
    assert {c.Nk % hk.KSTAGE for c in at} >= {0, 1, 2, 63} and {c.Nq for c in at} >= {hk.QWG - 1, hk.QWG, hk.QWG + 1}
    assert {(c.K, c.D) for c in CASES if c.op == "cosine"} == {(1, 1), (3, 63), (4, 64), (5, 65), (130, 256)}


def test_peaked_attention_cases_move_the_maximum_as_they_claim():
    for name, last in (("attn-B1_H2_q5_k130_hd32_peak_last", True), ("attn-B1_H2_q5_k130_hd32_peak_first", False)):
        c = _case(name)
        inp = hk.reference(c)[0]
        s = (inp["q"].double() @ inp["k"].double().transpose(-1, -2)) * hk.attn_scale(c)
        assert float(s.max()) > 89.0 and float(s.min()) < -80.0, (float(s.max()), float(s.min()))
        run = torch.cummax(s, -1).values
        moves = (run[..., 1:] > run[..., :-1]).sum(-1)
        assert bool((moves == c.Nk - 1).all()) if last else bool((moves == 0).all()), moves
        r = hk.emulation_ratios(c, emu="no_max")["o"]                   # exp(s) without the maximum: e^90 overflows fp32
        got, _ = hk.attn_compute(c, inp, emu="no_max")
        assert not bool(torch.isfinite(got["o"][:, :c.H * c.hd]).all()) and r == float("inf"), r


def test_one_pass_variance_misses_the_bound_on_the_offset_row():
    c = _case("layernorm-5x256_bias_offset")
    two, one = hk.emulation_ratios(c)["y"], hk.emulation_ratios(c, emu="one_pass")["y"]
    print(f"\n{c.name}: two-pass emulation {two:.3f}, one-pass E[x^2] - mean^2 {one:.3f}")
    assert two <= hk.EMU_MAX and one >= hk.MUT_MIN


def test_constant_row_gives_the_bias_and_special_cosine_rows_stay_in_range():
    for c in (c for c in CASES if c.op == "layernorm" and c.kind == "const"):
        inp, ref, _ = hk.reference(c)
        want = inp["b"].double() if inp["b"] is not None else torch.zeros(c.D, dtype=torch.float64)
        emu, _ = hk.layernorm_compute(c, inp, emu=True)
        assert torch.equal(ref["y"][hk.CONST_ROW], want) and torch.equal(emu["y"][hk.CONST_ROW], want)
    c = _case("layernorm-1x1_bias")
    inp, ref, _ = hk.reference(c)
    assert torch.equal(ref["y"][0], inp["b"].double())                  # D = 1: the row is its own mean
    for c in (c for c in CASES if c.op == "cosine"):
        inp, ref, bounds = hk.reference(c)
        same, opp, zero = hk.cosine_rows(c)
        emu, _ = hk.cosine_compute(c, inp, emu=True)
        nan = torch.isnan(ref["sim"])
        assert nan.tolist() == [k == zero for k in range(c.K)] and torch.isnan(emu["sim"]).tolist() == nan.tolist()
        if same is not None:
            assert abs(float(ref["sim"][same]) - 1.0) < 1e-12 and abs(float(ref["sim"][opp]) + 1.0) < 1e-12
            assert bool((emu["sim"][[same, opp]].abs() <= 1.0 + bounds["sim"][[same, opp]]).all())
    assert {hk.cosine_rows(c)[2] is not None for c in CASES if c.op == "cosine"} == {True, False}


# --------------------------------------------------------------------------------------------------------------- the composed head
@pytest.mark.parametrize("CK", hk.HEAD_CASES, ids=[f"C{c}_K{k}" for c, k in hk.HEAD_CASES])
def test_head_bound_rejects_wrong_heads(CK):
    C_, K = CK
    ref, dev, bound = hk.head_reference(C_, K)
    sd, pooled, text = hk.head_inputs(C_, K)
    again = dict(zip(("iou", "emb"), hk.head_oracle(sd, pooled, text, torch.float64, restated=True)))
    assert torch.equal(again["iou"], ref["iou"]) and torch.equal(again["emb"], ref["emb"]), "the restatement the mutants are built from is not the oracle"
    names = hk.head_mutant_names(C_, K)
    assert names
    line = []
    for m in names:
        got = dict(zip(("iou", "emb"), hk.head_oracle(sd, pooled, text, torch.float64, m)))
        r = hk.head_ratios(got, ref, bound)
        line.append(f"{m} iou={r['iou']:.3g} emb={r['emb']:.3g}")
        assert min(r.values()) >= hk.MUT_MIN, (m, r)
    print(f"\nhead C={C_} K={K}: fp32-oracle deviation iou {dev['iou']:.2e} emb {dev['emb']:.2e} | " + " | ".join(line))
    assert 0.0 < dev["iou"] < 1e-6 and 0.0 < dev["emb"] < 1e-5, dev      # the oracle's own fp32 arithmetic: what the bound is 4 x of


def test_every_head_mutant_applies_somewhere():
    assert {m for c, k in hk.HEAD_CASES for m in hk.head_mutant_names(c, k)} == set(hk.HEAD_MUTANTS)
    assert {k % hk.KSTAGE for _, k in hk.HEAD_CASES} >= {0, 1, 2} and {c for c, _ in hk.HEAD_CASES} == {1, 2, 3}


def test_restated_tail_reproduces_the_oracle_forward():
    """the inference tail as tests/test_head_f32_gpu.py restates it from `feats` and `hidden` gives what oracle.lisa.model_forward computes from the same two
    tensors (fp32: the same operations), and the empty proposal pools to exact zeros"""
    from oracle import cases, lisa as olisa
    cfg = cases.tiny_lisa_cfg("sam")
    sd = {k: v.to(torch.bfloat16).float() for k, v in cases.tiny_lisa_state(cfg, 3).items()}
    batch = hk.tail_batch(cfg)
    assert hk.TAIL_K % hk.KSTAGE and not bool(batch["sam_segs_list"][0][hk.TAIL_ZERO].any())
    with torch.no_grad():
        ref = olisa.model_forward(sd, cfg, **batch, inference=True, return_aux=True)
    _, D, g, _ = ref["feats"].shape
    cl = ref["feats"][0].permute(1, 2, 0).reshape(g * g, D)
    out = hk.tail_oracle(sd, cl, ref["hidden"], batch["input_ids"], batch["sam_segs_list"][0], cfg.seg_token_idx, torch.float32)
    assert out["pred_similarity"].shape == (2, hk.TAIL_K) and out["pred_iou"].shape == (1, hk.TAIL_K)
    tol = 5e-6                                                  # the same fp32 operations on other matrix shapes (the oracle runs text_hidden_fcs on every row): 2e-7 measured; a wrong wiring is wrong by 1e-2
    assert float((out["pred_embeddings"] - ref["pred_embeddings"][0]).abs().max()) <= tol
    assert float((out["pred_similarity"] - ref["pred_similarity"][0]).abs().max()) <= tol and float((out["pred_iou"] - ref["pred_iou"][0]).abs().max()) <= tol
    assert float(out["pooled"][hk.TAIL_ZERO].abs().max()) == 0.0 and bool(torch.isfinite(out["pooled"]).all())


# ------------------------------------------------------------------------------------------------------------------- argument checks
def _refused(lib, name, fn, order, ok, bads):
    n0 = lib.llmseg_launch_count()
    for bad in bads:
        a = dict(ok, **bad)
        rc = fn(*[a[k] for k in order])
        assert rc == -1 and name.encode() in lib.llmseg_last_error(), (name, bad, rc, lib.llmseg_last_error())
    assert lib.llmseg_launch_count() == n0


def test_linear_f32_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    order = ("x", "ldx", "W", "ldw", "w_kn", "bias", "residual", "ldr", "y", "ldy", "M", "N", "K", "act", "alpha", "stream")
    ok = dict(x=p(4096), ldx=5, W=p(4096), ldw=5, w_kn=0, bias=None, residual=None, ldr=0, y=p(4096), ldy=8, M=3, N=8, K=5, act=0, alpha=1.0, stream=None)
    bads = [dict(x=None), dict(W=None), dict(y=None), dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(K=-5), dict(ldx=4), dict(ldy=7), dict(ldw=4),
            dict(w_kn=1, ldw=7), dict(residual=p(4096), ldr=7), dict(act=-1), dict(act=6)]
    _refused(lib, "linear_f32", lib.llmseg_linear_f32, order, ok, bads)


def test_layernorm_f32_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    order = ("x", "w", "b", "y", "rows", "D", "eps", "stream")
    ok = dict(x=p(4096), w=p(4096), b=None, y=p(4096), rows=3, D=8, eps=1e-5, stream=None)
    _refused(lib, "layernorm_f32", lib.llmseg_layernorm_f32, order, ok, [dict(x=None), dict(w=None), dict(y=None), dict(rows=0), dict(rows=-2), dict(D=0), dict(D=-1)])


def test_attn_f32_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    order = ("q", "k", "v", "o", "strides", "batch", "heads", "Nq", "Nk", "head_dim", "scale", "stream")
    st = (C.c_int64 * 12)(*([64, 32, 64] * 4))
    ok = dict(q=p(4096), k=p(4096), v=p(4096), o=p(4096), strides=st, batch=1, heads=2, Nq=1, Nk=1, head_dim=32, scale=0.1, stream=None)
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(strides=None), dict(batch=0), dict(heads=0), dict(Nq=0), dict(Nk=0), dict(Nk=-3),
            dict(head_dim=48), dict(head_dim=128)]
    _refused(lib, "attn_f32", lib.llmseg_attn_f32, order, ok, bads)


def test_cosine_f32_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    order = ("t", "e", "sim", "K", "D", "stream")
    ok = dict(t=p(4096), e=p(4096), sim=p(4096), K=3, D=8, stream=None)
    _refused(lib, "cosine_f32", lib.llmseg_cosine_f32, order, ok, [dict(t=None), dict(e=None), dict(sim=None), dict(K=0), dict(D=0), dict(K=-1)])


def test_strided_view_check_of_attention_f32():
    """ops.attention_f32 asserts that each of its four strided views lies inside its tensor's storage: the head's own stride tuples pass, a tuple one row,
    one head or one batch too far does not"""
    from llmseg_amd import ops
    for c in (c for c in CASES if c.op == "attn"):
        q, k, v, o, (qs, ks, vs, os_) = hk.attn_buffers(c, hk.reference(c)[0])
        for t, st, rows in ((q, qs, c.Nq), (k, ks, c.Nk), (v, vs, c.Nk), (o, os_, c.Nq)):
            assert ops.strided_view_fits(t, st, c.B, c.H, rows, c.hd), (c, st)
            assert not ops.strided_view_fits(t, st, c.B, c.H, rows + 1, c.hd), (c, st)
            assert not ops.strided_view_fits(t, st, c.B + 1, c.H, rows, c.hd), (c, st)
            assert not ops.strided_view_fits(t, (st[0], st[1], -st[2]), c.B, c.H, rows, c.hd)
        assert not ops.strided_view_fits(v, vs, c.B, c.H + 1, c.Nk, c.hd)                      # v ends its buffer: one head further leaves it
        if c.layout == "kv" and c.B > 1:                                                       # the k | v batch stride handed to q [B * Nq, D]
            assert not ops.strided_view_fits(q, ks, c.B, c.H, c.Nq, c.hd)
