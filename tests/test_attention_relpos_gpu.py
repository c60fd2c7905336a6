"""GPU: every attention route that SAM's image encoder can take (14 x 14 windows through the rel-pos tables on each of the three window
kernels and the tiled kernel, their persistent loop at forced workgroup counts, o_row_map, the window gather, and the rel_h / rel_w grids up to
the 64-wide LDS-DMA kernel) against fp64 references, under the local tolerance that tests/test_attention_relpos_cpu.py validates against a bf16
emulation and mutants.  Outputs are pre-filled with a NaN canary; profiles/attn_relpos_parity.md lists the dispatch condition behind every case."""
import time

import pytest
import torch

from tests import attention_relpos_checks as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
CASES = {c.name: c for c in ar.cases()}
CANARY = 0x7FA5               # a bf16 NaN: a row the kernel should have written fails the parity check, a row it should not have is compared bit for bit
GUARD = 8                     # canary rows in front of and behind every output
ROUTES = ("default", "variant1", "variant0", "lse", "kv_pitch")       # the five dispatches of the table route (see _window)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    t0 = time.time()
    yield
    _set_variant(2)
    print(f"\ntests/test_attention_relpos_gpu.py: {time.time() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _default_variant():
    """llmseg_attn_set_variant is process-global: back to the default after every test, passed or failed"""
    try:
        yield
    finally:
        _set_variant(2)


def _set_variant(variant, wgs=0):
    from llmseg_amd import _lib
    assert _lib.load().llmseg_attn_set_variant(variant | (wgs << 4)) == 0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _canary_out(rows, D):
    """-> (the whole buffer, its rows [GUARD, GUARD + rows) that the kernel is given), all canary"""
    buf = torch.full((rows + 2 * GUARD, D), CANARY, dtype=torch.int16, device=DEV).view(BF)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf):
    b = _bits(buf)
    return bool((b[:GUARD] == CANARY).all()) and bool((b[-GUARD:] == CANARY).all())


def _packed(q, k, v):
    """q, k, v [B, H, N, hd] (host) -> the model's q|k|v rows [B * N, 3 * H * hd] on the GPU"""
    B, H, N, hd = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B * N, H * hd) for t in (q, k, v)], 1).to(DEV)


def _heads_first(o, B, N, H, hd):
    """[B * N, H * hd] GPU -> [B, H, N, hd] host"""
    return o.view(B, N, H, hd).transpose(1, 2).cpu()


def _report(name, r):
    print(f"\n{name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{name}: error / bound > 1: {bad}"


def _window(case, P, route, out, row_map=None, wgs=0):
    """one launch of the table route on the windows P (q, k, v [B, H, 196, 80]) -> lse or None.
    default: attn_win14_dma_kernel<false>; variant1: attn_win14_kernel; variant0: attn_fwd_kernel<80, 4>; lse: the default variant with lse requested
    (attn_fwd_kernel<80, 4>); kv_pitch: the default variant with q, k, v as separate tensors whose K and V row pitches differ (attn_win14_kernel)"""
    from llmseg_amd import ops
    B, H, N, hd = P["q"].shape
    D = H * hd
    th, tw = (t.to(DEV) for t in ar.kernel_tables(P))
    kw = dict(rel_tab_h=th, rel_tab_w=tw, grid_hw=(ar.WS, ar.WS), o_row_map=None if row_map is None else row_map.to(DEV))
    lse = torch.full((B, H, N), float("nan"), device=DEV) if route == "lse" else None
    _set_variant({"variant1": 1, "variant0": 0}.get(route, 2), wgs)
    if route == "kv_pitch":
        q, k, v = (t.transpose(1, 2).reshape(B * N, D).to(DEV) for t in (P["q"], P["k"], P["v"]))
        kbuf = torch.zeros(B * N, D + 8, device=DEV, dtype=BF)
        kbuf[:, :D] = k
        ops.attention(q, kbuf, v, out, batch=B, heads=H, Nq=N, Nk=N, head_dim=hd, q_strides=(N * D, hd, D), k_strides=(N * (D + 8), hd, D + 8),
                      v_strides=(N * D, hd, D), o_strides=(N * D, hd, D), **kw)
    else:
        ops.attention_packed(_packed(P["q"], P["k"], P["v"]), B, N, H, hd, out=out, lse=lse, **kw)
    torch.cuda.synchronize()
    return lse


@pytest.mark.parametrize("route", ROUTES)
def test_window_routes(route):
    """win_b3_h2 (6 items) on each of the four kernels that the table route can take"""
    case = CASES["win_b3_h2"]
    P, (ro, rl), _ = ar.reference(case)
    buf, out = _canary_out(case.B * case.N, case.H * case.hd)
    lse = _window(case, P, route, out)
    r = {"o": ar.ratio(_heads_first(out, case.B, case.N, case.H, case.hd), ro)}
    if lse is not None:
        r["lse"] = ar.lse_ratio(lse.cpu(), rl)
    assert _guards_intact(buf)
    _report(f"{case.name} {route}", r)


@pytest.mark.parametrize("route", ROUTES)
def test_window_routes_row_map(route):
    """the same with o_row_map = the reversed rows, every 5th query skipped: mapped rows hold the query's output, every other row keeps the canary bit for bit"""
    case = CASES["win_b3_h2"]
    P, (ro, rl), _ = ar.reference(case)
    rows, D = case.B * case.N, case.H * case.hd
    rm = torch.arange(rows - 1, -1, -1, dtype=torch.int32)
    rm[::5] = -1
    keep = rm >= 0
    buf, out = _canary_out(rows, D)
    lse = _window(case, P, route, out, row_map=rm)
    got = out.cpu()
    ref = ro.transpose(1, 2).reshape(rows, case.H, case.hd)
    r = {"o": ar.ratio(got[rm[keep].long()].view(-1, case.H, case.hd), ref[keep])}
    if lse is not None:
        r["lse"] = ar.lse_ratio(lse.cpu(), rl)
    untouched = torch.ones(rows, dtype=torch.bool)
    untouched[rm[keep].long()] = False
    assert int(untouched.sum()) == int((~keep).sum())
    assert bool((_bits(got)[untouched] == CANARY).all()), "a row that no query maps to was written"
    assert _guards_intact(buf)
    _report(f"{case.name} {route} o_row_map", r)


@pytest.mark.parametrize("variant", [2, 1])
def test_persistent_loop(variant):
    """win_b5_h8 (40 items) on 8 workgroups (five rounds, XCD-grouped vwg) and on 6 (not a multiple of 8; 7 and 6 rounds): fp64 parity, and
    the same bits as the unforced launch (one round) -- an item's arithmetic does not depend on the workgroup or round that computes it"""
    case = CASES["win_b5_h8"]
    P, (ro, _), _ = ar.reference(case)
    route = {2: "default", 1: "variant1"}[variant]
    outs, r = {}, {}
    for wgs in (0, 8, 6):
        buf, out = _canary_out(case.B * case.N, case.H * case.hd)
        _window(case, P, route, out, wgs=wgs)
        assert _guards_intact(buf)
        outs[wgs] = out
        r[f"o(wgs={wgs or 'default'})"] = ar.ratio(_heads_first(out, case.B, case.N, case.H, case.hd), ro)
    _report(f"{case.name} variant {variant}", r)
    for wgs in (8, 6):
        assert _same_bits(outs[wgs], outs[0]), f"{wgs} workgroups: bits differ from the unforced launch"


def test_second_round_at_the_default():
    """win_b33_h8 (264 items): the balanced default takes 136 workgroups x 2 rounds"""
    case = CASES["win_b33_h8"]
    P, (ro, _), _ = ar.reference(case)
    buf, out = _canary_out(case.B * case.N, case.H * case.hd)
    _window(case, P, "default", out)
    assert _guards_intact(buf)
    _report(case.name, {"o": ar.ratio(_heads_first(out, case.B, case.N, case.H, case.hd), ro)})


@pytest.mark.parametrize("name,wgs", [("gather_g15", 0), ("gather_g27", 0), ("gather_g28", 0), ("gather_g29", 0), ("gather_g15_i3_h8", 8)])
def test_window_gather(name, wgs):
    """attn_win14_dma_kernel<true>: fp64 parity on the real tokens, the bits of the o_row_map route over the materialised padded windows, and nothing
    written outside the token rows.  g = 15: windows with a 14 x 1 strip and with a single real token; 96 items on 8 workgroups: the next-item
    prefetch crosses windows, heads and images."""
    from llmseg_amd import ops
    case = CASES[name]
    P, (ro, _), _ = ar.reference(case)
    B, H, N, hd, g = case.B, case.H, case.N, case.hd, case.g
    D, rows = H * hd, case.images * g * g
    src = P["src"]
    th, tw = (t.to(DEV) for t in ar.kernel_tables(P))
    kw = dict(rel_tab_h=th, rel_tab_w=tw, grid_hw=(ar.WS, ar.WS))
    buf_map, o_map = _canary_out(rows, D)
    ops.attention_packed(_packed(P["q"], P["k"], P["v"]), B, N, H, hd, out=o_map, o_row_map=src.reshape(-1).to(torch.int32).to(DEV), **kw)
    tok = torch.cat([P["tok_" + n].reshape(rows, D) for n in "qkv"], 1).to(DEV)
    pad = torch.cat([P["pad_" + n].reshape(D) for n in "qkv"]).to(DEV)
    buf_gat, o_gat = _canary_out(rows, D)
    _set_variant(2, wgs)
    ops.attention_packed(tok, B, N, H, hd, out=o_gat, win_pad=(g, pad), **kw)
    torch.cuda.synchronize()
    assert _guards_intact(buf_gat) and _guards_intact(buf_map)
    in_windows = lambda o: o.cpu().view(rows, H, hd)[src.clamp(min=0)].permute(0, 2, 1, 3)        # [B, H, 196, hd]; padding rows are not compared
    r = {"o": ar.rows_ratio(case, P, in_windows(o_gat), ro), "o(row map)": ar.rows_ratio(case, P, in_windows(o_map), ro)}
    _report(f"{name} wgs={wgs or 'default'}", r)
    assert _same_bits(buf_gat, buf_map), "window gather: bits differ from the o_row_map route over the padded windows"


ARR = [(c.name, False) for c in ar.cases() if c.kind == "arr"] + [(c.name, True) for c in ar.cases() if c.kind == "arr" and c.lse]


@pytest.mark.parametrize("name,want_lse", ARR, ids=[n + ("_lse" if l else "") for n, l in ARR])
def test_array_routes(name, want_lse):
    """rel_h / rel_w as fp32 [heads][batch * Nq][rel_ld] arrays whose meaningless columns are NaN"""
    from llmseg_amd import ops
    case = CASES[name]
    P, (ro, rl), (Gh, Gw) = ar.reference(case)
    B, H, N, hd = case.B, case.H, case.N, case.hd
    rel_h, rel_w = (t.to(DEV) for t in ar.rel_arrays(case, Gh, Gw))
    buf, out = _canary_out(B * N, H * hd)
    lse = torch.full((B, H, N), float("nan"), device=DEV) if want_lse else None
    ops.attention_packed(_packed(P["q"], P["k"], P["v"]), B, N, H, hd, out=out, rel_h=rel_h, rel_w=rel_w, rel_ld=case.rel_ld, grid_hw=(case.gh, case.gw),
                         lse=lse)
    torch.cuda.synchronize()
    r = {"o": ar.ratio(_heads_first(out, B, N, H, hd), ro)}
    if want_lse:
        r["lse"] = ar.lse_ratio(lse.cpu(), rl)
    assert _guards_intact(buf)
    _report(name + (" lse" if want_lse else ""), r)
