"""GPU: the fused attention forward (attn_fwd_kernel, lse included) and backward (attn_bwd_all_kernel) against fp64 references at ragged
key masks and tile edges, under the local tolerance that tests/test_attention_edges_cpu.py validates against a bf16 emulation and
mutants; padding invariance and fully masked sequences bit for bit; the fused RoPE store of the backward on ragged batches."""
import time

import pytest
import torch

from tests import attention_edge_checks as ae

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
CASES = ae.cases()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    t0 = time.time()
    yield
    print(f"\ntests/test_attention_edges_gpu.py: {time.time() - t0:.1f} s")


def _dev_rows(t):
    """[B, H, N, hd] host -> [B, N, H, hd] contiguous on the GPU (the packed row layout of the model)"""
    return t.transpose(1, 2).contiguous().to(DEV)


def _st(t):
    """(batch, head, row) strides of a [B, N, H, hd] tensor"""
    return (t.stride(0), t.stride(2), t.stride(1))


def _host(t):
    """[B, N, H, hd] GPU -> [B, H, N, hd] host"""
    return t.transpose(1, 2).cpu()


def fwd(q, k, v, key_mask, causal, nk_valid=None):
    """q, k, v [B, H, N, hd] bf16 (host).  Self attention runs through ops.attention_packed (q|k|v rows), the rest through ops.attention.
    -> o [B, Nq, H, hd], lse [B, H, Nq], (q, k, v) as [B, N, H, hd] device views"""
    from llmseg_amd import ops
    B, H, Nq, hd = q.shape
    Nk = k.shape[2]
    lse = torch.full((B, H, Nq), float("nan"), device=DEV)
    km = None if key_mask is None else key_mask.to(DEV)
    if Nq == Nk and nk_valid is None:
        qkv = torch.cat([t.transpose(1, 2).reshape(B * Nq, H * hd) for t in (q, k, v)], 1).to(DEV)
        o = ops.attention_packed(qkv, B, Nq, H, hd, causal=causal, key_mask=km, lse=lse)
        x = qkv.view(B, Nq, 3, H, hd)
        return o.view(B, Nq, H, hd), lse, (x[:, :, 0], x[:, :, 1], x[:, :, 2])
    qd, kd, vd = _dev_rows(q), _dev_rows(k), _dev_rows(v)
    o = torch.full((B, Nq, H, hd), float("nan"), device=DEV, dtype=BF)
    nk = None if nk_valid is None else torch.tensor([nk_valid], dtype=torch.int32, device=DEV)
    ops.attention(qd, kd, vd, o, batch=B, heads=H, Nq=Nq, Nk=Nk, head_dim=hd, q_strides=_st(qd), k_strides=_st(kd), v_strides=_st(vd),
                  o_strides=_st(o), causal=causal, key_mask=km, lse=lse, nk_dev=nk)
    return o, lse, (qd, kd, vd)


def bwd(x, o, do, lse, key_mask, causal, rope=None):
    """-> dq, dk, dv as [B, N, H, hd] (pre-filled with NaN: a row the kernel does not write fails every check)"""
    from llmseg_amd import ops
    qd, kd, vd = x
    B, Nq, H, hd = qd.shape
    Nk = kd.shape[1]
    dq = torch.full((B, Nq, H, hd), float("nan"), device=DEV, dtype=BF)
    dk = torch.full((B, Nk, H, hd), float("nan"), device=DEV, dtype=BF)
    dv = torch.full((B, Nk, H, hd), float("nan"), device=DEV, dtype=BF)
    ops.attention_bwd(qd, kd, vd, o, do, dq, dk, dv, lse, batch=B, heads=H, Nq=Nq, Nk=Nk, head_dim=hd, q_strides=_st(qd), k_strides=_st(kd),
                      v_strides=_st(vd), o_strides=_st(o), do_strides=_st(do), dq_strides=_st(dq), dk_strides=_st(dk), dv_strides=_st(dv),
                      causal=causal, key_mask=None if key_mask is None else key_mask.to(DEV), rope=rope)
    return dq, dk, dv


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_parity_with_fp64(case):
    """o and lse (forward), dq / dk / dv (backward, dO random, lse and O from the forward) within the validated local tolerance"""
    (q, k, v, do), (ro, rl), _ = ae.reference(case)
    km = case.key_mask()
    o, lse, x = fwd(q, k, v, km, case.causal, case.nk_valid)
    r = {"o": ae.ratio(_host(o), ro), "lse": ae.lse_ratio(lse.cpu(), rl)}
    if case.bwd:
        g = bwd(x, o, _dev_rows(do), lse, km, case.causal)
        ref = ae.attn_bwd_ref(q, k, v, case.scale, case.causal, km, do, case.nk_valid, o=_host(o))
        r.update(ae.grad_ratios([_host(t) for t in g], ref))
        if km is not None:       # a padded key gets exactly no gradient
            pad = (km == 0).to(DEV)
            assert bool((g[1][pad] == 0).all()) and bool((g[2][pad] == 0).all()), f"{case.name}: masked keys' dk / dv rows not exactly zero"
    print(f"\n{case.name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"


@pytest.mark.parametrize("hd,L,T2,causal", [(128, 300, 319, True), (64, 65, 129, False), (32, 63, 64, True), (128, 128, 257, True),
                                            (64, 1030, 1100, False)])
def test_padding_invariance_bits(hd, L, T2, causal):
    """a sequence of length L alone (T = L, no mask) and right-padded to T2 inside a ragged batch give the same bits: o and lse rows < L,
    dq / dk / dv rows < L (dO rows >= L zero); its dq / dk / dv rows >= L are exactly zero.  (T = L and T2 take the same forward route.)"""
    case = ae.Case(f"inv_{hd}_{L}_{T2}_{int(causal)}", hd, 3, 2, T2, T2, causal, [T2, L, T2 - 1])
    q, k, v, do = ae.make_inputs(case)
    do[1, :, L:] = 0
    km = case.key_mask()
    o, lse, x = fwd(q, k, v, km, causal)
    g = bwd(x, o, _dev_rows(do), lse, km, causal)
    one = lambda t: t[1:2, :, :L].contiguous()
    o1, lse1, x1 = fwd(one(q), one(k), one(v), None, causal)
    g1 = bwd(x1, o1, _dev_rows(one(do)), lse1, None, causal)
    assert _same_bits(o[1:2, :L], o1), "forward o rows < L"
    assert _same_bits(lse[1:2, :, :L], lse1), "lse rows < L"
    for n, a, b in zip(("dq", "dk", "dv"), g, g1):
        assert _same_bits(a[1:2, :L], b), f"{n} rows < L"
        assert bool((a[1, L:] == 0).all()), f"{n} rows >= L not exactly zero"


@pytest.mark.parametrize("hd,T,causal", [(128, 200, True), (64, 130, False)])
def test_fully_masked_sequence(hd, T, causal):
    """one batch entry with an all-zero key mask: its o is 0 and its lse finite, its dq / dk / dv are exactly zero (dO = 0 there), and the
    other sequences' outputs and gradients are bit-identical to a batch without it"""
    case = ae.Case(f"empty_{hd}_{T}_{int(causal)}", hd, 3, 2, T, T, causal, [T, 0, 77])
    q, k, v, do = ae.make_inputs(case)
    do[1] = 0
    km = case.key_mask()
    o, lse, x = fwd(q, k, v, km, causal)
    g = bwd(x, o, _dev_rows(do), lse, km, causal)
    assert bool(torch.isfinite(lse[1]).all()), "lse of the fully masked sequence"
    assert bool((o[1] == 0).all()), "o of the fully masked sequence"
    for n, t in zip(("dq", "dk", "dv"), g):
        assert bool((t[1] == 0).all()), f"{n} of the fully masked sequence"
    keep = [0, 2]
    o2, lse2, x2 = fwd(q[keep], k[keep], v[keep], km[keep], causal)
    g2 = bwd(x2, o2, _dev_rows(do[keep]), lse2, km[keep], causal)
    assert _same_bits(o[keep], o2) and _same_bits(lse[keep], lse2)
    for n, a, b in zip(("dq", "dk", "dv"), g, g2):
        assert _same_bits(a[keep], b), n


@pytest.mark.parametrize("hd,T", [(64, 129), (128, 257)])
def test_fused_rope_store_bits_ragged(hd, T):
    """rope= on attention_bwd (the inverse rotation inside the dq / dk store) == a separate ops.rope_ over the stored gradient, bit for bit,
    on a causal batch with ragged right padding"""
    from llmseg_amd import ops
    case = ae.Case(f"rope_{hd}_{T}", hd, 4, 2, T, T, True, ae.ragged_lens(T)[:4])
    q, k, v, do = ae.make_inputs(case)
    km = case.key_mask()
    o, lse, x = fwd(q, k, v, km, True)
    ang = torch.outer(torch.arange(T).float(), 1.0 / (10000 ** (torch.arange(0, hd, 2).float() / hd)))
    cos, nsin = ang.cos().contiguous().to(DEV), (-ang.sin()).contiguous().to(DEV)
    dod = _dev_rows(do)
    fused = bwd(x, o, dod, lse, km, True, rope=(cos, nsin))
    dq, dk, dv = bwd(x, o, dod, lse, km, True)
    for t in (dq, dk):
        ops.rope_(t, cos, nsin, 4 * T, T, 2, hd, 2 * hd)
    for n, a, b in zip(("dq", "dk", "dv"), fused, (dq, dk, dv)):
        assert _same_bits(a, b), n
