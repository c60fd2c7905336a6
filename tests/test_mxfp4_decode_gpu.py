"""GPU: MXFP4 weight-only decode.  The quantiser kernel bit for bit against the torch restatement of its public arithmetic (packed bytes, scale bytes, W^)
between canaries; llmseg_gemm_mxfp4 on every case of tests/mxfp4_checks.py against fp64 references under the per-element bounds tests/test_mxfp4_decode_cpu.py
validates, and refused calls that launch and write nothing; generate(weight_format="mxfp4") against ONE teacher-forced cache-free oracle forward on an
independently quantised state dict, on the greedy, ragged, sampling and beam routes; no state leaks between the bf16, the int8 and the MXFP4 mode."""
import collections
import ctypes as C
import functools

import pytest
import torch

from tests import mxfp4_checks as xc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
CASES = xc.cases()
GUARD = 64                     # canary elements either side of every output (a multiple of 16 bytes in every type used)
_WORST = collections.defaultdict(lambda: (0.0, ""))


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield
    print("\nworst error / bound per output type")
    for k in sorted(_WORST):
        print(f"  {k:8s} {_WORST[k][0]:.3f}  at {_WORST[k][1]}")


def _fault_guard(name, e):
    if "HIP error" in str(e) or "illegal memory access" in str(e):          # a device fault: nothing more may be started on this GPU
        pytest.exit(f"{name}: {e}", returncode=3)


def _guarded(name, fn):
    """fn() and a synchronisation; a device fault ends the session"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        _fault_guard(name, e)
        raise


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32 if t.dtype == F32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Guarded:
    """an output of [rows, cols] inside a canary-filled allocation: GUARD elements before it, padding columns up to the pitch, one more row and GUARD elements behind"""

    def __init__(self, rows, cols, pad, dtype, fill):
        self.ld = cols + pad
        self.buf = torch.full((2 * GUARD + (rows + 1) * self.ld,), fill, dtype=dtype, device=DEV)
        self.w = self.buf[GUARD:GUARD + (rows + 1) * self.ld].view(rows + 1, self.ld)[:rows, :cols]
        self.before = self.buf.clone()

    def only_output_written(self):
        a, b = self.buf.clone(), self.before.clone()
        for t in (a, b):
            t[GUARD:GUARD + (self.w.shape[0] + 1) * self.ld].view(-1, self.ld)[:self.w.shape[0], :self.w.shape[1]] = 0
        return torch.equal(_bits(a), _bits(b))

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


# ------------------------------------------------------------------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("K", xc.QUANT_K)
@pytest.mark.parametrize("N", xc.QUANT_N)
def test_quantiser_equals_the_restatement_bit_for_bit(N, K):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    pad_w, pad_q, pad_s, pad_h = 8 * (1 + N % 3), 16 * (1 + K % 3), 1 + N % 4, 8 * (N % 2)
    w = xc.quant_input(N, K, pad_w)
    p_ref, s_ref, h_ref = xc.quantize_mxfp4_ref(w[:, :K].contiguous())
    wd = w.to(DEV)
    pb, sb, hb = Guarded(N, K // 2, pad_q, U8, 0xA5), Guarded(N, K // 32, pad_s, U8, 0xA5), Guarded(N, K, pad_h, BF, xc.NAN)
    p2, s2 = _guarded(f"quantize {N}x{K} without w_hat", lambda: ops.quantize_rows_mxfp4(wd[:, :K]))
    assert hb.untouched()
    n0 = lib.llmseg_launch_count()
    _guarded(f"quantize {N}x{K}", lambda: ops.quantize_rows_mxfp4(wd[:, :K], packed=pb.w, scale=sb.w, w_hat=hb.w))
    assert lib.llmseg_launch_count() - n0 == 1, "one launch"
    assert torch.equal(pb.w.cpu(), p_ref) and torch.equal(p2.cpu(), p_ref), "packed bytes"
    assert torch.equal(sb.w.cpu(), s_ref) and torch.equal(s2.cpu(), s_ref), "scale bytes"
    diff = (_bits(hb.w.cpu()) != _bits(h_ref)).nonzero()
    assert not len(diff), f"w_hat: {len(diff)} elements differ, the first at {diff[0].tolist()}: {hb.w[tuple(diff[0])].item()!r} for {h_ref[tuple(diff[0])].item()!r}"
    assert pb.only_output_written() and sb.only_output_written() and hb.only_output_written(), "a store outside the outputs (canary changed)"
    assert _same(wd, w.to(DEV)), "the input was written"
    if N >= len(xc.HAND_BLOCKS):
        _, codes, scales = xc.hand_blocks(K)
        got = xc.nibbles(pb.w.cpu())
        for r, name in enumerate(xc.HAND_BLOCKS):
            assert torch.equal(got[r], codes[r]) and torch.equal(sb.w[r].cpu().to(torch.int64), scales[r]), name


# ---------------------------------------------------------------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gemm_mxfp4_parity_with_fp64(case):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    inp, ref, bound = xc.reference(case)
    M, N, K = case.M, case.N, case.K
    lda, ldq, lds, ldc, ldr = xc.dims(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    cb = Guarded(M, N, case.ldc_pad, F32 if case.f32 else BF, xc.NAN)
    n0 = lib.llmseg_launch_count()
    _guarded(case.name, lambda: ops.gemm_mxfp4(d["a"][:M, :K], d["q"][:N, :K // 2], d["scale"][:N, :K // 32], residual=d["res"][:, :N] if case.res else None, out=cb.w))
    assert lib.llmseg_launch_count() - n0 == case.launches
    assert cb.only_output_written(), f"{case.name}: a store outside the output"
    r = xc.ratio(cb.w.cpu(), ref, bound)
    print(f"\n{case.name}: error / bound {r:.3f}")
    k = "fp32" if case.f32 else "bf16"
    _WORST[k] = max(_WORST[k], (r, case.name))
    assert r <= 1.0, f"{case.name}: error / bound = {r:.3f}"
    # no atomics, one order of summation: the same inputs give the same bits
    cb2 = Guarded(M, N, case.ldc_pad, F32 if case.f32 else BF, xc.NAN)
    _guarded(case.name, lambda: ops.gemm_mxfp4(d["a"][:M, :K], d["q"][:N, :K // 2], d["scale"][:N, :K // 32], residual=d["res"][:, :N] if case.res else None, out=cb2.w))
    assert _same(cb.w, cb2.w)


def test_gemm_mxfp4_allocates_its_output_in_both_types():
    from llmseg_amd import ops
    case = next(c for c in CASES if c.res and c.M == 4 and not c.f32)
    inp, ref, bound = xc.reference(case)
    M, N, K = case.M, case.N, case.K
    d = {k: v.to(DEV) for k, v in inp.items()}
    for f32 in (False, True):
        out = _guarded(case.name, lambda: ops.gemm_mxfp4(d["a"][:M, :K], d["q"][:N, :K // 2], d["scale"][:N, :K // 32], residual=d["res"][:, :N], out_f32=f32))
        assert out.dtype == (F32 if f32 else BF) and out.shape == (M, N)
        b = bound - xc.C_BF16 * 2.0 ** -8 * ref.abs() if f32 else bound          # the fp32 output carries no store rounding
        assert xc.ratio(out.cpu(), ref, b) <= 1.0


def test_refused_calls_launch_nothing_and_write_nothing():
    from llmseg_amd import _lib
    lib = _lib.load()
    M, N, K = 2, 4, 64
    a = torch.randn(M, K + 8, device=DEV).to(BF)
    q = torch.randint(0, 256, (N, K // 2 + 16), device=DEV, dtype=torch.int32).to(U8)
    s = torch.full((N, K // 32), 127, device=DEV, dtype=U8)
    cb = Guarded(M, N, 0, BF, xc.NAN)
    ok = dict(A=a.data_ptr(), Q=q.data_ptr(), scale=s.data_ptr(), C=cb.w.data_ptr(), M=M, N=N, K=K, lda=a.stride(0), ldq=q.stride(0), lds=s.stride(0), ldc=cb.ld)
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in (dict(M=0), dict(M=9), dict(K=K - 16), dict(A=a.data_ptr() + 2), dict(Q=q.data_ptr() + 8), dict(ldq=K // 2 - 16), dict(lds=1), dict(struct_size=0)):
        g = _lib.GemmMxfp4Args(**{k: v for k, v in dict(ok, **bad).items() if k != "struct_size"})
        if "struct_size" in bad:
            g.struct_size = C.sizeof(_lib.GemmW8Args)
        assert lib.llmseg_gemm_mxfp4(C.byref(g), stream) == -1, bad
    torch.cuda.synchronize()
    assert lib.llmseg_launch_count() == n0 and cb.untouched()
    g = _lib.GemmMxfp4Args(**ok)                                           # the same arguments, unspoilt, are accepted
    assert lib.llmseg_gemm_mxfp4(C.byref(g), stream) == 0
    torch.cuda.synchronize()
    assert lib.llmseg_launch_count() == n0 + 1 and bool(torch.isfinite(cb.w.float()).all())


# ---------------------------------------------------------------------------------------------------------------------------- generation
MAX_NEW = 6
PAD = 0
LENS = (24, 17)                # the ragged route: rows 0 and 1 of the tiny batch cut to these lengths


def _model(sd, cfg, sam_decoder=False):
    from llmseg_amd import lisa as hip_lisa
    from tests import model_checks as mc
    hcfg = mc.to_hip_cfg(cfg)
    if sam_decoder:
        hcfg.sam_decoder = True
    m = hip_lisa.LISAForCausalLM(hcfg, device=DEV)
    missing, _ = m.load_state_dict(sd, strict=False)
    assert not missing, missing[:5]
    return m


@functools.lru_cache(maxsize=None)
def _states(lora_r):
    """-> (cfg, sd, sd_q, sd_8, restated); shared by the tests below, which do not write to them"""
    from oracle import cases
    cfg = cases.tiny_lisa_cfg(lora_r=lora_r)
    return (cfg,) + xc.generation_states_mxfp4(cfg)


@functools.lru_cache(maxsize=None)
def _hip_model(lora_r):
    cfg, sd = _states(lora_r)[:2]
    return _model(sd, cfg)


@functools.lru_cache(maxsize=None)
def _batch():
    from oracle import cases
    from tests import model_checks as mc
    batch = mc._round_batch(cases.tiny_lisa_batch())
    return batch["images_clip"][:2], batch["input_ids"][:2]


def _oracle(osd, cfg, clip, fed):
    from oracle import lisa as olisa
    with torch.no_grad():
        _, lg, h = olisa.llava_forward(osd, cfg, clip, torch.ones_like(fed, dtype=torch.bool), fed)
    return lg.float(), h.float()


@pytest.mark.parametrize("lora_r", (0, 8))
def test_generate_mxfp4_runs_the_quantised_model(lora_r):
    """figures of the GPU run are printed before every assertion"""
    from tests import generate_checks as gchk
    cfg, sd, sd_q, sd_8, restated = _states(lora_r)
    m = _hip_model(lora_r)
    clip, ids0 = _batch()
    L = ids0.shape[1]
    seq, hid = _guarded("generate", lambda: m.generate(clip.to(DEV), ids0.to(DEV), max_new_tokens=MAX_NEW, eos_token_id=None, weight_format="mxfp4"))
    seq, hid = seq.cpu(), hid.float().cpu()
    assert seq.shape == (2, L + MAX_NEW) and bool((seq[:, :L] == ids0).all())
    fed = seq[:, :-1]                                                        # teacher forcing: the oracle sees the HIP path's own tokens
    logits_q, hid_q = _oracle(sd_q, cfg, clip, fed)
    hid_w, hid_8 = _oracle(sd, cfg, clip, fed)[1], _oracle(sd_8, cfg, clip, fed)[1]      # the unquantised and the int8 model on the same tokens
    assert hid.shape == hid_q.shape, (hid.shape, hid_q.shape)
    T = hid_q.shape[1] - (MAX_NEW - 1)
    tol = 3e-2 * max(1.0, hid_q.abs().max().item())
    vis_w, vis_8 = (hid_w - hid_q).abs().max().item(), (hid_8 - hid_q).abs().max().item()
    err = (hid - hid_q).abs().max().item()
    steps = logits_q[:, T - 1:]                                               # [2, MAX_NEW, V]: the logits each new token was chosen from
    gap = steps.max(-1).values - steps.gather(-1, seq[:, L:][..., None])[..., 0]
    print(f"\nlora_r={lora_r}: hidden err {err:.3e} (tol {tol:.3e}), the unquantised model differs by {vis_w:.3e}, the int8 model by {vis_8:.3e}, worst logit gap of a chosen "
          f"token {gap.max().item():.3e} (MARGIN {gchk.MARGIN}), mxfp4 prepare {m.mxfp4_prepare_ms():.3f} ms")
    # precondition (CPU): the other two models are visible at twice the tolerance, so a path that silently ran on W or on the int8 rows would fail below
    assert vis_w >= 2 * tol, f"the unquantised oracle differs from the MXFP4 one by only {vis_w:.3e} (tolerance {tol:.3e})"
    assert vis_8 >= 2 * tol, f"the int8 oracle differs from the MXFP4 one by only {vis_8:.3e} (tolerance {tol:.3e})"
    assert err <= tol, f"hidden states differ from the quantised oracle by {err:.3e} > {tol:.3e}"
    assert gap.shape == (2, MAX_NEW) and bool((gap <= gchk.MARGIN).all()), f"a chosen token is {gap.max().item():.3e} below the oracle's best logit"
    got = m.decode_weights_mxfp4()
    c = cfg.llama
    assert len(got) == 4 * c.layers
    for k, (p, s) in got.items():
        assert p.dtype == U8 and s.dtype == U8 and p.shape[1] * 2 == s.shape[1] * 32 and p.shape[0] == s.shape[0], k
    if lora_r == 0:
        for i in range(c.layers):
            pre = f"model.layers.{i}."
            for name, members in xc.MEMBERS:
                p, s = got[pre + name]
                assert torch.equal(p.cpu(), torch.cat([restated[pre + n][0] for n in members], 0)), pre + name
                assert torch.equal(s.cpu(), torch.cat([restated[pre + n][1] for n in members], 0)), pre + name


def test_no_leak_between_the_bf16_the_int8_and_the_mxfp4_mode():
    m = _hip_model(8)
    clip, ids0 = (t.to(DEV) for t in _batch())
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None)
    modes = {"bf16": {}, "int8": dict(weight_bits=8), "mxfp4": dict(weight_format="mxfp4")}
    first = {}
    for rnd in range(2):                                                     # bf16, int8, mxfp4, bf16, int8, mxfp4: every mode after each of the others
        for name, mode in modes.items():
            seq, hid = _guarded(name, lambda: m.generate(clip, ids0, **mode, **kw))
            if rnd == 0:
                first[name] = (seq, hid)
            else:
                assert torch.equal(seq, first[name][0]) and _same(hid, first[name][1]), f"a {name} call after calls of the other modes differs from the one before them"
    for a, b in (("bf16", "int8"), ("bf16", "mxfp4"), ("int8", "mxfp4")):
        assert not _same(first[a][1], first[b][1]), f"{a} and {b} gave the same hidden states: one of them ran the other's weights"
    # eager steps and the replayed graph run the same kernels on the same buffers
    seq_e, hid_e = _guarded("eager", lambda: m.generate(clip, ids0, weight_format="mxfp4", use_graph=False, **kw))
    assert torch.equal(first["mxfp4"][0], seq_e) and _same(first["mxfp4"][1], hid_e)
    seq_b, hid_b = _guarded("bf16 after eager", lambda: m.generate(clip, ids0, **kw))
    assert torch.equal(seq_b, first["bf16"][0]) and _same(hid_b, first["bf16"][1])


def _hidden_within_tolerance(lora_r, rows, what):
    """rows: [(clip [1, 3, 224, 224], fed tokens [1, n], hidden fp32 [n + Pn - 1, H] of the HIP path)]: each against the W^ oracle teacher-forced on `fed`"""
    cfg, _, sd_q = _states(lora_r)[:3]
    orc = [_oracle(sd_q, cfg, clip, fed)[1][0] for clip, fed, _ in rows]
    tol = 3e-2 * max(1.0, max(h.abs().max().item() for h in orc))
    errs = []
    for (_, _, hid), h in zip(rows, orc):
        assert hid.shape == h.shape, (what, hid.shape, h.shape)
        errs.append((hid - h).abs().max().item())
    print(f"\n{what} lora_r={lora_r}: hidden err per row {['%.3e' % e for e in errs]} (tol {tol:.3e})")
    assert max(errs) <= tol, f"{what}: hidden states differ from the W^ oracle by {max(errs):.3e} > {tol:.3e}"


@pytest.mark.parametrize("lora_r", (0, 8))
def test_ragged_route(lora_r):
    from llmseg_amd.generate import pad_prompts
    cfg = _states(lora_r)[0]
    m = _hip_model(lora_r)
    clip, ids0 = _batch()
    ids, mask = pad_prompts([ids0[i, :n].clone() for i, n in enumerate(LENS)], PAD)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None, pad_token_id=PAD, weight_format="mxfp4", attention_mask=mask.to(DEV))
    seq, hid = _guarded("ragged", lambda: m.generate(clip.to(DEV), ids.to(DEV), **kw))
    seq_e, hid_e = _guarded("ragged eager", lambda: m.generate(clip.to(DEV), ids.to(DEV), use_graph=False, **kw))
    assert torch.equal(seq, seq_e) and _same(hid, hid_e), "graph replay differs from eager steps"
    seq, hid = seq.cpu(), hid.float().cpu()
    Pn = cfg.n_img_tokens
    rows = []
    for i, L in enumerate(LENS):
        assert torch.equal(seq[i, :L], ids0[i, :L]) and bool((seq[i, L + MAX_NEW:] == PAD).all())
        rows.append((clip[i:i + 1], seq[i:i + 1, :L + MAX_NEW - 1], hid[i, :L - 1 + Pn + MAX_NEW - 1]))
    _hidden_within_tolerance(lora_r, rows, "attention_mask")


@pytest.mark.parametrize("lora_r", (0, 8))
def test_sampling_route(lora_r):
    m = _hip_model(lora_r)
    clip, ids0 = _batch()
    L = ids0.shape[1]
    us = torch.rand((2, MAX_NEW), dtype=F32, generator=torch.Generator().manual_seed(5)).to(DEV)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None, weight_format="mxfp4", do_sample=True, temperature=0.8, top_k=20, top_p=0.9, uniforms=us)
    seq, hid = _guarded("sampling", lambda: m.generate(clip.to(DEV), ids0.to(DEV), **kw))
    seq_e, hid_e = _guarded("sampling eager", lambda: m.generate(clip.to(DEV), ids0.to(DEV), use_graph=False, **kw))
    assert torch.equal(seq, seq_e) and _same(hid, hid_e), "graph replay differs from eager steps"
    seq, hid = seq.cpu(), hid.float().cpu()
    assert seq.shape == (2, L + MAX_NEW)
    _hidden_within_tolerance(lora_r, [(clip[i:i + 1], seq[i:i + 1, :-1], hid[i]) for i in range(2)], "do_sample")


@pytest.mark.parametrize("lora_r", (0, 8))
def test_beam_route_in_chunks_of_eight_rows(lora_r):
    m = _hip_model(lora_r)
    clip, ids0 = _batch()
    L = ids0.shape[1]
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None, pad_token_id=PAD, weight_format="mxfp4", num_beams=5, return_beam_scores=True)      # 2 x 5 = 10 rows: 8 + 2
    runs = {(bc, g): _guarded(f"beams {bc} graph={g}", lambda: m.generate(clip.to(DEV), ids0.to(DEV), beam_cache=bc, use_graph=g, **kw))
            for bc in ("indirect", "copy") for g in (True, False)}
    seq, hid, val = runs[("indirect", True)]
    for key, (s2, h2, v2) in runs.items():
        assert torch.equal(seq, s2) and _same(hid, h2) and _same(val, v2), f"beam_cache / use_graph = {key} differs from the indirect cache replayed from the graph"
    seq, hid = seq.cpu(), hid.float().cpu()
    assert seq.shape == (2, L + MAX_NEW) and val.shape == (2,)
    _hidden_within_tolerance(lora_r, [(clip[i:i + 1], seq[i:i + 1, :L + MAX_NEW - 1], hid[i]) for i in range(2)], "num_beams=5")


def test_evaluate_forwards_weight_format():
    from oracle import cases
    from tests import model_checks as mc, w8_checks as wc
    cfg = cases.tiny_lisa_cfg("sam")
    sd, _, _ = wc.generation_states(cfg)
    sd.update({k: v.to(BF).float() for k, v in cases.sam_decoder_state().items()})
    m = _model(sd, cfg, sam_decoder=True)
    batch = mc._round_batch(cases.tiny_lisa_batch(img_size=cfg.sam.img))
    clip, images, ids = batch["images_clip"][:2].to(DEV), batch["images"][:2].to(DEV), batch["input_ids"][:2].to(DEV)
    resize, orig = [(683, 1024), (1024, 768)], [(427, 640), (96, 72)]
    kw = dict(max_new_tokens=3, eos_token_id=None)
    seq_4, hid_4 = _guarded("generate", lambda: m.generate(clip, ids, weight_format="mxfp4", **kw))
    seq_w, hid_w = _guarded("generate", lambda: m.generate(clip, ids, **kw))
    assert not _same(hid_4, hid_w)
    calls = []
    real = m.generate
    m.generate = lambda *a, **k: (calls.append(k.get("weight_format")), real(*a, **k))[1]
    ids_4, masks = _guarded("evaluate", lambda: m.evaluate(clip, images, ids, resize, orig, weight_format="mxfp4", **kw))
    ids_w, _ = _guarded("evaluate", lambda: m.evaluate(clip, images, ids, resize, orig, **kw))
    assert calls == ["mxfp4", None]
    assert torch.equal(ids_4, seq_4) and len(masks) == 2 and torch.equal(ids_w, seq_w)


def test_argument_errors():
    m = _hip_model(8)
    clip, ids0 = (t.to(DEV) for t in _batch())
    kw = dict(max_new_tokens=2, eos_token_id=None)
    for bad in (dict(weight_bits=4), dict(weight_format="mxfp4", weight_bits=8), dict(weight_format="mxfp4", fuse_decode=False), dict(weight_format="fp4"),
                dict(weight_format="mxfp4", weight_bits=8, num_beams=2)):
        with pytest.raises(ValueError):
            m.generate(clip, ids0, **bad, **kw)
