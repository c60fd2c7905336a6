"""GPU: int8 weight-only decode.  The quantiser kernel bit for bit against the torch restatement of its public arithmetic; llmseg_gemm_w8 on every case of
tests/w8_checks.py against fp64 references under the per-element bounds tests/test_w8_decode_cpu.py validates; generate(weight_bits=8) against ONE
teacher-forced cache-free oracle forward on an independently quantised state dict; no state leaks between the bf16 and the int8 mode."""
import collections

import pytest
import torch

from tests import w8_checks as wc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
CASES = wc.cases()
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


# ------------------------------------------------------------------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("K", wc.QUANT_K)
@pytest.mark.parametrize("N", wc.QUANT_N)
def test_quantiser_equals_the_restatement_bit_for_bit(N, K):
    from llmseg_amd import ops
    pad_w, pad_q, pad_h = 8 * (1 + N % 3), 16 * (1 + K % 3), 8 * (N % 2)
    w = wc.quant_input(N, K, pad_w)
    q_ref, s_ref, h_ref = wc.quantize_ref(w[:, :K].contiguous())
    wd = w.to(DEV)
    qb = torch.full((N + 1, K + pad_q), 99, dtype=torch.int8, device=DEV)
    hb = torch.full((N + 1, K + pad_h), wc.NAN, dtype=BF, device=DEV)
    sb = torch.full((N + 1,), wc.NAN, dtype=F32, device=DEV)
    try:
        ops.quantize_rows_i8(wd[:, :K], q=qb[:N, :K], scale=sb[:N], w_hat=hb[:N, :K])
        q2, s2 = ops.quantize_rows_i8(wd[:, :K])                          # without the second output
        torch.cuda.synchronize()
    except RuntimeError as e:
        _fault_guard(f"quantize {N}x{K}", e)
        raise
    assert torch.equal(qb[:N, :K].cpu(), q_ref) and torch.equal(q2.cpu(), q_ref)
    assert torch.equal(sb[:N].cpu().view(torch.int32), s_ref.view(torch.int32)) and torch.equal(s2.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(hb[:N, :K].cpu().view(torch.int16), h_ref.view(torch.int16))
    # nothing outside the outputs was written
    assert bool((qb[:, K:] == 99).all()) and bool((qb[N] == 99).all()) and bool(torch.isnan(hb[:, K:].float()).all()) and bool(torch.isnan(hb[N].float()).all())
    assert bool(torch.isnan(sb[N]))
    if N >= 5:
        for r, want in wc.hand_rows_expected_q(K).items():
            assert torch.equal(qb[r, :K].cpu(), want), wc.HAND_ROWS[r]


# ---------------------------------------------------------------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gemm_w8_parity_with_fp64(case):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    inp, ref, bound = wc.reference(case)
    M, N, K = case.M, case.N, case.K
    lda, ldq, ldc, ldr = wc.dims(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    cb = torch.full((M + 1, ldc), wc.NAN, dtype=F32 if case.f32 else BF, device=DEV)
    try:
        n0 = lib.llmseg_launch_count()
        ops.gemm_w8(d["a"][:M, :K], d["q"][:N, :K], d["scale"][:N], residual=d["res"][:, :N] if case.res else None, out=cb[:M, :N])
        launches = lib.llmseg_launch_count() - n0
        torch.cuda.synchronize()
    except RuntimeError as e:
        _fault_guard(case.name, e)
        raise
    assert launches == case.launches
    assert bool(torch.isnan(cb[:, N:].float()).all()) and bool(torch.isnan(cb[M].float()).all()), f"{case.name}: a store outside the output"
    r = wc.ratio(cb[:M, :N].cpu(), ref, bound)
    print(f"\n{case.name}: error / bound {r:.3f}")
    k = "fp32" if case.f32 else "bf16"
    _WORST[k] = max(_WORST[k], (r, case.name))
    assert r <= 1.0, f"{case.name}: error / bound = {r:.3f}"


def test_gemm_w8_allocates_its_output_in_both_types():
    from llmseg_amd import ops
    case = next(c for c in CASES if c.res and c.M == 4 and not c.f32)
    inp, ref, bound = wc.reference(case)
    M, N, K = case.M, case.N, case.K
    d = {k: v.to(DEV) for k, v in inp.items()}
    for f32 in (False, True):
        out = ops.gemm_w8(d["a"][:M, :K], d["q"][:N, :K], d["scale"][:N], residual=d["res"][:, :N], out_f32=f32)
        assert out.dtype == (F32 if f32 else BF) and out.shape == (M, N)
        b = bound - wc.C_BF16 * 2.0 ** -8 * ref.abs() if f32 else bound          # the fp32 output carries no store rounding
        assert wc.ratio(out.cpu(), ref, b) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------- generation
MAX_NEW = 6


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


@pytest.mark.parametrize("lora_r", (0, 8))
def test_generate_w8_runs_the_quantised_model(lora_r):
    """figures of the GPU run are printed before every assertion"""
    from oracle import cases, lisa as olisa
    from tests import generate_checks as gchk, model_checks as mc
    cfg = cases.tiny_lisa_cfg(lora_r=lora_r)
    sd, sd_q, restated = wc.generation_states(cfg)
    m = _model(sd, cfg)
    batch = mc._round_batch(cases.tiny_lisa_batch())
    clip, ids0 = batch["images_clip"][:2], batch["input_ids"][:2]
    L = ids0.shape[1]
    with torch.no_grad():
        seq, hid = m.generate(clip.to(DEV), ids0.to(DEV), max_new_tokens=MAX_NEW, eos_token_id=None, weight_bits=8)
        seq, hid = seq.cpu(), hid.float().cpu()
        assert seq.shape == (2, L + MAX_NEW) and bool((seq[:, :L] == ids0).all())
        fed = seq[:, :-1]                                                    # teacher forcing: the oracle sees the HIP path's own tokens
        mask = torch.ones_like(fed, dtype=torch.bool)
        _, logits_q, hid_q = olisa.llava_forward(sd_q, cfg, clip, mask, fed)
        _, _, hid_w = olisa.llava_forward(sd, cfg, clip, mask, fed)           # the unquantised model on the same tokens
    assert hid.shape == hid_q.shape, (hid.shape, hid_q.shape)
    T = hid_q.shape[1] - (MAX_NEW - 1)
    tol = 3e-2 * max(1.0, hid_q.abs().max().item())
    visible = (hid_w - hid_q).abs().max().item()
    err = (hid - hid_q).abs().max().item()
    steps = logits_q[:, T - 1:].float()                                       # [2, MAX_NEW, V]: the logits each new token was chosen from
    chosen = seq[:, L:]
    gap = (steps.max(-1).values - steps.gather(-1, chosen[..., None])[..., 0])
    print(f"\nlora_r={lora_r}: hidden err {err:.3e} (tol {tol:.3e}), unquantised model differs by {visible:.3e}, worst logit gap of a chosen token {gap.max().item():.3e} "
          f"(MARGIN {gchk.MARGIN}), w8 prepare {m.w8_prepare_ms():.3f} ms")
    # precondition (CPU): quantisation is visible at twice the tolerance, so a path that silently ran on W would fail below
    assert visible >= 2 * tol, f"the unquantised oracle differs from the quantised one by only {visible:.3e} (tolerance {tol:.3e})"
    assert err <= tol, f"hidden states differ from the quantised oracle by {err:.3e} > {tol:.3e}"
    assert gap.shape == (2, MAX_NEW) and bool((gap <= gchk.MARGIN).all()), f"a chosen token is {gap.max().item():.3e} below the oracle's best logit"
    got = m.decode_weights_i8()
    c = cfg.llama
    assert len(got) == 4 * c.layers
    if lora_r == 0:
        for i in range(c.layers):
            p = f"model.layers.{i}."
            for name, members in (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("self_attn.o_proj.weight", ("self_attn.o_proj",)),
                                  ("gate_up", ("mlp.gate_proj", "mlp.up_proj")), ("mlp.down_proj.weight", ("mlp.down_proj",))):
                q, s = got[p + name]
                assert torch.equal(q.cpu(), torch.cat([restated[p + n][0] for n in members], 0)), p + name
                assert torch.equal(s.cpu(), torch.cat([restated[p + n][1] for n in members], 0)), p + name


def test_no_leak_between_the_bf16_and_the_int8_mode():
    from oracle import cases
    from tests import model_checks as mc
    cfg = cases.tiny_lisa_cfg(lora_r=8)
    sd, _, _ = wc.generation_states(cfg)
    m = _model(sd, cfg)
    batch = mc._round_batch(cases.tiny_lisa_batch())
    clip, ids0 = batch["images_clip"][:2].to(DEV), batch["input_ids"][:2].to(DEV)
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None)
    with pytest.raises(ValueError):
        m.generate(clip, ids0, weight_bits=4, **kw)
    with pytest.raises(ValueError):
        m.generate(clip, ids0, weight_bits=8, fuse_decode=False, **kw)
    seq_a, hid_a = m.generate(clip, ids0, **kw)
    seq_8, hid_8 = m.generate(clip, ids0, weight_bits=8, **kw)
    seq_b, hid_b = m.generate(clip, ids0, **kw)
    seq_9, hid_9 = m.generate(clip, ids0, weight_bits=8, **kw)
    assert torch.equal(seq_a, seq_b) and torch.equal(hid_a.view(torch.int16), hid_b.view(torch.int16)), "a default call after a weight_bits=8 call differs from one before it"
    assert torch.equal(seq_8, seq_9) and torch.equal(hid_8.view(torch.int16), hid_9.view(torch.int16)), "a weight_bits=8 call after a default call differs from one before it"
    assert not torch.equal(hid_a.view(torch.int16), hid_8.view(torch.int16)), "weight_bits=8 ran the unquantised model"
    # eager steps and the replayed graph run the same kernels on the same buffers
    seq_e, hid_e = m.generate(clip, ids0, weight_bits=8, use_graph=False, **kw)
    assert torch.equal(seq_8, seq_e) and torch.equal(hid_8.view(torch.int16), hid_e.view(torch.int16))


def test_evaluate_forwards_weight_bits():
    from oracle import cases
    from tests import model_checks as mc
    cfg = cases.tiny_lisa_cfg("sam")
    sd, _, _ = wc.generation_states(cfg)
    sd.update({k: v.to(BF).float() for k, v in cases.sam_decoder_state().items()})
    m = _model(sd, cfg, sam_decoder=True)
    batch = mc._round_batch(cases.tiny_lisa_batch(img_size=cfg.sam.img))
    clip, images, ids = batch["images_clip"][:2].to(DEV), batch["images"][:2].to(DEV), batch["input_ids"][:2].to(DEV)
    resize, orig = [(683, 1024), (1024, 768)], [(427, 640), (96, 72)]
    seq_8, _ = m.generate(clip, ids, max_new_tokens=3, eos_token_id=None, weight_bits=8)
    seq_w, _ = m.generate(clip, ids, max_new_tokens=3, eos_token_id=None)
    ids_8, masks = m.evaluate(clip, images, ids, resize, orig, max_new_tokens=3, eos_token_id=None, weight_bits=8)
    assert torch.equal(ids_8, seq_8) and len(masks) == 2
    ids_w, _ = m.evaluate(clip, images, ids, resize, orig, max_new_tokens=3, eos_token_id=None)
    assert torch.equal(ids_w, seq_w)
