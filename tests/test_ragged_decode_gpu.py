"""GPU: greedy decode over prompts of different lengths.  llmseg_decode_attn_rows on every case of tests/ragged_decode_checks.py against the row-by-row fp64
reference under the per-element bounds tests/test_ragged_decode_cpu.py validates, and bit for bit against the scalar entry point where the positions are
equal; generate(attention_mask=) against ONE teacher-forced cache-free oracle forward per row (the row alone, unpadded, on the tokens the HIP path chose),
in bf16 and with weight_bits=8; the packed layout, the [SEG] contract, the eos rule per row; no state leaks between uniform and ragged calls."""
import dataclasses
import functools

import pytest
import torch

from tests import forward_kernel_checks as fk
from tests import ragged_decode_checks as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
CASES = rc.cases()
SCALAR = [c for c in fk.cases() if c.op == "decode"]
LENS = (24, 17, 9)             # rows 0..2 of the tiny batch cut to these lengths (the precondition of the parity tests needs rows this short)
MAX_NEW = 5
PAD = 0


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield


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


# ------------------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_decode_attn_rows_parity_with_fp64(case):
    from llmseg_amd import _lib, ops
    from tests.test_backward_kernels_gpu import Out
    lib = _lib.load()
    inp, ref, bounds = rc.reference(case)
    N, H, cap = case.N, case.heads, rc.CAP
    D = H * rc.HD
    qkv, cos, sin = (inp[k].to(DEV) for k in ("qkv", "cos", "sin"))
    q0 = qkv.clone()
    o = {}
    for n in ("kc", "vc"):                                  # the caches and the output sit between guard regions
        o[n] = Out(N * cap, D, BF, NAN)
        o[n].w.copy_(inp[n].to(DEV).view(N * cap, D))
        o[n].before = o[n].buf.clone()
    o["out"] = Out(N, D, BF, NAN)
    posd = torch.tensor(case.pos, dtype=torch.int32, device=DEV)
    nf = rc.decode_scratch_floats(case)
    scratch = torch.empty(nf, dtype=F32, device=DEV) if nf else None
    cache = lambda n: o[n].w.view(N, cap, D)
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    _guarded(case.name, lambda: ops.decode_attn(qkv, cos, sin, cache("kc"), cache("vc"), posd, H, rc.HD, out=o["out"].w, scale=inp["scale"], scratch=scratch, per_row=True))
    assert lib.llmseg_launch_count() - n0 == case.launches, f"{case.name}: {lib.llmseg_launch_count() - n0} launches, the table says {case.launches}"
    assert all(b.guard_untouched() for b in o.values()), f"{case.name}: a store outside the buffers (guard region changed)"
    assert _same(qkv, q0), "decode_attn wrote its qkv operand"
    assert torch.equal(posd.cpu(), torch.tensor(case.pos, dtype=torch.int32)), "the positions were written"
    got = {"out": o["out"].w.cpu(), "kc": cache("kc").cpu(), "vc": cache("vc").cpu()}
    r = rc.ratios(got, ref, bounds)
    print(f"\n{case.name}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    # every cache slot other than (n, pos_n) keeps its input BITS (NaN sentinels included); the v row written is the bf16 input, bit for bit
    for k in ("kc", "vc"):
        keep = torch.ones((N, cap), dtype=torch.bool)
        keep[torch.arange(N), torch.tensor(case.pos)] = False
        assert torch.equal(_bits(got[k])[keep], _bits(inp[k])[keep]), f"{case.name}: {k} changed outside the rows' own slots"
    vnew = inp["qkv"][:, 2 * D:]
    assert torch.equal(_bits(got["vc"][torch.arange(N), torch.tensor(case.pos)]), _bits(vnew)), f"{case.name}: the appended v rows are not the input's bits"
    assert r["vc"] == 0.0, r
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}: error / bound > 1: {bad}"


@pytest.mark.parametrize("case", SCALAR, ids=[c.name for c in SCALAR])
def test_equal_positions_give_the_bits_of_the_scalar_entry(case):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    inp = fk.inp_cached(case)
    N, H, cap = case.N, case.heads, fk.CAP
    qkv, cos, sin = (inp[k].to(DEV) for k in ("qkv", "cos", "sin"))
    nf = fk.decode_scratch_floats(case)
    res = []
    for per_row in (False, True):
        kc, vc = inp["kc"].to(DEV).clone(), inp["vc"].to(DEV).clone()
        out = torch.full((N, H * fk.HD), NAN, dtype=BF, device=DEV)
        scratch = torch.full((nf,), NAN, dtype=F32, device=DEV) if nf else None
        posd = torch.full((N if per_row else 1,), case.pos, dtype=torch.int32, device=DEV)
        n0 = lib.llmseg_launch_count()
        _guarded(case.name, lambda: ops.decode_attn(qkv, cos, sin, kc, vc, posd, H, fk.HD, out=out, scale=inp["scale"], scratch=scratch, per_row=per_row))
        res.append((out, kc, vc, lib.llmseg_launch_count() - n0))
    (o0, k0, v0, l0), (o1, k1, v1, l1) = res
    assert l0 == l1 == case.launches - 1                       # (the table counts the rope_kv_append call of the other test as well)
    assert bool(torch.isfinite(o0.float()).all())
    assert _same(o0, o1) and _same(k0, k1) and _same(v0, v1), f"{case.name}: the per-row entry with equal positions differs from the scalar entry"


# ---------------------------------------------------------------------------------------------------------------------------- generation
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


def _prompts(img_size=896):
    """-> (batch, clip [3, 3, 224, 224], the three full rows [3, 24], the cut rows, image index of every row)"""
    from oracle import cases
    from tests import model_checks as mc
    batch = mc._round_batch(cases.tiny_lisa_batch(img_size=img_size))
    img = [0, 0, 1]                                         # offset [0, 2, 3]: rows 0 and 1 talk about image 0, row 2 about image 1
    ids = batch["input_ids"][:3]
    return batch, batch["images_clip"][img], ids, [ids[i, :n].clone() for i, n in enumerate(LENS)], img


@functools.lru_cache(maxsize=None)
def _states(lora_r):
    from oracle import cases
    from tests import w8_checks as wc
    cfg = cases.tiny_lisa_cfg(lora_r=lora_r)
    sd, sd_q, _ = wc.generation_states(cfg)
    return cfg, sd, sd_q


@functools.lru_cache(maxsize=None)
def _ragged_run(lora_r, weight_bits):
    """one ragged generate() call and, per row, the oracle's teacher-forced forward on the row alone; shared by the tests below, which do not write to it"""
    from llmseg_amd.generate import pad_prompts
    from oracle import lisa as olisa
    cfg, sd, sd_q = _states(lora_r)
    osd = sd if weight_bits is None else sd_q
    m = _model(sd, cfg)
    _, clip, _, rows, _ = _prompts()
    ids, mask = pad_prompts(rows, PAD)
    seq, hid = _guarded("generate", lambda: m.generate(clip.to(DEV), ids.to(DEV), max_new_tokens=MAX_NEW, eos_token_id=None, pad_token_id=PAD, weight_bits=weight_bits,
                                                       attention_mask=mask.to(DEV)))
    seq, hid_bf = seq.cpu(), hid.cpu()
    oracle, naive = [], []
    with torch.no_grad():
        for i, L in enumerate(LENS):
            fed = seq[i:i + 1, :L + MAX_NEW - 1]                # teacher forcing: the row's prompt and the tokens the HIP path chose, all but the last
            _, lg, h = olisa.llava_forward(osd, cfg, clip[i:i + 1], torch.ones_like(fed, dtype=torch.bool), fed)
            oracle.append((lg[0].float(), h[0].float()))
            # what a path that ignored the mask would compute: the row with its pad tokens as real tokens in front of the same continuation
            fed_n = torch.cat([ids[i:i + 1], seq[i:i + 1, L:L + MAX_NEW - 1]], 1)
            _, _, hn = olisa.llava_forward(osd, cfg, clip[i:i + 1], torch.ones_like(fed_n, dtype=torch.bool), fed_n)
            naive.append(hn[0].float())
    return dict(cfg=cfg, sd=sd, osd=osd, m=m, clip=clip, rows=rows, ids=ids, mask=mask, seq=seq, hid_bf=hid_bf, oracle=oracle, naive=naive)


def _check_parity(lora_r, weight_bits):
    """figures of the GPU run are printed before every assertion"""
    from tests import generate_checks as gchk
    run = _ragged_run(lora_r, weight_bits)
    cfg, seq, hid = run["cfg"], run["seq"], run["hid_bf"].float()
    Pn, Lm = cfg.n_img_tokens, max(LENS)
    Tm = Lm - 1 + Pn
    tol = 3e-2 * max(1.0, max(h.abs().max().item() for _, h in run["oracle"]))
    # precondition (CPU): on the two short rows, the decode-position hidden states of a forward that takes the pad tokens for real tokens differ
    # from the right answer by at least twice the tolerance, so a path that ignored the mask at any of the three uses of the position would fail below
    for i in (1, 2):
        T_i = LENS[i] - 1 + Pn
        right, wrong = run["oracle"][i][1][T_i:T_i + MAX_NEW - 1], run["naive"][i][Tm:Tm + MAX_NEW - 1]
        visible = (right - wrong).abs().max().item()
        print(f"\nrow {i} (L = {LENS[i]}): pad tokens taken for real move the decode-position hidden states by {visible:.3e} = {visible / tol:.2f} x the tolerance")
        assert visible >= 2 * tol, f"row {i}: the padded forward differs from the right one by only {visible:.3e} (tolerance {tol:.3e})"
    # layout, exactly
    assert seq.shape == (3, Lm + MAX_NEW) and seq.dtype == torch.int64 and hid.shape == (3, Tm + MAX_NEW - 1, cfg.llama.hidden)
    errs, gaps = [], []
    for i, L in enumerate(LENS):
        T_i = L - 1 + Pn
        assert torch.equal(seq[i, :L], run["rows"][i]), f"row {i}: the prompt is not the prefix of the sequence"
        assert bool((seq[i, L + MAX_NEW:] == PAD).all()), f"row {i}: fill after the generated tokens"
        assert bool((run["hid_bf"][i, T_i + MAX_NEW - 1:].view(torch.int16) == 0).all()), f"row {i}: zeros after the row's last hidden state"
        lg, h = run["oracle"][i]
        assert h.shape[0] == T_i + MAX_NEW - 1
        errs.append((hid[i, :T_i + MAX_NEW - 1] - h).abs().max().item())
        steps = lg[T_i - 1:]                                   # [MAX_NEW, V]: the logits each new token was chosen from
        chosen = seq[i, L:L + MAX_NEW]
        gaps.append(steps.max(-1).values - steps.gather(-1, chosen[:, None])[:, 0])
        assert gaps[-1].shape == (MAX_NEW,)
    gap = torch.stack(gaps)
    print(f"lora_r={lora_r} weight_bits={weight_bits}: hidden err per row {['%.3e' % e for e in errs]} (tol {tol:.3e}), worst logit gap of a chosen token per row "
          f"{['%.3e' % g.max().item() for g in gaps]} (MARGIN {gchk.MARGIN})")
    assert max(errs) <= tol, f"hidden states differ from the per-row oracle by {max(errs):.3e} > {tol:.3e}"
    assert bool((gap <= gchk.MARGIN).all()), f"a chosen token is {gap.max().item():.3e} below the oracle's best logit"


@pytest.mark.parametrize("lora_r", (0, 8))
def test_generate_ragged_parity_with_the_per_row_oracle(lora_r):
    _check_parity(lora_r, None)


@pytest.mark.parametrize("lora_r", (0, 8))
def test_generate_ragged_w8_parity_with_the_quantised_per_row_oracle(lora_r):
    _check_parity(lora_r, 8)


def test_seg_embeddings_read_the_packed_layout():
    from oracle import generate as ogen
    run = _ragged_run(0, None)
    cfg, m = run["cfg"], run["m"]
    fake = run["seq"].clone()
    fake[2, LENS[2] + 1] = cfg.seg_token_idx                 # a generated position of the shortest row (row 0 carries the [SEG] of its prompt)
    got = _guarded("seg_embeddings", lambda: m.seg_embeddings(fake.to(DEV), run["hid_bf"].to(DEV)))
    counts = []
    for i, L in enumerate(LENS):
        want = ogen.seg_embeddings(run["sd"], cfg, fake[i:i + 1, :L + MAX_NEW], run["oracle"][i][1][None])[0]
        counts.append(want.shape[0])
        assert got[i].shape == want.shape, (i, got[i].shape, want.shape)
        if want.numel():
            err, tol = (got[i].float().cpu() - want).abs().max().item(), 3e-2 * max(1.0, want.abs().max().item())
            print(f"\nrow {i}: [SEG] embedding err {err:.3e} (tol {tol:.3e})")
            assert err <= tol, (i, err, tol)
    assert counts == [1, 0, 1], counts


def _expected_with_eos(toks, eos, pad):
    """greedy rule on rows that do not influence each other: from the tokens of a run without eos -> the tokens of the run with it, [N, n_new]"""
    N, K = toks.shape
    rows, n_new = [], 0
    for i in range(N):
        hit = (toks[i] == eos).nonzero().flatten()
        k = int(hit[0]) + 1 if hit.numel() else K
        n_new = max(n_new, k)
        rows.append(torch.cat([toks[i, :k], torch.full((K - k,), pad, dtype=toks.dtype)]))
    return torch.stack(rows)[:, :n_new]


def test_no_leak_between_uniform_and_ragged_calls():
    from llmseg_amd.generate import pad_prompts
    cfg, sd, _ = _states(8)
    m = _model(sd, cfg)
    _, clip, full, rows, _ = _prompts()
    clip, full = clip.to(DEV), full.to(DEV)
    ids, mask = (t.to(DEV) for t in pad_prompts(rows, PAD))
    kw = dict(max_new_tokens=MAX_NEW, eos_token_id=None, pad_token_id=PAD)
    gen = lambda *a, **k: _guarded("generate", lambda: m.generate(*a, **k))
    uni_a = gen(clip, full, **kw)                            # both on one DecodeState: N = 3 and the same capacity
    rag_a = gen(clip, ids, attention_mask=mask, **kw)
    uni_b = gen(clip, full, **kw)
    rag_b = gen(clip, ids, attention_mask=mask, **kw)
    assert len(m.__dict__["_decode_states"]) == 1
    assert torch.equal(uni_a[0], uni_b[0]) and _same(uni_a[1], uni_b[1]), "a uniform call after a ragged call differs from one before it"
    assert torch.equal(rag_a[0], rag_b[0]) and _same(rag_a[1], rag_b[1]), "a ragged call after a uniform call differs from one before it"
    eager = gen(clip, ids, attention_mask=mask, use_graph=False, **kw)
    assert torch.equal(rag_a[0], eager[0]) and _same(rag_a[1], eager[1]), "eager steps and the replayed graph differ"
    # an all-True mask, and one that is all True once the columns nobody uses are trimmed, are the call without a mask
    ones = gen(clip, full, attention_mask=torch.ones_like(full, dtype=torch.bool), **kw)
    assert torch.equal(uni_a[0], ones[0]) and _same(uni_a[1], ones[1])
    wide = torch.cat([full, torch.full((3, 2), PAD, dtype=full.dtype, device=DEV)], 1)
    wmask = torch.cat([torch.ones_like(full, dtype=torch.bool), torch.zeros((3, 2), dtype=torch.bool, device=DEV)], 1)
    trimmed = gen(clip, wide, attention_mask=wmask, **kw)
    assert torch.equal(uni_a[0], trimmed[0]) and _same(uni_a[1], trimmed[1])
    # row 0 of the ragged call is a full row: its prompt states are those of the uniform call (the same prefill on the same row)
    Tm = full.shape[1] - 1 + cfg.n_img_tokens
    assert _same(rag_a[1][0, :Tm], uni_a[1][0, :Tm])
    # ... and so are its decode steps: the per-row kernel at the position the scalar one reads
    assert torch.equal(rag_a[0][0], uni_a[0][0]) and _same(rag_a[1][0], uni_a[1][0])
    # eos per row: the shortest row's second token ends that row, which emits pad from then on while the others go on
    toks = torch.stack([rag_a[0][i, L:L + MAX_NEW] for i, L in enumerate(LENS)]).cpu()
    eos, pad = int(toks[2, 1]), 7
    want = _expected_with_eos(toks, eos, pad)
    got, hid = gen(clip, ids, attention_mask=mask, max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=pad)
    got = got.cpu()
    n_new = want.shape[1]
    print(f"\neos {eos}: tokens without eos {toks.tolist()}, expected with eos {want.tolist()}")
    assert bool((want[2] == pad).any()) and n_new > 2, "the case must finish one row while another goes on"
    assert got.shape == (3, max(LENS) + n_new) and hid.shape[1] == Tm + n_new - 1
    for i, L in enumerate(LENS):
        assert torch.equal(got[i, :L], rows[i]) and torch.equal(got[i, L:L + n_new], want[i]) and bool((got[i, L + n_new:] == pad).all()), (i, got[i, L:].tolist(), want[i].tolist())
    # early stop: row 1 is row 0's prompt plus row 0's first token, so it emits row 0's tokens one step ahead; with row 0's third token as eos both rows have finished
    # after three steps, which the simulation on the tokens of the run without eos confirms before the run with eos is judged
    t0 = toks[2]
    pair = [rows[2], torch.cat([rows[2], t0[:1]])]
    pids, pmask = (t.to(DEV) for t in pad_prompts(pair, PAD))
    pclip = clip[[2, 2]]
    free, _ = gen(pclip, pids, attention_mask=pmask, **kw)
    ptoks = torch.stack([free[i, p.numel():p.numel() + MAX_NEW] for i, p in enumerate(pair)]).cpu()
    eos = int(ptoks[0, 2])
    want = _expected_with_eos(ptoks, eos, pad)
    print(f"early stop: eos {eos}, tokens without eos {ptoks.tolist()}, expected with eos {want.tolist()}")
    assert want.shape[1] < MAX_NEW, "the case must finish every row before max_new_tokens"
    got, hid = gen(pclip, pids, attention_mask=pmask, max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=pad)
    assert got.shape == (2, pids.shape[1] + want.shape[1]) and hid.shape[1] == pids.shape[1] - 1 + cfg.n_img_tokens + want.shape[1] - 1
    for i, p in enumerate(pair):
        assert torch.equal(got[i, p.numel():p.numel() + want.shape[1]].cpu(), want[i]), (i, got[i].tolist(), want[i].tolist())


def test_rejections():
    from llmseg_amd.generate import pad_prompts
    from oracle import cases
    cfg, sd, _ = _states(0)
    m = _model(sd, cfg)
    _, clip, full, rows, _ = _prompts()
    clip = clip.to(DEV)
    ids, mask = (t.to(DEV) for t in pad_prompts(rows, PAD))
    kw = dict(max_new_tokens=2, eos_token_id=None)
    hole, left, short = mask.clone(), mask.flip(1), mask.clone()
    hole[1, 5] = False
    short[2, 2:] = False                                     # the <image> token of every row sits at index 2
    bad = {"a hole": hole, "left padding": left, "a row that ends before its <image> token": short, "an empty row": mask & (torch.arange(3, device=DEV) != 1)[:, None],
           "another shape": mask[:, :-1], "another dtype": mask.long(), "not a tensor": mask.tolist()}
    for what, am in bad.items():
        with pytest.raises(ValueError):
            m.generate(clip, ids, attention_mask=am, **kw)
            pytest.fail(f"accepted {what}")
    with pytest.raises(ValueError, match="fuse_decode"):
        m.generate(clip, ids, attention_mask=mask, fuse_decode=False, **kw)
    m.generate(clip, full.to(DEV), attention_mask=torch.ones_like(full, dtype=torch.bool), fuse_decode=False, **kw)      # every row full: the uniform route takes it
    cfg64 = dataclasses.replace(cfg, llama=dataclasses.replace(cfg.llama, heads=4))                                   # head_dim 64: the two-launch route
    m64 = _model({k: v.to(BF).float() for k, v in cases.tiny_lisa_state(cfg64).items()}, cfg64)
    with pytest.raises(ValueError, match="head_dim 128.*out of scope"):
        m64.generate(clip, ids, attention_mask=mask, **kw)


def test_evaluate_forwards_the_mask():
    from llmseg_amd.generate import pad_prompts
    from oracle import cases
    from tests import w8_checks as wc
    cfg = cases.tiny_lisa_cfg("sam")
    sd, _, _ = wc.generation_states(cfg)
    sd.update({k: v.to(BF).float() for k, v in cases.sam_decoder_state().items()})
    m = _model(sd, cfg, sam_decoder=True)
    batch, clip, _, rows, img = _prompts(img_size=cfg.sam.img)
    images = batch["images"][img].to(DEV)
    ids, mask = (t.to(DEV) for t in pad_prompts(rows, PAD))
    resize, orig = [(683, 1024), (683, 1024), (1024, 768)], [(427, 640), (427, 640), (96, 72)]
    seq, _ = _guarded("generate", lambda: m.generate(clip.to(DEV), ids, max_new_tokens=3, eos_token_id=None, attention_mask=mask))
    out_ids, masks = _guarded("evaluate", lambda: m.evaluate(clip.to(DEV), images, ids, resize, orig, max_new_tokens=3, eos_token_id=None, attention_mask=mask))
    assert torch.equal(out_ids, seq) and len(masks) == 3
    n_seg = (out_ids[:, 1:] == cfg.seg_token_idx).sum(1).tolist()                                          # row 0 keeps the [SEG] of its prompt; the cut rows lost theirs
    assert n_seg[0] >= 1 and [tuple(x.shape) for x in masks] == [(n, h, w) for n, (h, w) in zip(n_seg, orig)]
