"""Digests for comparing two builds of the quantised decode path bit for bit: the first 16 hex digits of the SHA-256 of
  * the whole guarded output buffer of `ops.gemm_w8` on every case of tests/w8_checks.py and of `ops.gemm_mxfp4` on every case of tests/mxfp4_checks.py, on the seeded
    operands of `inputs(case)`, sliced as the GPU parity tests slice them;
  * every result of `generate()` (5 new tokens, no eos, use_graph True and False) on the tiny head_dim-128 model (LoRA rank 8) at weight_bits=8 x {1, 2, 9 rows} and
    weight_format="mxfp4" x {1, 3, 9 rows}, and per mode a ragged, a sampled and a num_beams=2 call;
  * all packed rows and scales of `decode_weights_i8()` / `decode_weights_mxfp4()` after those calls (the quantisers' outputs).
The file imports the package of the checkout it lies in.  Copy it into tools/ of a checkout of another commit, run both, `diff` the outputs.
usage: python tools/decode_gemm_digests.py > digests.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from llmseg_amd import _lib, ops  # noqa: E402
from llmseg_amd.generate import pad_prompts  # noqa: E402
from tests import mxfp4_checks as xc, test_beam_gpu as tb, w8_checks as wc  # noqa: E402

assert os.path.realpath(_lib.LIB_PATH).startswith(os.path.realpath(ROOT)), (_lib.LIB_PATH, ROOT)
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


for case in wc.cases():
    inp = wc.inputs(case)
    M, N, K = case.M, case.N, case.K
    lda, ldq, ldc, ldr = wc.dims(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    cb = torch.full((M + 1, ldc), wc.NAN, dtype=F32 if case.f32 else BF, device=DEV)
    ops.gemm_w8(d["a"][:M, :K], d["q"][:N, :K], d["scale"][:N], residual=d["res"][:, :N] if case.res else None, out=cb[:M, :N])
    torch.cuda.synchronize()
    print(f"GEMM w8 {case.name} {sha(cb)}", flush=True)

for case in xc.cases():
    inp = xc.inputs(case)
    M, N, K = case.M, case.N, case.K
    lda, ldq, lds, ldc, ldr = xc.dims(case)
    d = {k: v.to(DEV) for k, v in inp.items()}
    cb = torch.full((M + 1, ldc), xc.NAN, dtype=F32 if case.f32 else BF, device=DEV)
    ops.gemm_mxfp4(d["a"][:M, :K], d["q"][:N, :K // 2], d["scale"][:N, :K // 32], residual=d["res"][:, :N] if case.res else None, out=cb[:M, :N])
    torch.cuda.synchronize()
    print(f"GEMM mxfp4 {case.name} {sha(cb)}", flush=True)

m = tb._hip_model(8)
_, clip0, ids0, _ = tb._prompts()
MODES = {"w8": dict(weight_bits=8), "mxfp4": dict(weight_format="mxfp4")}
ROWS = {"w8": (1, 2, 9), "mxfp4": (1, 3, 9)}


def run(name, clip, ids, **kw):
    for graph in (True, False):
        res = tb._guarded(name, lambda: m.generate(clip.to(DEV), ids.to(DEV), max_new_tokens=5, eos_token_id=None, pad_token_id=0, use_graph=graph, **kw))
        torch.cuda.synchronize()
        print(f"GEN {name} graph={int(graph)} " + " ".join(sha(t) for t in res), flush=True)


for mode, kw in MODES.items():
    for n in ROWS[mode]:
        reps = -(-n // 3)
        run(f"{mode}_n{n}", clip0.repeat(reps, 1, 1, 1)[:n], ids0.repeat(reps, 1)[:n], **kw)
    ids, mask = pad_prompts([ids0[0, :24], ids0[1, :17]], 0)
    run(f"{mode}_ragged", clip0[:2], ids, attention_mask=mask.to(DEV), **kw)
    us = torch.rand((2, 5), dtype=F32, generator=torch.Generator().manual_seed(11)).to(DEV)
    run(f"{mode}_sampled", clip0[:2], ids0[:2], do_sample=True, temperature=0.8, top_k=50, top_p=0.9, uniforms=us, return_logprobs=True, **kw)
    run(f"{mode}_beams2", clip0[:2], ids0[:2], num_beams=2, return_beam_scores=True, **kw)
    w = m.decode_weights_i8() if mode == "w8" else m.decode_weights_mxfp4()
    h = hashlib.sha256()
    for k in sorted(w):
        for t in w[k]:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    print(f"WEIGHTS {mode} {h.hexdigest()[:16]}", flush=True)
