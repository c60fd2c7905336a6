"""Digests for comparing two builds of `generate()`'s front end bit for bit: the first 16 hex digits of the SHA-256 of every result tensor of `generate()` (5 new
tokens, use_graph True and False) on the tiny head_dim-128 model (LoRA rank 8) of tests/test_beam_gpu.py, on every route the call can take before and at the pick:
  * greedy, two prompts of one length and the ragged pair of 24 and 17 tokens, without an eos and with one that a row emits before the end (taken from the run
    without: the early stop and the pad path run);
  * sampled (temperature 0.8, top_k 50, top_p 0.9, fixed uniforms, return_logprobs), uniform and ragged;
  * the four logits controls, each alone, penalty and n-gram ban together, all four with min_new_tokens=2 and an eos, and all four on the ragged sampled route;
  * fuse_decode=False;
  * num_beams 2 and 3 with beam_cache "indirect" and "copy" and return_beam_scores, and with an eos at length_penalty 0.5 / 2.0 and early_stopping both ways;
  * weight_bits=8 and weight_format="mxfp4": greedy ragged, sampled, two beams.
The file imports the package of the checkout it lies in.  Copy it into tools/ of a checkout of another commit, run both, `diff` the outputs.
usage: python tools/generate_digests.py > digests.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from llmseg_amd import _lib  # noqa: E402
from llmseg_amd.generate import pad_prompts  # noqa: E402
from tests import test_beam_gpu as tb  # noqa: E402

assert os.path.realpath(_lib.LIB_PATH).startswith(os.path.realpath(ROOT)), (_lib.LIB_PATH, ROOT)
DEV = "cuda"
MAX_NEW = 5


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


m = tb._hip_model(8)
_, clip0, ids0, _ = tb._prompts()
clip, ids = clip0[:2].to(DEV), ids0[:2].to(DEV)
rids, rmask = (t.to(DEV) for t in pad_prompts([ids0[0, :24], ids0[1, :17]], 0))
UNIFORM, RAGGED = dict(input_ids=ids), dict(input_ids=rids, attention_mask=rmask)
us = torch.rand((2, MAX_NEW), dtype=torch.float32, generator=torch.Generator().manual_seed(11)).to(DEV)
SAMPLED = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, uniforms=us, return_logprobs=True)


def run(name, input_ids, eos_token_id=None, **kw):
    """-> the results of the use_graph=True call"""
    first = None
    for graph in (True, False):
        res = tb._guarded(name, lambda: m.generate(clip, input_ids, max_new_tokens=MAX_NEW, eos_token_id=eos_token_id, pad_token_id=0, use_graph=graph, **kw))
        torch.cuda.synchronize()
        print(f"GEN {name} graph={int(graph)} eos={eos_token_id} " + " ".join(sha(t) for t in res), flush=True)
        first = res if first is None else first
    print(f"NEW {name} " + " ".join(str(r[-(MAX_NEW + 7):]) for r in first[0].tolist()).replace(", ", ","), flush=True)      # every row's tail (new tokens, fill): what the route exercised
    return first


def early_eos(new):
    """new tokens [N, n] of a run without an eos -> a token that a row emits before its last step, if possible one the other rows emit later or not at all"""
    rows = new.tolist()
    cands = [(k, t, i) for i, r in enumerate(rows) for k, t in enumerate(r[:-1])]
    alone = [c for c in cands if all(c[1] not in r[:c[0] + 1] for j, r in enumerate(rows) if j != c[2])]
    return min(alone or cands)[1]


for route, prompts in (("uniform", UNIFORM), ("ragged", RAGGED)):
    L = prompts["input_ids"].shape[1]
    lens = [L, L] if route == "uniform" else [24, 17]
    seq = run(f"greedy_{route}", **prompts)[0]
    new = torch.stack([seq[i, n:n + MAX_NEW] for i, n in enumerate(lens)]).cpu()
    eos = early_eos(new)
    run(f"greedy_{route}_eos", eos_token_id=eos, **prompts)
    run(f"sampled_{route}", **prompts, **SAMPLED)
    if route == "uniform":
        ban = sorted(set(new[:, 0].tolist()))                  # the first token every row would emit
        ALL = dict(repetition_penalty=0.2, no_repeat_ngram_size=2, min_new_tokens=2, suppress_tokens=ban)      # (a penalty below 1 rewards repeats: the n-gram ban then bites)
        run("controls_repetition_penalty", repetition_penalty=0.2, **prompts)
        run("controls_no_repeat_ngram", no_repeat_ngram_size=1, **prompts)
        run("controls_penalty_and_ngram", repetition_penalty=0.2, no_repeat_ngram_size=2, **prompts)
        run("controls_min_new_tokens", min_new_tokens=2, eos_token_id=eos, **prompts)
        run("controls_suppress", suppress_tokens=ban, **prompts)
        run("controls_all_eos", eos_token_id=eos, **ALL, **prompts)
        run("greedy_unfused", fuse_decode=False, **prompts)
    else:
        run("controls_all_ragged_sampled", eos_token_id=eos, **ALL, **prompts, **SAMPLED)

L = ids.shape[1]
for B in (2, 3):
    for cache in ("indirect", "copy"):
        seq = run(f"beams{B}_{cache}", ids, num_beams=B, beam_cache=cache, return_beam_scores=True)[0]
    eos = early_eos(seq[:, L:L + MAX_NEW].cpu())
    for lp in (0.5, 2.0):
        for early in (False, True):
            run(f"beams{B}_lp{lp}_early{int(early)}", ids, eos_token_id=eos, num_beams=B, length_penalty=lp, early_stopping=early, return_beam_scores=True)

for mode, kw in (("w8", dict(weight_bits=8)), ("mxfp4", dict(weight_format="mxfp4"))):
    run(f"{mode}_greedy_ragged", **RAGGED, **kw)
    run(f"{mode}_sampled", **UNIFORM, **SAMPLED, **kw)
    run(f"{mode}_beams2", **UNIFORM, num_beams=2, return_beam_scores=True, **kw)
