"""Beam-search decode timing at Llama-7B size (random weights): ms per token of generate(num_beams=B) with the beam-indexed cache ("indirect"), with the
physically re-ordered cache ("copy"), and of the greedy route at N * B sequences (the route beam search leaves untouched: the yardstick), interleaved in one
process; then `ops.beam_step` alone against the torch sequence it replaces (log_softmax + add + topk(2 B)).  T = 319 prompt positions (L = 64 ids + the image
tokens), HIP events around whole calls, graph replay; ms per token = (a `new_tokens` call - a 2-token call) / (new_tokens - 2).
usage: python tools/beam_bench.py [new_tokens=32] [reps=3] [beams=4]
One JSON line per figure; profiles/beam_search.md is written from them."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llmseg_amd import ops  # noqa: E402
from llmseg_amd.lisa import LISAForCausalLM  # noqa: E402
from llmseg_amd.params import LisaConfig, LlamaConfig  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
NEW = int(args[0]) if len(args) > 0 else 32
REPS = int(args[1]) if len(args) > 1 else 3
B = int(args[2]) if len(args) > 2 else 4
dev = torch.device("cuda:0")
cfg = LisaConfig(backbone="sam", build_unused_towers=False)
cfg.llama = LlamaConfig(lora_r=8)
m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
m.prepare()
g = torch.Generator().manual_seed(1)
L = 319 + 1 - cfg.n_img_tokens


def timed(**kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    m.generate(**kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def prompts(n):
    ids = torch.randint(3, 31999, (n, L), generator=g)
    ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
    return ids, torch.randn(n, 3, 224, 224, generator=g).to(dev, torch.bfloat16)


for N in (1, 2):
    ids, clip = prompts(N)
    ids_g, clip_g = ids.repeat_interleave(B, 0), clip.repeat_interleave(B, 0)
    modes = {"indirect": dict(images_clip=clip, input_ids=ids, num_beams=B, beam_cache="indirect"), "copy": dict(images_clip=clip, input_ids=ids, num_beams=B, beam_cache="copy"),
             "greedy_NB": dict(images_clip=clip_g, input_ids=ids_g)}
    per = {k: [] for k in modes}
    for kw in modes.values():
        timed(max_new_tokens=NEW, eos_token_id=None, **kw)     # warm-up: allocations, the captured step
    for _ in range(REPS):                                      # interleaved: every mode once per repetition
        for k, kw in modes.items():
            t_a = timed(max_new_tokens=2, eos_token_id=None, **kw)
            t_b = timed(max_new_tokens=NEW, eos_token_id=None, **kw)
            per[k].append((t_b - t_a) / (NEW - 2))
    for k in modes:
        print(json.dumps(dict(N=N, beams=B, rows=N * B, mode=k, T=319, new_tokens=NEW, ms_per_token=[round(p, 3) for p in per[k]])), flush=True)

# the pick alone: llmseg_beam_step (two launches) against log_softmax + add + topk(2 B) in torch, 32000 logits per row
V, cap = 32000, 384
for N in (1, 2):
    R = N * B
    logits = torch.randn(R, V, generator=g).to(dev, torch.bfloat16)
    scores = -torch.rand(R, generator=g).to(dev)
    done = torch.zeros(N, dtype=torch.int32, device=dev)
    src_a, src_b = torch.zeros((R, cap), dtype=torch.int32, device=dev), torch.zeros((R, cap), dtype=torch.int32, device=dev)
    pos = torch.full((R,), 350, dtype=torch.int32, device=dev)
    out = ops.beam_step(logits, scores, done, src_a, src_b, pos, B)
    ws = torch.empty((R * 2 * B,), dtype=torch.int64, device=dev)

    def ours():
        ops.beam_step(logits, scores, done, src_a, src_b, pos, B, out=out, workspace=ws)

    def torch_seq():
        lp = torch.log_softmax(logits.float(), -1) + scores[:, None]
        return torch.topk(lp.view(N, B * V), 2 * B, dim=1)

    res = {}
    for name, fn in (("beam_step", ours), ("torch", torch_seq)) * REPS:
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        e1.synchronize()
        res.setdefault(name, []).append(round(e0.elapsed_time(e1) / 50 * 1e3, 1))
    print(json.dumps(dict(N=N, beams=B, V=V, pick_us=res)), flush=True)
