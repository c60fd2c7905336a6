"""Decode-step timing of batched greedy generation at Llama-7B size (random weights) for prompts of EQUAL length (the uniform route: one device-side
position) against prompts whose lengths are SPREAD over 64 tokens (`generate(attention_mask=)`: one position per sequence), at N = 2, 4, 8 sequences, with
bf16 weights and with weight_bits=8.  The longest prompt has 128 tokens in both layouts, so both run at the same cache capacity.  ms per token = the
difference of a 2-token and a `new_tokens`-token call over the steps between them; every figure is taken `reps` times.
usage: python tools/decode_ragged_bench.py [new_tokens=24] [reps=3] [--uniform-only]
  --uniform-only: the equal-length layout alone, without the attention_mask keyword (runs on a tree that does not have it: the parent's figures)
One JSON line per figure; profiles/ragged_decode.md is written from them."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llmseg_amd.lisa import LISAForCausalLM  # noqa: E402
from llmseg_amd.params import LisaConfig, LlamaConfig  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
UNIFORM_ONLY = "--uniform-only" in sys.argv
NEW = int(args[0]) if len(args) > 0 else 24
REPS = int(args[1]) if len(args) > 1 else 3
LMAX, SPREAD = 128, 64
dev = torch.device("cuda:0")
cfg = LisaConfig(backbone="sam", build_unused_towers=False)
cfg.llama = LlamaConfig(lora_r=8)
m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
m.prepare()
g = torch.Generator().manual_seed(1)


def timed(**kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.generate(**kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for N in (2, 4, 8):
    ids = torch.randint(3, 31999, (N, LMAX), generator=g)
    ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
    clip = torch.randn(N, 3, 224, 224, generator=g).to(dev, torch.bfloat16)
    lens = [LMAX - (SPREAD * i) // (N - 1) for i in range(N)]          # LMAX .. LMAX - 64, evenly
    mask = torch.arange(LMAX)[None, :] < torch.tensor(lens)[:, None]
    for bits in (None, 8):
        for layout in ("equal",) if UNIFORM_ONLY else ("equal", "spread"):
            kw = dict(images_clip=clip, input_ids=ids, eos_token_id=None, weight_bits=bits)
            if layout == "spread":
                kw["attention_mask"] = mask
            timed(max_new_tokens=NEW, **kw)                    # warm-up: allocations, the captured step
            per = []
            for _ in range(REPS):
                t_a = timed(max_new_tokens=2, **kw)
                t_b = timed(max_new_tokens=NEW, **kw)
                per.append((t_b - t_a) / (NEW - 2) * 1e3)
            print(json.dumps(dict(N=N, weight_bits=bits, layout=layout, lens=lens if layout == "spread" else [LMAX] * N, new_tokens=NEW,
                                  ms_per_token=[round(p, 3) for p in per])), flush=True)
