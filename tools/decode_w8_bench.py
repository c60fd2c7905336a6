"""Decode-step timing of generate(weight_bits=8) beside the bf16 path at Llama-7B size, random weights, 64-token prompt: ms per generated token for
N = 1, 2, 4, 8 sequences and, for the int8 mode, the per-call cost of the LoRA merge + quantisation.  The weight stream of a token is every decoder
weight + lm_head once: 13.2 GB at bf16, 6.9 GB with the four per-layer matrices as int8 rows (lm_head stays bf16).
ms per token = (time of a call generating NEW tokens - time of a call generating 2) / (NEW - 2): prefill, merge and quantisation cancel.  Each figure is the
median of `repeats` such pairs after a warm-up pair (min .. max beside it).
usage: python tools/decode_w8_bench.py [bits=16|8|both] [N list=1,2,4,8] [new_tokens=24] [repeats=5] [lora_r=8] [json out]
bits = 16 passes no weight_bits argument at all, so the same file times a tree that does not have the mode yet."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llmseg_amd.lisa import LISAForCausalLM  # noqa: E402
from llmseg_amd.params import LisaConfig, LlamaConfig  # noqa: E402

BITS = sys.argv[1] if len(sys.argv) > 1 else "both"
NS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,2,4,8").split(",")]
NEW = int(sys.argv[3]) if len(sys.argv) > 3 else 24
REP = int(sys.argv[4]) if len(sys.argv) > 4 else 5
R = int(sys.argv[5]) if len(sys.argv) > 5 else 8
OUT = sys.argv[6] if len(sys.argv) > 6 else None
assert BITS in ("16", "8", "both") and NEW > 2 and REP >= 1

assert torch.cuda.is_available(), "decode_w8_bench needs a GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
cfg = LisaConfig(backbone="sam", build_unused_towers=False)
cfg.llama = LlamaConfig(lora_r=R)
m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
m.prepare()
c = cfg.llama
layer_w = c.layers * (4 * c.hidden * c.hidden + 3 * c.hidden * c.inter)
scales = 4.0 * c.layers * (3 * c.hidden + c.hidden + 2 * c.inter + c.hidden)
GB = {16: (2.0 * layer_w + 2.0 * c.vocab * c.hidden) / 1e9, 8: (1.0 * layer_w + scales + 2.0 * c.vocab * c.hidden) / 1e9}


def timed(clip, ids, new, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.generate(clip, ids, max_new_tokens=new, eos_token_id=None, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


rows = []
for N in NS:
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 31999, (N, 64), generator=g)
    ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
    clip = torch.randn(N, 3, 224, 224, generator=g).to(dev, torch.bfloat16)
    for bits in ((16, 8) if BITS == "both" else (int(BITS),)):
        kw = {} if bits == 16 else {"weight_bits": 8}
        timed(clip, ids, 2, kw); timed(clip, ids, NEW, kw)              # warm-up: allocations, code objects, the step's graph
        per, prep = [], []
        for _ in range(REP):
            ta = timed(clip, ids, 2, kw)
            tb = timed(clip, ids, NEW, kw)
            per.append((tb - ta) / (NEW - 2) * 1e3)
            if bits == 8:
                prep.append(m.w8_prepare_ms())
        row = dict(N=N, bits=bits, ms_per_token=statistics.median(per), ms_min=min(per), ms_max=max(per), gb_per_token=GB[bits],
                   tb_per_s=GB[bits] / statistics.median(per), prefill_plus_1_ms=ta * 1e3, repeats=REP, new_tokens=NEW, lora_r=R)
        if prep:
            row.update(prepare_ms=statistics.median(prep), prepare_min=min(prep), prepare_max=max(prep))
        rows.append(row)
        print(f"N={N} bits={bits}: {row['ms_per_token']:.3f} ms/token ({row['ms_min']:.3f} .. {row['ms_max']:.3f}, {REP} pairs), stream {GB[bits]:.2f} GB/token -> "
              f"{row['tb_per_s']:.2f} TB/s" + (f"; merge + quantise {row['prepare_ms']:.2f} ms per call ({row['prepare_min']:.2f} .. {row['prepare_max']:.2f})" if prep else ""),
              flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1)
