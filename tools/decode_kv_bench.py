"""Decode-step timing of generate(kv_format="mxfp8") beside the bf16 KV cache at Llama-7B size, random weights, 64-token prompt (319 keys after the prefill).
A cached token is 2 x 32 x 4096 values per sequence: 512 KiB in bf16, 264 KiB as E4M3 bytes with one E8M0 scale byte per 32.

ms per generated token = (time of a call generating PAST + NEW tokens - time of a call generating PAST + 2) / (NEW - 2): the prefill (and the quantisation of its K
and V), the merge and the weight quantisation cancel, and with PAST > 0 so do the first PAST steps: the figure is the step at a context of about 319 + PAST keys.
The two cache formats ALTERNATE pair by pair in one session; median of `repeats` pairs after a warm-up pair (min .. max beside it).  The call of PAST + 2 tokens
at PAST = 0 is the prefill + 2 tokens: its difference between the formats is what the quantiser costs in the prefill (64 launches at 32 layers).

cases: g1, g8 = greedy at 1 and 8 sequences; b4, b16 = 3 prompts x 4 and x 16 beams (beam_cache="indirect").  weights: 16 = bf16, mxfp4.

usage: python tools/decode_kv_bench.py [cases=g1,g8,b4,b16] [weights=16,mxfp4] [past=0,512] [new_tokens=34] [repeats=5] [lora_r=8] [json out]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

assert torch.cuda.is_available(), "decode_kv_bench needs a GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
CASES = {"g1": (1, 1), "g8": (8, 1), "b4": (3, 4), "b16": (3, 16)}          # name -> (prompts, beams)


def main():
    from llmseg_amd.lisa import LISAForCausalLM
    from llmseg_amd.params import LisaConfig, LlamaConfig
    arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
    cases, weights = arg(1, "g1,g8,b4,b16").split(","), arg(2, "16,mxfp4").split(",")
    pasts = [int(x) for x in arg(3, "0,512").split(",")]
    NEW, REP, R, out = int(arg(4, "34")), int(arg(5, "5")), int(arg(6, "8")), arg(7, None)
    assert set(cases) <= set(CASES) and set(weights) <= {"16", "mxfp4"} and NEW > 2 and REP >= 1
    cfg = LisaConfig(backbone="sam", build_unused_towers=False)
    cfg.llama = LlamaConfig(lora_r=R)
    m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
    m.prepare()
    c = cfg.llama
    tok_kib = {None: 2 * c.layers * c.hidden * 2 / 1024, "mxfp8": 2 * c.layers * c.hidden * (1 + 1 / 32) / 1024}

    def timed(clip, ids, new, kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate(clip, ids, max_new_tokens=new, eos_token_id=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    rows = []
    for case in cases:
        N, B = CASES[case]
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(3, 31999, (N, 64), generator=g)
        ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
        clip = torch.randn(N, 3, 224, 224, generator=g).to(dev, torch.bfloat16)
        T = ids.shape[1] - 1 + cfg.n_img_tokens
        for w in weights:
            for past in pasts:
                base = dict({} if w == "16" else {"weight_format": w}, **({"num_beams": B} if B > 1 else {}))
                kws = {None: base, "mxfp8": dict(base, kv_format="mxfp8")}
                for kw in kws.values():                                         # warm-up: allocations, code objects, the states and their graphs
                    timed(clip, ids, past + 2, kw); timed(clip, ids, past + NEW, kw)
                per, first = {k: [] for k in kws}, {k: [] for k in kws}
                for _ in range(REP):
                    for k, kw in kws.items():                                   # alternating: one pair per format and repeat
                        ta = timed(clip, ids, past + 2, kw)
                        tb = timed(clip, ids, past + NEW, kw)
                        per[k].append((tb - ta) / (NEW - 2) * 1e3)
                        first[k].append(ta * 1e3)
                row = dict(case=case, prompts=N, beams=B, weights=w, keys_from=T + past + 2, keys_to=T + past + NEW, repeats=REP, new_tokens=NEW, lora_r=R)
                for k in kws:
                    name = "bf16" if k is None else k
                    row.update({f"{name}_ms_per_token": statistics.median(per[k]), f"{name}_ms_min": min(per[k]), f"{name}_ms_max": max(per[k]),
                                f"{name}_call_of_{past + 2}_ms": statistics.median(first[k]),
                                f"{name}_kv_gb_per_step": N * B * (T + past + NEW / 2) * tok_kib[k] * 1024 / 1e9})
                rows.append(row)
                print(f"{case} ({N} x {B} rows) weights={w} keys {row['keys_from']}..{row['keys_to']}: "
                      f"bf16 cache {row['bf16_ms_per_token']:.3f} ms/token ({row['bf16_ms_min']:.3f} .. {row['bf16_ms_max']:.3f}), "
                      f"mxfp8 cache {row['mxfp8_ms_per_token']:.3f} ({row['mxfp8_ms_min']:.3f} .. {row['mxfp8_ms_max']:.3f}), {REP} alternating pairs; K+V read per step "
                      f"{row['bf16_kv_gb_per_step']:.2f} / {row['mxfp8_kv_gb_per_step']:.2f} GB; call of {past + 2} tokens {row[f'bf16_call_of_{past + 2}_ms']:.1f} / "
                      f"{row[f'mxfp8_call_of_{past + 2}_ms']:.1f} ms", flush=True)
                if out:
                    with open(out, "w") as f:
                        json.dump(rows, f, indent=1)
            m.__dict__.pop("_decode_states", None)                              # the next weight mode starts from an empty pool of states
            torch.cuda.empty_cache()


main()
