"""Timing of sampling (generate(do_sample=True), llmseg_sample_tokens) on the GPU.
  kernel: the sampling launch alone on seeded bf16 logits 3 * randn [N, V] (V = 32003 unless given), for a few (T, k, p) settings: microseconds per launch from a pair
          of device events around `iters` back-to-back launches, median of `repeats` such windows after a warm-up window.  One launch reads the row once (64 KB
          per row): the figure is latency, not bandwidth.
  decode: ms per decoded token at Llama-7B size (random weights, 64-token prompt), greedy and sampled ALTERNATING in one process:
          (a call generating NEW tokens - a call generating 2) / (NEW - 2), so prefill and LoRA merge cancel; median (min .. max) of `repeats` pairs per mode.
          modes = greedy passes no sampling argument at all, so the same file times a tree that does not have the feature yet.
usage: python tools/sampling_bench.py kernel [N list=1,8] [iters=2000] [repeats=7] [json out] [V=32003]
       python tools/sampling_bench.py decode [modes=greedy,sampled] [N list=1,8] [new_tokens=66] [repeats=7] [json out]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "kernel"
assert MODE in ("kernel", "decode"), __doc__
assert torch.cuda.is_available(), "sampling_bench needs a GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
rows = []

if MODE == "kernel":
    from llmseg_amd import ops
    NS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,8").split(",")]
    ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    REP = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    OUT = sys.argv[5] if len(sys.argv) > 5 else None
    V = int(sys.argv[6]) if len(sys.argv) > 6 else 32003
    for N in NS:
        g = torch.Generator().manual_seed(N)
        logits = (3.0 * torch.randn(N, V, generator=g)).to(dev, torch.bfloat16)
        u = torch.rand(N, generator=g).to(dev)
        unfinished = torch.ones(N, dtype=torch.int64, device=dev)
        nxt = torch.empty(N, dtype=torch.int64, device=dev)
        lp = torch.empty(N, dtype=torch.float32, device=dev)
        for name, (T, k, p) in (("T only", (0.7, 0, 1.0)), ("top-k 50", (0.7, 50, 1.0)), ("top-p 0.9", (0.7, 0, 0.9)), ("top-k 50 + top-p 0.9", (0.7, 50, 0.9))):
            def window():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(ITERS):
                    ops.sample_tokens(logits, T, k, p, u, eos_token_id=2, pad_token_id=0, unfinished=unfinished, next=nxt, logprob=lp)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / ITERS * 1e3
            window()
            us = [window() for _ in range(REP)]
            rows.append(dict(mode="kernel", N=N, V=V, setting=name, T=T, k=k, p=p, us_per_launch=statistics.median(us), us_min=min(us), us_max=max(us), iters=ITERS, repeats=REP))
            print(f"kernel N={N} V={V} {name}: {statistics.median(us):.2f} us per launch ({min(us):.2f} .. {max(us):.2f}, {REP} windows of {ITERS})", flush=True)
else:
    from llmseg_amd.lisa import LISAForCausalLM
    from llmseg_amd.params import LisaConfig, LlamaConfig
    MODES = (sys.argv[2] if len(sys.argv) > 2 else "greedy,sampled").split(",")
    NS = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,8").split(",")]
    NEW = int(sys.argv[4]) if len(sys.argv) > 4 else 66
    REP = int(sys.argv[5]) if len(sys.argv) > 5 else 7
    OUT = sys.argv[6] if len(sys.argv) > 6 else None
    assert set(MODES) <= {"greedy", "sampled"} and NEW > 2 and REP >= 1
    KW = {"greedy": {}, "sampled": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=0)}
    cfg = LisaConfig(backbone="sam", build_unused_towers=False)
    cfg.llama = LlamaConfig(lora_r=8)
    m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
    m.prepare()

    def timed(clip, ids, new, kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate(clip, ids, max_new_tokens=new, eos_token_id=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for N in NS:
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(3, 31999, (N, 64), generator=g)
        ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
        clip = torch.randn(N, 3, 224, 224, generator=g).to(dev, torch.bfloat16)
        for mode in MODES:                                                 # warm-up: allocations, code objects, the step's graph
            timed(clip, ids, 2, KW[mode]); timed(clip, ids, NEW, KW[mode])
        per = {mode: [] for mode in MODES}
        for _ in range(REP):
            for mode in MODES:                                             # alternating: drift of the box hits every mode alike
                ta = timed(clip, ids, 2, KW[mode])
                tb = timed(clip, ids, NEW, KW[mode])
                per[mode].append((tb - ta) / (NEW - 2) * 1e3)
        for mode in MODES:
            x = per[mode]
            rows.append(dict(mode=mode, N=N, ms_per_token=statistics.median(x), ms_min=min(x), ms_max=max(x), repeats=REP, new_tokens=NEW))
            print(f"decode N={N} {mode}: {statistics.median(x):.3f} ms/token ({min(x):.3f} .. {max(x):.3f}, {REP} pairs)", flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1)
