"""Decode-step timing of generate(weight_format="mxfp4") beside the int8 and the bf16 path at Llama-7B size, random weights, 64-token prompt.
The weight stream of a token is every decoder weight + lm_head once: 13.21 GB at bf16, 6.74 GB with the four per-layer matrices as int8 rows, 3.70 GB with
them as MXFP4 rows (4 bits + one scale byte per 32; lm_head stays bf16).

steps:   ms per generated token for N sequences = (time of a call generating NEW tokens - time of a call generating 2) / (NEW - 2): prefill, merge and
         quantisation cancel.  Median of `repeats` such pairs after a warm-up pair (min .. max beside it); the quantised modes also report the per-call
         merge + quantisation cost (device events) and prefill + first token.
shapes:  back-to-back launches of one GEMM shape replayed from a hipGraph, rotating over 6 weight buffers (every launch reads cold rows): us per launch and TB/s of the weight
         bytes for `gemm_mxfp4`, `gemm_w8` and the bf16 skinny kernel at 1 / 2 / 4 / 8 rows, and the four shapes x 32 layers.

usage: python tools/decode_mxfp4_bench.py steps  [modes=16,8,mxfp4] [N list=1,2,4,8] [new_tokens=66] [repeats=7] [lora_r=8] [json out]
       python tools/decode_mxfp4_bench.py shapes [launches=60] [json out]
mode 16 passes no weight argument at all, so `steps 16` of this file also times a tree that does not have the mode yet."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

assert len(sys.argv) > 1 and sys.argv[1] in ("steps", "shapes"), __doc__
assert torch.cuda.is_available(), "decode_mxfp4_bench needs a GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
H, INTER, LAYERS = 4096, 11008, 32
SHAPES = (("q|k|v", 3 * H, H), ("o_proj", H, H), ("gate|up", 2 * INTER, H), ("down_proj", H, INTER))


def shapes():
    from llmseg_amd import ops
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    out = sys.argv[3] if len(sys.argv) > 3 else None
    ROT = 6
    rows, total = [], {}
    for name, N, K in SHAPES:
        w = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(ROT)]
        q8 = [ops.quantize_rows_i8(x) for x in w]
        q4 = [ops.quantize_rows_mxfp4(x) for x in w]
        for M in (1, 2, 4, 8):
            a = torch.randn(M, K, device=dev).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev).to(torch.bfloat16)
            o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            forms = {"mxfp4": (lambda i: ops.gemm_mxfp4(a, *q4[i], residual=res, out=o), N * (K // 2 + K // 32)),
                     "int8": (lambda i: ops.gemm_w8(a, *q8[i], residual=res, out=o), N * (K + 4)),
                     "bf16": (lambda i: ops.gemm(a, w[i], residual=res, out=o), 2 * N * K)}
            row = dict(shape=name, N=N, K=K, rows=M)
            for form, (fn, nbytes) in forms.items():
                for i in range(2 * ROT):
                    fn(i % ROT)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()                  # the launches as one graph: the host issues a launch in ~10 us, longer than most of these kernels run
                with torch.cuda.graph(graph):
                    for i in range(launches):
                        fn(i % ROT)
                graph.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                graph.replay()
                e1.record()
                e1.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / launches
                del graph
                row[form + "_us"], row[form + "_tb_s"] = us, nbytes / us / 1e6
                total[(form, M)] = total.get((form, M), 0.0) + us
            rows.append(row)
            print(f"{name:9s} {N:5d} x {K:5d} rows {M}: " + "  ".join(f"{f} {row[f + '_us']:6.1f} us {row[f + '_tb_s']:.2f} TB/s" for f in forms), flush=True)
        del w, q8, q4
    for M in (1, 2, 4, 8):
        print(f"the four x {LAYERS} layers, rows {M}: " + "  ".join(f"{f} {total[(f, M)] * LAYERS / 1e3:.2f} ms" for f in ("mxfp4", "int8", "bf16")), flush=True)
        rows.append(dict(shape="four_x_layers", rows=M, **{f + "_ms": total[(f, M)] * LAYERS / 1e3 for f in ("mxfp4", "int8", "bf16")}))
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


def steps():
    from llmseg_amd.lisa import LISAForCausalLM
    from llmseg_amd.params import LisaConfig, LlamaConfig
    modes = (sys.argv[2] if len(sys.argv) > 2 else "16,8,mxfp4").split(",")
    NS = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,2,4,8").split(",")]
    NEW = int(sys.argv[4]) if len(sys.argv) > 4 else 66
    REP = int(sys.argv[5]) if len(sys.argv) > 5 else 7
    R = int(sys.argv[6]) if len(sys.argv) > 6 else 8
    out = sys.argv[7] if len(sys.argv) > 7 else None
    assert set(modes) <= {"16", "8", "mxfp4"} and NEW > 2 and REP >= 1
    cfg = LisaConfig(backbone="sam", build_unused_towers=False)
    cfg.llama = LlamaConfig(lora_r=R)
    m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
    m.prepare()
    c = cfg.llama
    assert (c.hidden, c.inter, c.layers) == (H, INTER, LAYERS)
    layer_w = c.layers * (4 * c.hidden * c.hidden + 3 * c.hidden * c.inter)
    rows_w = c.layers * (3 * c.hidden + c.hidden + 2 * c.inter + c.hidden)
    head = 2.0 * c.vocab * c.hidden
    GB = {"16": (2.0 * layer_w + head) / 1e9, "8": (1.0 * layer_w + 4.0 * rows_w + head) / 1e9, "mxfp4": (layer_w * (0.5 + 1.0 / 32) + head) / 1e9}
    KW = {"16": {}, "8": {"weight_bits": 8}, "mxfp4": {"weight_format": "mxfp4"}}
    PREP = {"8": "w8_prepare_ms", "mxfp4": "mxfp4_prepare_ms"}

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
        for mode in modes:
            kw = KW[mode]
            timed(clip, ids, 2, kw); timed(clip, ids, NEW, kw)              # warm-up: allocations, code objects, the step's graph
            per, prep, first = [], [], []
            for _ in range(REP):
                ta = timed(clip, ids, 2, kw)
                tb = timed(clip, ids, NEW, kw)
                per.append((tb - ta) / (NEW - 2) * 1e3)
                first.append(ta * 1e3)
                if mode in PREP:
                    prep.append(getattr(m, PREP[mode])())
            row = dict(N=N, mode=mode, ms_per_token=statistics.median(per), ms_min=min(per), ms_max=max(per), gb_per_token=GB[mode],
                       tb_per_s=GB[mode] / statistics.median(per), prefill_plus_2_ms=statistics.median(first), repeats=REP, new_tokens=NEW, lora_r=R)
            if prep:
                row.update(prepare_ms=statistics.median(prep), prepare_min=min(prep), prepare_max=max(prep))
            rows.append(row)
            print(f"N={N} mode={mode}: {row['ms_per_token']:.3f} ms/token ({row['ms_min']:.3f} .. {row['ms_max']:.3f}, {REP} pairs), stream {GB[mode]:.2f} GB/token -> "
                  f"{row['tb_per_s']:.2f} TB/s; call of 2 tokens {row['prefill_plus_2_ms']:.1f} ms" +
                  (f"; merge + quantise {row['prepare_ms']:.2f} ms per call ({row['prepare_min']:.2f} .. {row['prepare_max']:.2f})" if prep else ""), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


shapes() if sys.argv[1] == "shapes" else steps()
