"""Timing of the logits processors (generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=), llmseg_logits_process) on the GPU,
against the torch route: Hugging Face's own four processor objects (RepetitionPenalty, NoRepeatNGram, MinNewTokensLength, SuppressTokens) on the device, applied at
the same place in the loop with `input_ids` grown by torch.cat as HF's loop does (if transformers does not import: the restated rule of
tests/logits_process_checks.py, which runs on the CPU).  Settings everywhere: theta = 1.2, g = 3, two suppressed ids and a banned token.
  kernel: the launch alone on seeded bf16 logits 3 * randn [N, V] with a random in-range history of `hist` ids per row (append = None, so the history keeps its
          length): microseconds per launch from a pair of device events around `iters` back-to-back launches, median of `repeats` windows after a warm-up window.
          The torch route on the same inputs is timed by the host clock around `iters / 10` synchronised calls (it synchronises by itself: NoRepeatNGram reads the
          history on the host).
  decode: ms per decoded token at Llama-7B size (random weights, 64-token prompt), modes ALTERNATING in one process: greedy (no control), kernel (the four controls
          through llmseg_logits_process), torch (the four controls through the torch route, swapped in for ops.logits_process);
          (a call generating NEW tokens - a call generating 2) / (NEW - 2), so prefill and LoRA merge cancel; median (min .. max) of `repeats` pairs per mode.
          Every mode runs the eos rule with an eos id the greedy run never emits (the controlled modes ban it throughout: min_new_tokens = max_new_tokens), so every
          call generates exactly the tokens asked for and every mode has the loop's one host synchronisation per token.
usage: python tools/generation_controls_bench.py kernel [N list=1,8] [hist list=100,600] [iters=2000] [repeats=7] [json out] [V=32003]
       python tools/generation_controls_bench.py decode [modes=greedy,kernel,torch] [N list=1,8] [new_tokens=66] [repeats=7] [json out]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "kernel"
assert MODE in ("kernel", "decode"), __doc__
assert torch.cuda.is_available(), "generation_controls_bench needs a GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
rows = []
THETA, G = 1.2, 3

try:
    import transformers as tf
    TORCH_ROUTE = "transformers " + tf.__version__
except ImportError:
    tf = None
    TORCH_ROUTE = "restated rule (CPU)"


class TorchRoute:
    """a stand-in for ops.logits_process with its signature: the same processors through torch.  It keeps `input_ids` itself, as HF's loop does (one torch.cat per
    token); ids outside the vocabulary (the <image> placeholder) are clamped into it once, at the first call: HF's gather cannot take them."""

    def __init__(self, prompt_len, min_new, eos, suppress):
        self.ids = None
        if tf is not None:
            self.procs = [tf.RepetitionPenaltyLogitsProcessor(penalty=THETA), tf.NoRepeatNGramLogitsProcessor(G)]
            if eos is not None:
                self.procs.append(tf.MinNewTokensLengthLogitsProcessor(prompt_len, min_new, eos, device=dev))
            self.procs.append(tf.SuppressTokensLogitsProcessor(suppress, device=dev))
        self.eos, self.suppress = eos, suppress

    def __call__(self, logits, hist, hist_len, append=None, repetition_penalty=1.0, no_repeat_ngram_size=0, ban_token=None, suppress=None):
        if append is None:
            self.ids = hist[:, :int(hist_len[0])].clamp(0, logits.shape[1] - 1)
        else:
            self.ids = torch.cat([self.ids, append[:, None]], 1)
        return self.process(logits, ban_token)

    def process(self, logits, ban_token):
        if tf is not None:
            for p in self.procs:
                logits = p(self.ids, logits)
            return logits
        from tests import logits_process_checks as lc
        return lc.rule_rows(logits.cpu(), self.ids.tolist(), theta=THETA, g=G, ban=ban_token, suppress=self.suppress).to(dev)


if MODE == "kernel":
    from llmseg_amd import ops
    NS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,8").split(",")]
    HS = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "100,600").split(",")]
    ITERS = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    REP = int(sys.argv[5]) if len(sys.argv) > 5 else 7
    OUT = sys.argv[6] if len(sys.argv) > 6 else None
    V = int(sys.argv[7]) if len(sys.argv) > 7 else 32003
    BAN, SUP = 2, [11, 29871]
    for N in NS:
        for H in HS:
            g = torch.Generator().manual_seed(N * 1000 + H)
            logits0 = (3.0 * torch.randn(N, V, generator=g)).to(dev, torch.bfloat16)
            logits = logits0.clone()
            hist = torch.zeros((N, ops.LOGITS_HIST_CAP), dtype=torch.int64)
            hist[:, :H] = torch.randint(0, V, (N, H), generator=g)
            hist[:, H // 2:H // 2 + 20] = hist[:, :20]                      # a repeated stretch: the n-gram ban finds matches
            hist = hist.to(dev)
            hist_len = torch.full((N,), H, dtype=torch.int32, device=dev)
            sup = torch.tensor(SUP, dtype=torch.int32, device=dev)

            def window():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(ITERS):
                    ops.logits_process(logits, hist, hist_len, repetition_penalty=THETA, no_repeat_ngram_size=G, ban_token=BAN, suppress=sup)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / ITERS * 1e3
            window()
            us = [window() for _ in range(REP)]
            route = TorchRoute(H, H + 1, BAN, SUP)                          # min_new_tokens beyond the history: the eos is banned, as in the kernel call
            route(logits0, hist, hist_len, ban_token=BAN)                  # takes the history once; the windows time the processors alone

            def torch_window():
                n = max(ITERS // 10, 10)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    route.process(logits0, BAN)
                    torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n * 1e6
            torch_window()
            tus = [torch_window() for _ in range(REP)]
            rows.append(dict(mode="kernel", N=N, V=V, hist=H, us_per_launch=statistics.median(us), us_min=min(us), us_max=max(us), iters=ITERS, repeats=REP,
                             torch_route=TORCH_ROUTE, torch_us_per_call=statistics.median(tus), torch_us_min=min(tus), torch_us_max=max(tus)))
            print(f"kernel N={N} V={V} hist={H}: {statistics.median(us):.2f} us per launch ({min(us):.2f} .. {max(us):.2f}, {REP} windows of {ITERS}); "
                  f"torch route ({TORCH_ROUTE}): {statistics.median(tus):.1f} us per synchronised call ({min(tus):.1f} .. {max(tus):.1f})", flush=True)
else:
    from llmseg_amd import ops
    from llmseg_amd.lisa import LISAForCausalLM
    from llmseg_amd.params import LisaConfig, LlamaConfig
    MODES = (sys.argv[2] if len(sys.argv) > 2 else "greedy,kernel,torch").split(",")
    NS = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,8").split(",")]
    NEW = int(sys.argv[4]) if len(sys.argv) > 4 else 66
    REP = int(sys.argv[5]) if len(sys.argv) > 5 else 7
    OUT = sys.argv[6] if len(sys.argv) > 6 else None
    assert set(MODES) <= {"greedy", "kernel", "torch"} and NEW > 2 and REP >= 1
    cfg = LisaConfig(backbone="sam", build_unused_towers=False)
    cfg.llama = LlamaConfig(lora_r=8)
    m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
    m.prepare()
    SUP = [11, 29871]
    REAL = ops.logits_process

    def timed(clip, ids, new, mode, eos):
        kw = dict(max_new_tokens=new, eos_token_id=eos)
        if mode != "greedy":
            kw.update(repetition_penalty=THETA, no_repeat_ngram_size=G, min_new_tokens=new, suppress_tokens=SUP)
        ops.logits_process = TorchRoute(ids.shape[1], new, eos, SUP) if mode == "torch" else REAL
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seq, _ = m.generate(clip, ids, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            ops.logits_process = REAL
        assert seq.shape[1] == ids.shape[1] + new, "a call stopped early: the differencing needs calls of the full length"
        return dt, seq

    for N in NS:
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(3, 31999, (N, 64), generator=g)
        ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
        clip = torch.randn(N, 3, 224, 224, generator=g).to(dev, torch.bfloat16)
        free, _ = m.generate(clip, ids, max_new_tokens=NEW, eos_token_id=None)
        emitted = set(free[:, 64:].flatten().tolist())
        eos = next(t for t in range(3, 32000) if t not in emitted and t not in SUP)      # never emitted by the greedy run
        outs = {}
        for mode in MODES:                                                 # warm-up: allocations, code objects, the step's graph
            timed(clip, ids, 2, mode, eos)
            outs[mode] = timed(clip, ids, NEW, mode, eos)[1]
        if "kernel" in outs and "torch" in outs and tf is not None:        # the two routes compute one rule (the <image> id aside, which no row can emit)
            print(f"decode N={N}: kernel and torch routes emit {'the same' if torch.equal(outs['kernel'], outs['torch']) else 'DIFFERENT'} tokens", flush=True)
        per = {mode: [] for mode in MODES}
        for _ in range(REP):
            for mode in MODES:                                             # alternating: drift of the box hits every mode alike
                ta = timed(clip, ids, 2, mode, eos)[0]
                tb = timed(clip, ids, NEW, mode, eos)[0]
                per[mode].append((tb - ta) / (NEW - 2) * 1e3)
        for mode in MODES:
            x = per[mode]
            rows.append(dict(mode=mode, N=N, ms_per_token=statistics.median(x), ms_min=min(x), ms_max=max(x), repeats=REP, new_tokens=NEW,
                             torch_route=TORCH_ROUTE if mode == "torch" else None))
            print(f"decode N={N} {mode}: {statistics.median(x):.3f} ms/token ({min(x):.3f} .. {max(x):.3f}, {REP} pairs)", flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1)
