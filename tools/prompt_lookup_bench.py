"""ms per EMITTED token of generate(prompt_lookup_num_tokens=k) beside the plain greedy route at Llama-7B size, random weights, 64-token prompt, one session.

A call emits NEW tokens; ms per token = (time of a call emitting NEW - time of a call emitting 2) / (NEW - 2): the prefill, the LoRA merge and the weight quantisation
cancel.  The plain route and the mode ALTERNATE call by call; median of `repeats` rounds after a warm-up round (min .. max beside it).
Acceptance is forced with `_lookup_forced`: the drafts are the mode's own continuation (found by iterating from the plain route's output until a call reproduces its
drafts) with none / every second / all of them right; the rate that a row then really saw -- accepted drafts / drafted, and tokens per step -- is read from
`_lookup_trace` in an untimed call and printed beside the time.  "unforced" is the history lookup itself on a prompt that repeats an 8-token pattern (random weights
do not continue a pattern: the figure is what a wasted draft costs, and the trace says how few were accepted).

cases: n1 = one sequence, k in `ks`; n8 = 8 sequences at k = 3.  weights: 16 = bf16, mxfp4.
mode "trace": one warmed call per k at one sequence and nothing else, to be run under a kernel trace (the draft and accept launches are lookup_draft_kernel,
lookup_argmax_kernel and lookup_accept_kernel).

usage: python tools/prompt_lookup_bench.py [cases=n1,n8] [weights=16,mxfp4] [ks=1,3,7] [new_tokens=34] [repeats=3] [lora_r=8] [json out | "trace"]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

assert torch.cuda.is_available(), "prompt_lookup_bench needs a GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")


def main():
    from llmseg_amd.lisa import LISAForCausalLM
    from llmseg_amd.params import LisaConfig, LlamaConfig
    arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
    cases, weights, ks = arg(1, "n1,n8").split(","), arg(2, "16,mxfp4").split(","), [int(x) for x in arg(3, "1,3,7").split(",")]
    NEW, REP, R, out = int(arg(4, "34")), int(arg(5, "3")), int(arg(6, "8")), arg(7, None)
    assert set(cases) <= {"n1", "n8"} and set(weights) <= {"16", "mxfp4"} and NEW > 2 and REP >= 1
    cfg = LisaConfig(backbone="sam", build_unused_towers=False)
    cfg.llama = LlamaConfig(lora_r=R)
    m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
    m.prepare()
    V = cfg.llama.vocab

    def timed(clip, ids, new, kw):
        if "_lookup_forced" in kw:                                             # the hook takes [N, max_new_tokens]
            kw = dict(kw, _lookup_forced=kw["_lookup_forced"][:, :new].contiguous())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = m.generate(clip, ids, max_new_tokens=new, eos_token_id=None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def prompts(N, repeating=False):
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(3, 31999, (N, 64), generator=g)
        if repeating:
            ids[:, 4:] = ids[:, 4:12].repeat(1, 8)[:, :60]
        ids[:, 0] = 1; ids[:, 1] = 32001; ids[:, 2] = -200; ids[:, 3] = 32002
        return ids, torch.randn(N, 3, 224, 224, generator=g).to(dev, torch.bfloat16)

    def own_continuation(clip, ids, base, k):
        """forced drafts that the mode itself confirms: start from the plain route's tokens and iterate"""
        _, (seq, _) = timed(clip, ids, NEW, base)
        cont = seq[:, ids.shape[1]:].clone()
        for _ in range(4):
            _, (seq, _) = timed(clip, ids, NEW, dict(base, prompt_lookup_num_tokens=k, _lookup_forced=cont))
            nxt = seq[:, ids.shape[1]:]
            if torch.equal(nxt, cont):
                break
            cont = nxt.clone()
        return cont

    def forced(cont, kind):
        wrong = (cont + 1) % V
        return {"acc0": wrong, "acc50": torch.where(torch.arange(cont.shape[1], device=cont.device)[None, :] % 2 == 0, cont, wrong), "acc100": cont}[kind]

    rows = []
    if out == "trace":
        ids, clip = prompts(1)
        for k in ks:
            for _ in range(3):
                timed(clip, ids, NEW, dict(prompt_lookup_num_tokens=k))
        return
    for case in cases:
        N = 1 if case == "n1" else 8
        for w in weights:
            if case == "n8" and w != "16":
                continue
            base = {} if w == "16" else {"weight_format": w}
            for k in (ks if case == "n1" else [3]):
                ids, clip = prompts(N)
                cont = own_continuation(clip, ids, base, k)
                rid, rclip = prompts(N, repeating=True)
                runs = {"plain": (clip, ids, base)}
                for kind in ("acc0", "acc50", "acc100"):
                    runs[kind] = (clip, ids, dict(base, prompt_lookup_num_tokens=k, _lookup_forced=forced(cont, kind)))
                runs["unforced_repeating_prompt"] = (rclip, rid, dict(base, prompt_lookup_num_tokens=k))
                runs["plain_repeating_prompt"] = (rclip, rid, base)
                seen = {}
                for name, (c_, i_, kw) in runs.items():                        # warm-up (states, graphs), and the acceptance each run really sees
                    timed(c_, i_, 2, kw)
                    if "prompt_lookup_num_tokens" in kw:
                        tr = []
                        timed(c_, i_, NEW, dict(kw, _lookup_trace=tr))
                        drafted, accepted = sum(sum(t["draft_len"]) for t in tr), sum(sum(t["accepted"]) for t in tr)
                        seen[name] = dict(steps=len(tr), drafted=drafted, accepted=accepted, accept_rate=accepted / max(drafted, 1), tokens_per_row_step=(NEW - 1) / max(len(tr), 1))
                    timed(c_, i_, NEW, kw)
                per = {name: [] for name in runs}
                for _ in range(REP):
                    for name, (c_, i_, kw) in runs.items():                    # alternating: every run once per round
                        ta, _ = timed(c_, i_, 2, kw)
                        tb, _ = timed(c_, i_, NEW, kw)
                        per[name].append((tb - ta) / (NEW - 2) * 1e3)
                row = dict(case=case, sequences=N, weights=w, k=k, new_tokens=NEW, repeats=REP, lora_r=R)
                for name in runs:
                    row[name] = dict(ms_per_token=statistics.median(per[name]), ms_min=min(per[name]), ms_max=max(per[name]), **seen.get(name, {}))
                rows.append(row)
                print(f"{case} weights={w} k={k}: " + "; ".join(
                    f"{name} {v['ms_per_token']:.3f} ms/token ({v['ms_min']:.3f} .. {v['ms_max']:.3f})" +
                    (f" [accepted {v['accepted']}/{v['drafted']} = {v['accept_rate']:.2f}, {v['steps']} steps, {v['tokens_per_row_step']:.2f} tokens/step]" if "steps" in v else "")
                    for name, v in ((n, row[n]) for n in runs)), flush=True)
                if out:
                    with open(out, "w") as f:
                        json.dump(rows, f, indent=1)
            m.__dict__.pop("_decode_states", None)                              # the next weight mode starts from an empty pool of states
            torch.cuda.empty_cache()


main()
