"""Generation half of `LISAForCausalLM.evaluate` (reference `model/LISA.py:477-521`; `prepare_inputs_for_generation`,
`model/llava/model/language_model/llava_llama.py:137-163`): greedy decoding with a KV cache, the hidden state of every fed token,
and the `[SEG]` embeddings `text_hidden_fcs` makes of them.

MI355X-first shape of the loop:
  * prefill = the path's own batched forward (`TrainableMixin._llama` with the no-grad kernels), which leaves RoPE-rotated K and V of
    every layer in its packed q|k|v buffer; they are copied once into the cache [layer][N, Tmax, H] (bf16, 0.5 MB per token and sequence
    at Llama-7B: 288 GB of HBM hold any batch the path sees);
  * a decode step feeds ONE token per sequence: RMSNorm -> q|k|v GEMM (+LoRA) on N rows -> RoPE at the step's position -> K, V rows
    appended to the cache -> attention of the single query over the cache (`llmseg_attn_fwd`, Nq = 1, strided K / V) -> o_proj -> MLP.
    At N <= 8 rows every GEMM is a weight stream (13.5 GB per token): HBM-bound, not MFMA-bound;
  * prompts of different lengths share a batch (`attention_mask`, right padding): the prefill masks the padding as training does, and every decode
    step runs each sequence at its own device-side position (RoPE angle, cache slot, key count: `llmseg_decode_attn_rows`);
  * the reference generates WITHOUT a cache in its shipped configuration (`use_cache = False`) and reads the hidden states of its last
    forward; the cache yields the same tensor step by step (oracle/generate.py explains the equivalence and pins it).
HF greedy-search rules restated from `transformers==4.29.0 generation/utils.py::greedy_search` (third party): finished rows emit
`pad_token_id`, a row finishes on `eos_token_id`, the loop stops when all rows are finished or `max_new_tokens` tokens were added.
"""
import math
import types

import torch

from . import ops
from .trainable import IMAGE_TOKEN_INDEX, _Direct

BF16 = torch.bfloat16

# generate()'s quantised weight modes (weight_bits=8, weight_format="mxfp4").  Per mode: the name its persistent buffers and events are kept under; shape and
# dtype of the (packed rows, scales) of a matrix [N, K]; the `ops` quantiser, called with its own keyword names on the buffers (packed, scale, w_hat); the `ops`
# GEMM.  (`ops` is looked up at the call, so a wrapped `ops` is seen.)
QUANT_MODES = {
    8: dict(name="w8", buffers=lambda N, K: (((N, K), torch.int8), ((N,), torch.float32)),
            quantize=lambda w, b: ops.quantize_rows_i8(w, q=b[0], scale=b[1], w_hat=b[2]),
            gemm=lambda a, q, scale, **kw: ops.gemm_w8(a, q, scale, **kw)),
    "mxfp4": dict(name="mxfp4", buffers=lambda N, K: (((N, K // 2), torch.uint8), ((N, K // 32), torch.uint8)),
                  quantize=lambda w, b: ops.quantize_rows_mxfp4(w, packed=b[0], scale=b[1], w_hat=b[2]),
                  gemm=lambda a, packed, scale, **kw: ops.gemm_mxfp4(a, packed, scale, **kw)),
}
QUANT_MATRICES = ("qkv", "self_attn.o_proj.weight", "gate_up", "mlp.down_proj.weight")      # the quantised matrices of a layer, under "model.layers.{i}."


def pad_prompts(prompts, pad_token_id=0):
    """Prompts of different lengths (1-D id tensors, one <image> token each) -> (input_ids int64 [N, L], attention_mask bool [N, L]) for
    `generate(..., attention_mask=)`: right padding with `pad_token_id` (0 if None), L = the longest prompt."""
    assert len(prompts) > 0 and all(t.dim() == 1 and t.numel() > 0 for t in prompts)
    L = max(int(t.numel()) for t in prompts)
    ids = torch.full((len(prompts), L), 0 if pad_token_id is None else int(pad_token_id), dtype=torch.int64, device=prompts[0].device)
    mask = torch.zeros((len(prompts), L), dtype=torch.bool, device=prompts[0].device)
    for i, t in enumerate(prompts):
        ids[i, :t.numel()] = t
        mask[i, :t.numel()] = True
    return ids, mask


def _weight_mode(weight_bits, weight_format, fuse_decode):
    """generate()'s weight arguments, checked -> the weight mode None | 8 | "mxfp4": what the prefill and the decode state are keyed by."""
    if weight_bits not in (None, 8):
        raise ValueError(f"weight_bits must be None (bf16 weights) or 8 (int8 rows with per-row scales), got {weight_bits!r}")
    if weight_bits == 8 and not fuse_decode:
        raise ValueError("weight_bits=8 needs fuse_decode=True: the LoRA deltas are merged into q|k|v before quantisation")
    if weight_format not in (None, "mxfp4"):
        raise ValueError(f"weight_format must be None or 'mxfp4' (E2M1 elements with one E8M0 scale per 32), got {weight_format!r}")
    if weight_format is None:
        return weight_bits
    if weight_bits is not None:
        raise ValueError("weight_format='mxfp4' and weight_bits=8 are two quantised modes: pass one of them")
    if not fuse_decode:
        raise ValueError("weight_format='mxfp4' needs fuse_decode=True: the LoRA deltas are merged into q|k|v before quantisation")
    return weight_format


def _check_kv(model, kv_format, kv_cache, fuse_decode):
    """generate()'s KV-cache arguments, checked -> what the decode state is keyed by on top of today's key: () for the bf16 cache, else ("kv", kv_format, kv_cache)."""
    if kv_format not in (None, "mxfp8"):
        raise ValueError(f"kv_format must be None (a bf16 KV cache) or 'mxfp8' (E4M3 elements with one E8M0 scale per 32), got {kv_format!r}")
    if kv_cache not in ("packed", "bf16"):
        raise ValueError(f"kv_cache must be 'packed' or 'bf16', got {kv_cache!r}")
    if kv_format is None:
        if kv_cache != "packed":
            raise ValueError("kv_cache='bf16' needs kv_format: it is the yardstick of a quantised cache (the same values held in bf16)")
        return ()
    if not fuse_decode:
        raise ValueError(f"kv_format={kv_format!r} needs fuse_decode=True (the packed cache is built into the fused decode step only)")
    c = model.config.llama
    if c.head_dim != 128:
        raise ValueError(f"kv_format={kv_format!r} needs head_dim 128, got {c.head_dim}: the two-launch route is out of scope")
    if c.hidden % 32:
        raise ValueError(f"kv_format={kv_format!r} needs hidden % 32 == 0 (one scale per 32 elements), got hidden = {c.hidden}")
    return ("kv", kv_format, kv_cache)


def _check_controls(model, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, eos_token_id, max_new_tokens, num_beams):
    """generate()'s logits controls, checked -> None with all four at their defaults (no logits-processor launch), else the four by name, suppress_tokens as a list."""
    if repetition_penalty == 1.0 and no_repeat_ngram_size == 0 and min_new_tokens == 0 and suppress_tokens is None:
        return None
    if isinstance(repetition_penalty, bool) or not (isinstance(repetition_penalty, (int, float)) and math.isfinite(repetition_penalty) and repetition_penalty > 0):
        raise ValueError(f"repetition_penalty must be a finite number > 0 (1 = off), got {repetition_penalty!r}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if not (isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 2 ** 31):
            raise ValueError(f"{name} must be an integer >= 0 (0 = off), got {v!r}")
    if min_new_tokens > 0 and eos_token_id is None:
        raise ValueError("min_new_tokens needs an eos_token_id: it bans that token until enough tokens were emitted")
    if min_new_tokens > max_new_tokens:
        raise ValueError(f"min_new_tokens = {min_new_tokens} exceeds max_new_tokens = {max_new_tokens}")
    if suppress_tokens is not None:
        vocab = model.config.llama.vocab
        try:
            suppress_tokens = list(suppress_tokens)
        except TypeError:
            raise ValueError(f"suppress_tokens must be a sequence of integers in [0, {vocab}), got {suppress_tokens!r}") from None
        if not suppress_tokens or not all(isinstance(t, int) and not isinstance(t, bool) and 0 <= t < vocab for t in suppress_tokens):
            raise ValueError(f"suppress_tokens must be a non-empty sequence of integers in [0, vocab = {vocab}), got {suppress_tokens!r}")
    if isinstance(num_beams, int) and num_beams >= 2:
        raise ValueError("repetition_penalty, no_repeat_ngram_size, min_new_tokens and suppress_tokens with num_beams >= 2 are out of scope: beam search applies "
                         "processors to the log-softmax, another rule")
    return dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens)


def _check_beams(model, num_beams, length_penalty, early_stopping, return_beam_scores, beam_cache, trace, do_sample, fuse_decode):
    """generate()'s beam arguments, checked: num_beams == 1 takes none of the others; what num_beams >= 2 does not go with is refused here."""
    if not (isinstance(num_beams, int) and not isinstance(num_beams, bool) and num_beams >= 1):
        raise ValueError(f"num_beams must be an integer >= 1, got {num_beams!r}")
    if beam_cache not in ("indirect", "copy"):
        raise ValueError(f"beam_cache must be 'indirect' or 'copy', got {beam_cache!r}")
    if not isinstance(early_stopping, bool):
        raise ValueError(f"early_stopping must be True or False ('never' is out of scope), got {early_stopping!r}")
    if isinstance(length_penalty, bool) or not (isinstance(length_penalty, (int, float)) and math.isfinite(length_penalty)):
        raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}")
    if num_beams == 1 and not (length_penalty == 1.0 and early_stopping is False and not return_beam_scores and beam_cache == "indirect" and trace is None):
        raise ValueError("length_penalty, early_stopping, return_beam_scores and beam_cache need num_beams >= 2")
    if num_beams >= 2:
        if do_sample:
            raise ValueError("do_sample with num_beams >= 2 (beam sampling) is out of scope")
        if not fuse_decode:
            raise ValueError("num_beams >= 2 needs fuse_decode=True (the beam-indexed cache is built into the fused decode step only)")
        if model.config.llama.head_dim != 128:
            raise ValueError(f"num_beams >= 2 needs head_dim 128, got {model.config.llama.head_dim}: the two-launch route is out of scope")
        if num_beams > 16 or 2 * num_beams > model.config.llama.vocab:
            raise ValueError(f"num_beams must be <= 16 and 2 * num_beams <= vocab = {model.config.llama.vocab}, got {num_beams}")


def _check_sampling(do_sample, temperature, top_k, top_p, seed, uniforms, return_logprobs, input_ids, max_new_tokens):
    """generate()'s sampling arguments, checked -> None for the arg-max (which takes none of them), else the arguments by name."""
    if not do_sample:
        if not (temperature == 1.0 and top_k == 0 and top_p == 1.0 and seed is None and uniforms is None and not return_logprobs):
            raise ValueError("temperature, top_k, top_p, seed, uniforms and return_logprobs need do_sample=True (greedy decoding takes none of them)")
        return None
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    if not (isinstance(top_k, int) and not isinstance(top_k, bool) and 0 <= top_k < 2 ** 31):
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k!r}")
    if not (isinstance(top_p, (int, float)) and 0 < top_p <= 1):
        raise ValueError(f"top_p must be in (0, 1] (1 = off), got {top_p!r}")
    if seed is not None and uniforms is not None:
        raise ValueError("pass seed= or uniforms=, not both")
    if uniforms is not None and (not torch.is_tensor(uniforms) or uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (input_ids.shape[0], max_new_tokens)):
        raise ValueError(f"uniforms must be an fp32 tensor [N, max_new_tokens] = {(input_ids.shape[0], max_new_tokens)}, got "
                         f"{getattr(uniforms, 'dtype', type(uniforms))} {tuple(getattr(uniforms, 'shape', ()))}")
    return dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, uniforms=uniforms, return_logprobs=return_logprobs)


def _check_lookup(model, prompt_lookup_num_tokens, max_matching_ngram_size, forced, trace, input_ids, max_new_tokens, do_sample, num_beams, controls, kv, fuse_decode):
    """generate()'s prompt-lookup arguments, checked -> None when the mode is off (it takes none of the others), else (k, max_matching_ngram_size)."""
    k, g = prompt_lookup_num_tokens, max_matching_ngram_size
    if not (isinstance(g, int) and not isinstance(g, bool) and g >= 1):
        raise ValueError(f"max_matching_ngram_size must be an integer >= 1, got {g!r}")
    if k is None:
        if g != 2 or forced is not None or trace is not None:
            raise ValueError("max_matching_ngram_size needs prompt_lookup_num_tokens (the mode is off without it)")
        return None
    if not (isinstance(k, int) and not isinstance(k, bool) and 1 <= k < ops.DECODE_CHUNK_MAX):
        raise ValueError(f"prompt_lookup_num_tokens must be None (off) or an integer in [1, {ops.DECODE_CHUNK_MAX - 1}] (k + 1 <= {ops.DECODE_CHUNK_MAX} rows a step keep one "
                         f"sequence on the skinny GEMM), got {k!r}")
    if do_sample:
        raise ValueError("prompt_lookup_num_tokens with do_sample is out of scope: verifying drafts against a sampled token is speculative sampling, another accept rule")
    if isinstance(num_beams, int) and num_beams >= 2:
        raise ValueError("prompt_lookup_num_tokens with num_beams >= 2 is out of scope: a draft belongs to one hypothesis, the beams re-order every step")
    if controls is not None:
        raise ValueError("prompt_lookup_num_tokens with repetition_penalty, no_repeat_ngram_size, min_new_tokens or suppress_tokens is out of scope: the processors "
                         "would have to rewrite the logits of every drafted position under its own history")
    if kv:
        raise ValueError("prompt_lookup_num_tokens with kv_format is out of scope: the MXFP8 cache would need a further instance of the chunk attention kernel")
    if not fuse_decode:
        raise ValueError("prompt_lookup_num_tokens needs fuse_decode=True (the chunk attention step is built into the fused decode step only)")
    if model.config.llama.head_dim != 128:
        raise ValueError(f"prompt_lookup_num_tokens needs head_dim 128, got {model.config.llama.head_dim}: the two-launch route is out of scope")
    if forced is not None and (not torch.is_tensor(forced) or forced.dtype != torch.int64 or tuple(forced.shape) != (input_ids.shape[0], max_new_tokens)):
        raise ValueError(f"_lookup_forced must be an int64 tensor [N, max_new_tokens] = {(input_ids.shape[0], max_new_tokens)}")
    return k, g


def _row_prompts(model, input_ids, attention_mask, fuse_decode, fill, controls, max_new_tokens):
    """The row loop's prompts, checked where the trimmed mask is known -> (input_ids, attention_mask, lens): trimmed to the longest prompt, the padding set to `fill`,
    lens = the prompt lengths L_i on the host; (input_ids, None, None) on the uniform route."""
    lens = None
    if attention_mask is not None:
        input_ids, attention_mask, lens = model._ragged_prompts(input_ids, attention_mask)
    if lens is not None:
        if not fuse_decode:
            raise ValueError("prompts of different lengths need fuse_decode=True (the per-row positions are built into the fused decode step only)")
        if model.config.llama.head_dim != 128:
            raise ValueError(f"prompts of different lengths need head_dim 128, got {model.config.llama.head_dim}: per-row key counts for the two-launch "
                             "route (llmseg_rope_kv_append + llmseg_attn_fwd) are out of scope")
        input_ids = torch.where(attention_mask.to(input_ids.device), input_ids, torch.full_like(input_ids, fill))
    if controls is not None and input_ids.shape[1] + max_new_tokens > ops.LOGITS_HIST_CAP:
        raise ValueError(f"repetition_penalty, no_repeat_ngram_size, min_new_tokens and suppress_tokens keep a history of prompt + max_new_tokens = "
                         f"{input_ids.shape[1]} + {max_new_tokens} ids per row: more than the cap of {ops.LOGITS_HIST_CAP}")
    return input_ids, attention_mask, lens


def _make_pick(ids, lens, max_new_tokens, eos_token_id, pad_token_id, sampling, controls):
    """The row loop's pick, decided once per call from the checked arguments -> (pick, live): pick(logits [N, V], step) = the next token of every row (int64 [N]) by the arg-max,
    or by `ops.sample_tokens` (`sampling`), after the `ops.logits_process` launch if there are `controls`; a finished row emits pad_token_id.  live.unfinished (int64 [N]) is 0
    for the finished rows; live.logprobs holds what `ops.sample_tokens` returned at every step; live.last is the token the history has yet to take in."""
    dev, (N, L) = ids.device, ids.shape
    live = types.SimpleNamespace(unfinished=torch.ones((N,), dtype=torch.int64, device=dev), logprobs=[], last=None)
    if sampling is None:
        def pick(logits, step):
            nxt = logits.float().argmax(-1)
            if eos_token_id is not None:
                nxt = nxt * live.unfinished + pad_token_id * (1 - live.unfinished)
                live.unfinished = live.unfinished * (nxt != eos_token_id).long()
            return nxt
    else:
        uniforms = sampling["uniforms"]
        if uniforms is None:
            gen = None if sampling["seed"] is None else torch.Generator(device=dev).manual_seed(int(sampling["seed"]))
            uniforms = torch.rand((N, max_new_tokens), device=dev, dtype=torch.float32, generator=gen)
        u_steps = uniforms.to(dev).t().contiguous()            # [max_new_tokens, N]: step s reads one contiguous row

        def pick(logits, step):                                # one launch: the pick, pad for finished rows and the update of `unfinished`
            nxt, lp, _, _ = ops.sample_tokens(logits, sampling["temperature"], sampling["top_k"], sampling["top_p"], u_steps[step], eos_token_id=eos_token_id,
                                              pad_token_id=pad_token_id, unfinished=live.unfinished, want_logprob=sampling["return_logprobs"])
            live.logprobs.append(lp)
            return nxt
    if controls is None:
        return pick, live
    hist = torch.zeros((N, L + max_new_tokens), dtype=torch.int64, device=dev)      # each row's history at a fixed address: its own prompt, left-aligned
    hist[:, :L] = ids
    hist_len = (torch.full((N,), L, dtype=torch.int32) if lens is None else lens.to(torch.int32)).to(dev)
    suppress = None if controls["suppress_tokens"] is None else torch.tensor(controls["suppress_tokens"], dtype=torch.int32, device=dev)

    def processed_pick(logits, step):                          # one launch: the token just picked joins the history, then the processors rewrite the step's logits in place
        logits = ops.logits_process(logits, hist, hist_len, append=live.last, repetition_penalty=controls["repetition_penalty"], suppress=suppress,
                                    no_repeat_ngram_size=controls["no_repeat_ngram_size"], ban_token=eos_token_id if step < controls["min_new_tokens"] else None)
        live.last = pick(logits, step)
        return live.last
    return processed_pick, live


def _uniform_rows(st, hidden_p, lm_w, max_new_tokens):
    """The row loop's layout when every prompt has the same length -> (the first logits, store(st.hidden, n_new), pack(seqs, n_new) -> (sequences, hidden)): one position for
    all rows (st.pos), one column of `hidden` per step."""
    N, T, H = hidden_p.shape
    st.pos.copy_(torch.tensor([T, T + 1], dtype=torch.int32))
    hidden = torch.empty((N, T + max_new_tokens - 1, H), device=hidden_p.device, dtype=BF16)
    hidden[:, :T] = hidden_p

    def store(h, n_new):
        hidden[:, T + n_new - 1] = h
    return ops.gemm(hidden_p[:, -1].contiguous(), lm_w), store, lambda seqs, n_new: (torch.cat(seqs, 1), hidden[:, :T + n_new - 1])      # only the last position's logits are needed


def _ragged_rows(st, hidden_p, lm_w, max_new_tokens, lens, Pn, fill):
    """The same three when the prompts differ in length (lens [N], on the host): a position per row (st.pos_rows), both results packed per row, left-aligned."""
    N, T, H = hidden_p.shape
    dev = hidden_p.device
    t_rows = (lens - 1 + Pn).to(dev)                           # T_i: row i's prefill length = the position of its first fed token
    st.pos_rows.copy_(t_rows.to(torch.int32))
    hidden = torch.zeros((N, T + max_new_tokens - 1, H), device=dev, dtype=BF16)
    own = torch.arange(T, device=dev)[None, :] < t_rows[:, None]
    hidden[:, :T] = torch.where(own[:, :, None], hidden_p, torch.zeros_like(hidden_p))
    last = torch.arange(N, device=dev) * T + t_rows - 1                                # each row's own last prompt position
    logits = ops.gemm(ops.gather_rows(hidden_p.reshape(N * T, H), last), lm_w)
    slot = torch.arange(N, device=dev) * hidden.shape[1] + t_rows - 1                    # flat row of `hidden` that holds each sequence's newest state

    def pack(seqs, n_new):                                     # row i: prompt, new tokens, fill
        out = torch.cat([seqs[0], torch.full((N, n_new), fill, dtype=torch.int64, device=dev)], 1)
        out.scatter_(1, lens.to(dev)[:, None] + torch.arange(n_new, device=dev)[None, :], torch.cat(seqs[1:], 1))
        return out, hidden[:, :T + n_new - 1]
    return logits, lambda h, n_new: hidden.view(-1, H).index_copy_(0, slot.add_(1), h), pack


class BeamBook:
    """The host's book of a beam search over N prompts of B beams, in plain Python: per prompt the pool of its B best hypotheses (value, kind, step, slot), the "done"
    rule, the live beams that join at the end, and the back-trace of the winner through the parents."""

    def __init__(self, N, B, length_penalty, early_stopping, eos_token_id):
        self.N, self.B, self.lp, self.early, self.eos = N, B, length_penalty, early_stopping, eos_token_id
        self.done, self.pools = [False] * N, [[] for _ in range(N)]

    @staticmethod
    def add(pool, B, hyp):
        """Hugging Face's BeamHypotheses.add: keep the B best by value; a newcomer enters a full pool only when it beats the worst, which then leaves."""
        if len(pool) < B:
            pool.append(hyp)
        elif hyp[0] > min(h[0] for h in pool):
            worst = min(range(len(pool)), key=lambda i: pool[i][0])
            pool[worst] = hyp

    def step(self, step, step_best, fin_count, fin_parent, fin_score):
        """The record of pick `step` (lists [N], [N], [N][B], [N][B]): the eos candidates become hypotheses of step + 1 tokens, then the done rule."""
        g = step + 1
        for n in range(self.N):
            if self.done[n]:
                continue
            for k in range(fin_count[n]):
                self.add(self.pools[n], self.B, (fin_score[n][k] / g ** self.lp, "eos", step, fin_parent[n][k]))
            if len(self.pools[n]) >= self.B and (self.early or min(h[0] for h in self.pools[n]) >= step_best[n] / g ** self.lp):
                self.done[n] = True

    def finish(self, last_scores, tokens, parents):
        """last_scores [N * B] of the last pick; tokens, parents [steps][N * B] of every pick -> per prompt (the winner's tokens, its value, the flat rows
        t * N * B + n * B + slot of the steps' hidden states for every token of the winner but the last: the state of each FED token)."""
        steps, B, R = len(tokens), self.B, self.N * self.B
        winners = []
        for n in range(self.N):
            if not self.done[n]:                               # a prompt that is not done: its live beams are hypotheses of `steps` tokens
                for i in range(B):
                    self.add(self.pools[n], B, (last_scores[n * B + i] / steps ** self.lp, "live", steps - 1, i))
            value, kind, s, slot = max(self.pools[n], key=lambda h: h[0])      # (the first of equal values)
            seq, rows = ([int(self.eos)], []) if kind == "eos" else ([], [])
            for t in range(s - len(seq), -1, -1):              # from the last picked token back to the first, through the parents
                seq.append(tokens[t][n * B + slot])
                rows.append(t * R + n * B + slot)
                slot = parents[t][n * B + slot]
            winners.append((seq[::-1], value, rows[::-1][:len(seq) - 1]))
        return winners


class DecodeState:
    """Everything a decode step touches, at fixed addresses (so the step can be captured once and replayed): the KV cache
    [layers][N, capacity, H] bf16 x 2, the device-side position {pos, pos + 1} (or one position per sequence, pos_rows, when the prompts
    differ in length), the step's input embeddings and its outputs.  kv = ("kv", "mxfp8", "packed"): K and V are uint8 E4M3 codes, with their E8M0 scale bytes
    ks, vs [layers][N, capacity, H / 32]; ("kv", "mxfp8", "bf16"): the bf16 cache, which then holds x_hat (the yardstick of the packed cache).
    q > 1 (prompt lookup): a step feeds q tokens per sequence, so x, hidden and logits hold N * q step rows (row n * q + j = token j of sequence n) while the cache
    stays [N, capacity]; the step reads pos_rows and does not advance it (the accept launch does)."""

    def __init__(self, layers, N, cap, H, V, device, kv=(), q=1):
        self.kv_format, self.kv_packed = (kv[1], kv[2] == "packed") if kv else (None, False)
        self.k = torch.empty((layers, N, cap, H), device=device, dtype=torch.uint8 if self.kv_packed else BF16)
        self.v = torch.empty_like(self.k)
        self.ks = self.vs = None
        if self.kv_packed:
            self.ks = torch.empty((layers, N, cap, H // 32), device=device, dtype=torch.uint8)
            self.vs = torch.empty_like(self.ks)
        self.pos = torch.zeros((2,), device=device, dtype=torch.int32)       # [0] = position of the token being fed, [1] = keys present after it
        self.pos_rows = torch.zeros((N,), device=device, dtype=torch.int32)  # ragged prompts: position of the token being fed, per sequence
        self.q, self.rows = q, N * q                                          # tokens per sequence and step; rows of a step
        self.x = torch.empty((self.rows, H), device=device, dtype=BF16)
        self.hidden = torch.empty((self.rows, H), device=device, dtype=BF16)
        self.logits = torch.empty((self.rows, V), device=device, dtype=BF16)
        self.N, self.cap, self.H = N, cap, H
        self.graph = None
        self.warm = False            # the state's first step ran eagerly (the step is captured at its second)
        self.fused = False           # decode step on merged-LoRA weights (+ norm / SwiGLU on the GEMM's A load for a single sequence)
        self.qkv_w = None            # per-layer q|k|v weights with the LoRA deltas merged in (fused steps)
        self.bits = None             # weight mode of the captured step: None = bf16 weights, 8 = weight_bits, "mxfp4" = weight_format
        self.ragged = False          # the captured step reads pos_rows (one position per sequence) instead of pos
        self.qw = None               # quantised modes: {layer-matrix name: (packed rows, scales, w_hat bf16)} of `_quantize_decode_weights`
        self.beam_src = None         # beam search over the never-moved cache: int32 [N, capacity], key t of row r lives in physical row beam_src[r, t]
        self.src_a = self.src_b = None      # beam search: the table at a fixed address (the captured step reads it) and the buffer `ops.beam_step` re-orders it into


class GenerateMixin:
    def _merge_lora(self):
        """q|k|v weights with the LoRA deltas folded in (W + (alpha / r) B A on the q and v blocks, peft `merge_and_unload` -- what the
        reference's released checkpoints are, merge_lora_weights_and_save_hf_model.py), rebuilt from the CURRENT LoRA matrices at every
        `generate()` call into persistent buffers (3.2 GB at Llama-7B; ~2 ms): a decode step then needs no LoRA launches.  The rounding of
        W + delta to bf16 differs from the training forward's x W^T + (x A^T) B^T by one bf16 ulp of W."""
        c = self.config.llama
        F = _Direct
        H = c.hidden
        bufs = self.__dict__.setdefault("_merged_qkv", [None] * c.layers)
        s = c.lora_alpha / c.lora_r
        for i in range(c.layers):
            p = f"model.layers.{i}."
            w = self._wcat(p + "qkv", [p + f"self_attn.{n}_proj.weight" for n in "qkv"], F)
            if bufs[i] is None:
                bufs[i] = torch.empty_like(w)
            bufs[i].copy_(w)
            lp = p + "self_attn."
            for blk, n in ((0, "q_proj"), (2, "v_proj")):
                a_, b_ = self._w(lp + n + ".lora_A.default.weight", F), self._w(lp + n + ".lora_B.default.weight", F)
                r = a_.shape[0]
                if r % 8:                                     # the GEMM contracts in 16-byte chunks: pad the rank with zeros
                    rp = (r + 7) // 8 * 8
                    a_ = torch.cat([a_, torch.zeros((rp - r, H), device=a_.device, dtype=a_.dtype)], 0)
                    b_ = torch.cat([b_, torch.zeros((H, rp - r), device=b_.device, dtype=b_.dtype)], 1).contiguous()
                view = bufs[i][blk * H:(blk + 1) * H]
                ops.gemm(b_, a_, trans_w=True, alpha=s, residual=view, out=view)           # [H, r] @ [r, H] + W block
        return bufs

    def _decode_body(self, st):
        """One token per sequence through the decoder stack: st.x (embeddings of the token at position st.pos[0]) -> st.hidden, st.logits;
        K / V of the token are appended to the cache and the position advances.  No host-visible state: the step is a pure kernel
        sequence over fixed buffers, replayable from a hipGraph.  Every route is this one loop; the routes differ in how a layer's four
        matrices are applied (`_decode_linears`) and in how attention runs (`_decode_attention`).  Six launches per layer for a single
        sequence (LoRA merged): q|k|v GEMM with the input RMSNorm on its A load, RoPE + KV append + attention (+ the split's merge), o_proj
        (+ residual), gate|up GEMM with the post-attention RMSNorm on its A load, down_proj (+ residual) with SwiGLU on its A load."""
        c = self.config.llama
        F = _Direct
        N, H = st.x.shape
        lin = self._decode_linears(st)
        cos, sin, _ = self._rope(st.cap)
        x = st.x
        att = torch.empty((N, H), device=x.device, dtype=BF16)
        scratch = ops.decode_attn_scratch(st.N, c.heads, x.device) if st.fused and c.head_dim == 128 else None
        if scratch is not None and st.q > 1:                   # the same key split, partials per step row
            scratch = torch.empty((scratch.numel() * st.q,), device=x.device, dtype=torch.float32)
        for i in range(c.layers):
            qkv = lin(i, "qkv", x, norm="input_layernorm.weight")
            self._decode_attention(st, i, qkv, cos, sin, att, scratch)
            x = lin(i, "self_attn.o_proj.weight", att, residual=x)
            gu = lin(i, "gate_up", x, norm="post_attention_layernorm.weight")
            x = lin(i, "mlp.down_proj.weight", gu, swiglu=True, residual=x)
        ops.norm(x, self._w("model.norm.weight", F), None, eps=c.eps, rms=True, out=st.hidden)
        ops.gemm(st.hidden, self._w("lm_head.weight", F), out=st.logits)          # lm_head stays bf16 at weight_bits = 8 too: 2 % of the stream, and it decides the arg-max
        if st.q == 1:                                          # (q > 1: the accept launch advances pos_rows by what stands of the chunk)
            (st.pos_rows if st.ragged else st.pos).add_(1)

    def _decode_attention(self, st, i, qkv, cos, sin, att, scratch):
        """RoPE of the new token's q and k at the device-side position, its K / V appended to layer i's cache, attention of the one query over the cache -> att."""
        c = self.config.llama
        hd, heads, H = c.head_dim, c.heads, st.H
        if st.q > 1:                                           # prompt lookup: q tokens per sequence at pos_rows[n] .. pos_rows[n] + q - 1, causal among themselves
            ops.decode_attn_chunk(qkv, cos, sin, st.k[i], st.v[i], st.pos_rows, heads, hd, st.q, out=att, scratch=scratch)
            return
        if st.fused and hd == 128:                             # one launch (+ the split's merge); ragged: every sequence at its own position (RoPE angle, cache slot, key count)
            pos = st.pos_rows if st.ragged else st.pos
            if st.kv_packed:                                   # the same step on the MXFP8 cache: slot [n][pos] receives the rounding of the new k / v
                ops.decode_attn(qkv, cos, sin, st.k[i], st.v[i], pos, heads, hd, out=att, scratch=scratch, per_row=st.ragged, beam_src=st.beam_src,
                                k_scale=st.ks[i], v_scale=st.vs[i])
                return
            ops.decode_attn(qkv, cos, sin, st.k[i], st.v[i], pos, heads, hd, out=att, scratch=scratch, per_row=st.ragged, beam_src=st.beam_src)
            if st.kv_format is not None:                       # kv_cache="bf16", the yardstick: slot [n][pos_n] <- its x_hat, in place, at the position the step reads
                row0 = pos if st.ragged else pos[:1]
                ops.kv_quantize_mxfp8(st.k[i], x_hat=st.k[i], row0=row0, rows=1)
                ops.kv_quantize_mxfp8(st.v[i], x_hat=st.v[i], row0=row0, rows=1)
        else:
            ld = qkv.stride(0)
            ops.rope_kv_append_(qkv, cos, sin, st.k[i], st.v[i], st.pos, heads, hd)       # q, k rotated at the device-side position; k, v -> cache
            ops.attention(qkv, st.k[i], st.v[i], att, batch=st.N, heads=heads, Nq=1, Nk=st.cap, head_dim=hd, q_strides=(ld, hd, ld),
                          k_strides=(st.cap * H, hd, H), v_strides=(st.cap * H, hd, H), o_strides=(H, hd, H), nk_dev=st.pos[1:])

    def _decode_linears(self, st):
        """How a decode step applies a layer's four matrices (QUANT_MATRICES) on this state's route, chosen once per step:
        -> lin(i, name, a, norm=None, swiglu=False, residual=None) = f(a) @ W_name^T (+ residual) of layer i, f = the RMSNorm of weight `norm`, SwiGLU, or nothing."""
        c = self.config.llama
        F = _Direct
        H = st.H
        prefix = "model.layers.{}.".format

        def pre(p, a, norm, swiglu):                           # f as a launch of its own
            if norm is not None:
                return F.norm(a, self._w(p + norm, F), None, c.eps, True)
            return ops.swiglu(a, c.inter) if swiglu else a

        if st.bits is not None:                                # int8 or MXFP4 rows; the A-load fusions of the bf16 route for a single sequence are not built for these kernels
            gemm = QUANT_MODES[st.bits]["gemm"]

            def lin_quantised(i, name, a, norm=None, swiglu=False, residual=None):
                p = prefix(i)
                return ops.gemm_rows(gemm, pre(p, a, norm, swiglu), *st.qw[p + name][:2], residual=residual)
            return lin_quantised

        members = {"qkv": [f"self_attn.{n}_proj.weight" for n in "qkv"], "gate_up": ["mlp.gate_proj.weight", "mlp.up_proj.weight"]}

        def weight(i, p, name):                                # bf16: q|k|v with the LoRA deltas merged in where the step is fused
            if name == "qkv" and st.qkv_w is not None:
                return st.qkv_w[i]
            return self._wcat(p + name, [p + m for m in members[name]], F) if name in members else self._w(p + name, F)

        onload = st.fused and st.rows == 1   # RMSNorm / SwiGLU on the skinny GEMM's A load: every wave redoes the transform, a win for one row only (two rows: 4.02 vs
        #                                      3.90 ms per token with the norm on load, 5.97 vs 4.34 with both): more rows keep the separate launches
        if onload:
            def lin_onload(i, name, a, norm=None, swiglu=False, residual=None):
                p = prefix(i)
                return ops.gemm(a, weight(i, p, name), residual=residual, a_norm_w=None if norm is None else self._w(p + norm, F), a_norm_eps=c.eps, a_swiglu=swiglu)
            return lin_onload

        lora = not st.fused and c.lora_r > 0                   # fuse_decode=False: the LoRA deltas of q and v as launches of their own
        s = c.lora_alpha / c.lora_r if lora else 0.0

        def lin(i, name, a, norm=None, swiglu=False, residual=None):
            p = prefix(i)
            h = pre(p, a, norm, swiglu)
            out = ops.gemm(h, weight(i, p, name), residual=residual)      # skinny GEMM: a weight stream
            if lora and name == "qkv":
                lp = p + "self_attn."
                aq, bq = self._w(lp + "q_proj.lora_A.default.weight", F), self._w(lp + "q_proj.lora_B.default.weight", F)
                av, bv = self._w(lp + "v_proj.lora_A.default.weight", F), self._w(lp + "v_proj.lora_B.default.weight", F)
                if c.lora_r == 8:                              # rank-8 kernels: [h Aq^T | h Av^T] in one pass, then the two rank-8 updates
                    xa = ops.lora_down(h, aq, x2=h, w2=av)
                    ops.lora_apply_(out[:, :H], xa, bq, alpha=s)
                    ops.lora_apply_(out[:, 2 * H:], xa[:, 8:], bv, alpha=s)
                else:
                    ops.gemm(ops.gemm(h, aq), bq, residual=out[:, :H], out=out[:, :H], alpha=s)
                    ops.gemm(ops.gemm(h, av), bv, residual=out[:, 2 * H:], out=out[:, 2 * H:], alpha=s)
            return out
        return lin

    def _quantize_decode_weights(self, mode):
        """A quantised mode of QUANT_MODES: the four matrices of every layer (QUANT_MATRICES: merged q|k|v with the LoRA deltas folded in, o_proj, gate|up,
        down_proj) as packed rows and scales -- int8 rows with one fp32 scale each, or MXFP4 rows (packed E2M1 nibbles and one E8M0 scale byte per 32 columns) --
        plus W^ in bf16 for the prefill (bf16(q * scale), or the exact element * 2^e), from one quantiser launch per matrix into persistent buffers kept per
        mode (6.5 GB or 3.4 GB, + 13 GB at Llama-7B).  Rebuilt from the CURRENT weights at every call, as the merge is: weights loaded or trained in place can
        never be stale.  The cost (merge included) is timed with a pair of events per mode: `w8_prepare_ms()`, `mxfp4_prepare_ms()`."""
        c = self.config.llama
        F = _Direct
        fmt = QUANT_MODES[mode]
        ev = self.__dict__.get(f"_{fmt['name']}_events")
        if ev is None:
            ev = self.__dict__[f"_{fmt['name']}_events"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        merged = self._merge_lora() if c.lora_r > 0 else None
        bufs = self.__dict__.setdefault("_" + fmt["name"], {})
        for i in range(c.layers):
            p = f"model.layers.{i}."
            src = (merged[i] if merged is not None else self._wcat(p + "qkv", [p + f"self_attn.{n}_proj.weight" for n in "qkv"], F),
                   self._w(p + "self_attn.o_proj.weight", F),
                   self._wcat(p + "gate_up", [p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"], F),
                   self._w(p + "mlp.down_proj.weight", F))
            for name, w in zip(QUANT_MATRICES, src):
                b = bufs.get(p + name)
                if b is None:
                    (ps, pd), (ss, sd) = fmt["buffers"](*w.shape)
                    b = bufs[p + name] = (torch.empty(ps, device=w.device, dtype=pd), torch.empty(ss, device=w.device, dtype=sd), torch.empty_like(w))
                fmt["quantize"](w, b)
        ev[1].record()
        return bufs

    def _prepare_ms(self, mode):
        ev = self.__dict__[f"_{QUANT_MODES[mode]['name']}_events"]
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    def _decode_weights(self, mode):
        return {k: (b[0], b[1]) for k, b in self.__dict__["_" + QUANT_MODES[mode]["name"]].items()}

    def w8_prepare_ms(self):
        """Device time of the last `generate(weight_bits=8)` call's LoRA merge + quantisation (waits for that work to finish)."""
        return self._prepare_ms(8)

    def decode_weights_i8(self):
        """{layer-matrix name: (q int8 [N, K], scale fp32 [N])} of the last `generate(weight_bits=8)` call: names are "model.layers.{i}." +
        "qkv" (merged q|k|v), "self_attn.o_proj.weight", "gate_up" (gate|up) and "mlp.down_proj.weight"."""
        return self._decode_weights(8)

    def mxfp4_prepare_ms(self):
        """Device time of the last `generate(weight_format="mxfp4")` call's LoRA merge + quantisation (waits for that work to finish)."""
        return self._prepare_ms("mxfp4")

    def decode_weights_mxfp4(self):
        """{layer-matrix name: (packed uint8 [N, K / 2], scale uint8 [N, K / 32])} of the last `generate(weight_format="mxfp4")` call; the names are
        `decode_weights_i8`'s."""
        return self._decode_weights("mxfp4")

    def _prefill_quantised(self, embeds, key_mask_u8, qw, kv_out):
        """The prompt through the decoder stack of the QUANTISED model: the no-grad kernel sequence of `_llama` on W^ (entry [2] of every matrix: bf16(q * scale)
        of the int8 mode, the exact element * 2^e of MXFP4), so that prefill and decode steps run one model (the one a cache-free forward on the dequantised
        state dict runs).  -> final-norm hidden [N, T, H]."""
        c = self.config.llama
        F = _Direct
        N, T, H = embeds.shape
        x = embeds.reshape(N * T, H)
        rope = self._rope(T)
        for i in range(c.layers):
            p = f"model.layers.{i}."
            h = F.norm(x, self._w(p + "input_layernorm.weight", F), None, c.eps, True)
            qkv = ops.gemm(h, qw[p + "qkv"][2])
            a = F.rope_attn(qkv, rope, N, T, c.heads, c.head_dim, True, key_mask_u8)
            kv_out(i, qkv)                                     # qkv now holds the rotated K and V
            x = ops.gemm(a, qw[p + "self_attn.o_proj.weight"][2], residual=x)
            h = F.norm(x, self._w(p + "post_attention_layernorm.weight", F), None, c.eps, True)
            gu = ops.gemm(h, qw[p + "gate_up"][2])
            x = ops.gemm(ops.swiglu(gu, c.inter), qw[p + "mlp.down_proj.weight"][2], residual=x)
        return F.norm(x, self._w("model.norm.weight", F), None, c.eps, True).view(N, T, H)

    def _decode_step(self, st, use_graph=True):
        """Run one decode step; from the second step of a state on, replay it from a hipGraph (captured once per (N, capacity): a step is
        ~420 launches of 5-20 us kernels, the host cannot issue them as fast as the GPU finishes them)."""
        if not use_graph:
            return self._decode_body(st)
        if st.graph is None:
            if not st.warm:
                st.warm = True
                return self._decode_body(st)                    # first step of this state: eager (also warms every allocation)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):      # (another thread -- an RCCL watchdog -- may query events meanwhile: train.py::_capture)
                self._decode_body(st)
            st.graph = g                                        # capture records, it does not execute: fall through to the replay
        st.graph.replay()

    def _prefill(self, images_clip, input_ids, attention_mask, rows, max_new_tokens, mode, fused, key, kv=(), chunk=1):
        """What every generate() route does before its loop: the prompts (input_ids [N, L], trimmed; attention_mask = the ragged call's mask, else None) through the prefill
        in the call's weight mode (`_weight_mode`), K and V of prompt n into physical row n * rows of the decode state of N * rows rows (rows = 1, or the beams per prompt), the state made ready
        for the call's route.  The states are kept per (N * rows, capacity) + key + kv (kv = `_check_kv`'s: a quantised cache is a state of its own, and K / V go into it
        through `ops.kv_quantize_mxfp8`).  chunk = q > 1 (prompt lookup): the state's steps take q tokens per sequence, and the capacity has room for a chunk behind
        the last position.  -> (state, final-norm hidden [N, T, H], T, embedding weights, lm_head weights)."""
        self.prepare()
        c = self.config
        cl = c.llama
        dev = self.device_
        F = _Direct
        N, L = input_ids.shape
        Pn, H = c.n_img_tokens, cl.hidden
        T = L - 1 + Pn
        assert max_new_tokens >= 1
        plan = self.make_plan(input_ids, None, torch.ones((N, L), dtype=torch.bool) if attention_mask is None else attention_mask, list(range(N + 1)), None, inference=False)
        proj = self.encode_images(images_clip.to(dev, BF16))
        emb_w = self._w("model.embed_tokens.weight", F)
        embeds = F.embed_splice(input_ids.to(dev).contiguous(), emb_w, proj[1:], Pn, (Pn + 1) * H, plan.tok_index)
        cap = (T + max_new_tokens + (chunk if chunk > 1 else 0) + 63) // 64 * 64      # chunk: pos_n + q <= cap at every step (pos_n <= T + max_new_tokens - 1)
        states = self.__dict__.setdefault("_decode_states", {})
        key = key + kv
        st = states.get((N * rows, cap) + key)
        if st is None:
            st = states[(N * rows, cap) + key] = DecodeState(cl.layers, N * rows, cap, H, cl.vocab, dev, kv=kv, q=chunk)

        # ragged prompts: K and V are copied for [:, :T] of every row.  The slots at or beyond a row's own T_i = L_i - 1 + Pn then hold the padding's
        # K / V (and, past T, whatever an earlier call left): garbage that is never read, because the step that feeds a row's token at position
        # pos writes cache[pos] itself and attends to keys 0 .. pos only -- a slot is overwritten before the row's key count reaches it.
        def keep_kv(i, qkv):                                   # qkv [N*T, 3H] after the in-place RoPE of q and k
            k, v = qkv[:, H:2 * H].view(N, T, H), qkv[:, 2 * H:3 * H].view(N, T, H)
            if st.kv_format is None:
                st.k[i, ::rows, :T].copy_(k)
                st.v[i, ::rows, :T].copy_(v)
            elif st.kv_packed:                                 # through the quantiser: one launch per layer and tensor
                ops.kv_quantize_mxfp8(k, q=st.k[i, ::rows, :T], scale=st.ks[i, ::rows, :T])
                ops.kv_quantize_mxfp8(v, q=st.v[i, ::rows, :T], scale=st.vs[i, ::rows, :T])
            else:                                              # the yardstick: the bf16 cache holds x_hat
                ops.kv_quantize_mxfp8(k, x_hat=st.k[i, ::rows, :T])
                ops.kv_quantize_mxfp8(v, x_hat=st.v[i, ::rows, :T])
        if mode is None:
            st.qw = None
            hidden_p = self._llama(embeds, plan.key_mask, F, kv_out=keep_kv)      # [N, T, H]
        else:
            st.qw = self._quantize_decode_weights(mode)
            hidden_p = self._prefill_quantised(embeds, plan.key_mask, st.qw, keep_kv)
        ragged = attention_mask is not None or rows > 1 or chunk > 1       # (chunk: likewise) beams: every row at its own device-side position (they are equal; the per-row kernels read them)
        if fused != st.fused or mode != st.bits or ragged != st.ragged:
            st.fused, st.bits, st.ragged, st.graph, st.warm = fused, mode, ragged, None, False      # a different kernel sequence: capture again
        st.qkv_w = self._merge_lora() if (fused and cl.lora_r > 0 and mode is None) else None
        return st, hidden_p, T, emb_w, self._w("lm_head.weight", F)

    @torch.no_grad()
    def generate(self, images_clip, input_ids, max_new_tokens=32, eos_token_id=2, pad_token_id=0, use_graph=True, fuse_decode=True,
                 weight_bits=None, attention_mask=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=None, uniforms=None,
                 return_logprobs=False, num_beams=1, length_penalty=1.0, early_stopping=False, return_beam_scores=False, beam_cache="indirect", _beam_trace=None,
                 weight_format=None, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, kv_format=None, kv_cache="packed", prompt_lookup_num_tokens=None,
                 max_matching_ngram_size=2, _lookup_forced=None, _lookup_trace=None):
        """Greedy generation (or sampling: do_sample, or beam search: num_beams, both below).  images_clip bf16 [N, 3, 224, 224] (one image per sequence), input_ids int64 [N, L] holding exactly one
        IMAGE_TOKEN_INDEX each.
        -> (sequences int64 [N, L + n_new], hidden bf16 [N, T + n_new - 1, H]: final-norm hidden state of every token but the last).
        attention_mask (bool [N, L], None = every token is a prompt token): prompts of different lengths, RIGHT-padded (`pad_prompts` builds
        the pair).  Row i is its first L_i = attention_mask[i].sum() tokens and must hold its <image> token among them; both tensors are
        trimmed to Lm = max L_i, and a mask that is all True after that is the call without a mask (the same kernels on the same route).
        Otherwise every decode step runs each sequence at its own position (`llmseg_decode_attn_rows`: head_dim 128 and fuse_decode only),
        and both results are packed per row, left-aligned: sequences [N, Lm + n_new] holds row i's prompt, its n_new new tokens, then
        pad_token_id (0 if None); hidden [N, Tm + n_new - 1, H] holds row i's T_i = L_i - 1 + n_img_tokens prefill states, the state of its
        k-th fed token at T_i + k - 1, then zeros -- the layout `seg_embeddings` reads.
        weight_bits = 8 (opt-in; needs fuse_decode, the LoRA is merged first): the greedy continuation of the model whose four per-layer
        matrices (merged q|k|v, o_proj, gate|up, down_proj) are W^ = q * scale, int8 rows with one fp32 scale each (`ops.quantize_rows_i8`);
        lm_head, embeddings, norms, the KV cache and attention stay bf16.  The prefill runs on bf16(W^), the decode steps stream the int8 rows
        (`ops.gemm_w8`): half the bytes of a step.  The weights are re-quantised at every call (`w8_prepare_ms()` gives the cost);
        `decode_weights_i8()` returns them.  Measured at Llama-7B (profiles/w8_decode.md): 2.70 / 2.85 / 3.40 / 4.97 ms per token at 1 / 2 / 4 / 8 sequences
        against 3.33 / 3.88 / 4.33 / 5.08 in bf16 -- at 8 sequences there is no gain (the int8 kernel takes as long as the bf16 kernel there, whatever
        the FMA form) -- and 9.4 ms per call for the merge + quantisation, repaid after about 11 tokens at one sequence.
        weight_format = "mxfp4" (opt-in; needs fuse_decode, the LoRA is merged first; not together with weight_bits): the same scheme on OCP MXFP4 rows -- 4-bit
        E2M1 elements with one power-of-two E8M0 scale per 32 columns, 4.25 bits per weight (`ops.quantize_rows_mxfp4`; the rule is stated in include/llmseg_hip.h).
        W^ = element * 2^e is exact in bf16, so the prefill (on W^) and the decode steps (`ops.gemm_mxfp4` on the packed rows: the vector ALU at 1-2 rows, the
        matrix cores from 3) run exactly one model; lm_head, embeddings, norms, the KV cache and attention stay bf16.  Re-quantised at every call
        (`mxfp4_prepare_ms()`); `decode_weights_mxfp4()` returns the packed rows and scale bytes.  It composes with attention_mask, do_sample, num_beams and
        use_graph as weight_bits=8 does.  Measured at Llama-7B (profiles/mxfp4_decode.md): 2.09 / 2.71 / 3.01 / 3.41 ms per token at 1 / 2 / 4 / 8 sequences against
        int8's 2.71 / 2.89 / 3.42 / 4.99 and bf16's 3.35 / 3.88 / 4.32 / 5.08 in one session (disjoint ranges everywhere; the smallest gain over int8, 7 %, is at 2
        sequences) and 9.1 ms per call for the merge + quantisation.  At one sequence 1.1 of the 2.09 ms are the step's non-GEMM launches.
        do_sample=True: every token is drawn by `ops.sample_tokens` (ONE launch per step: temperature, top-k, top-p, the draw and the eos / pad
        bookkeeping; the rule is stated in include/llmseg_hip.h) instead of the arg-max; everything before the pick -- prefill, decode step,
        hipGraph, weight_bits, attention_mask -- is the greedy route's.  temperature > 0; top_k >= 0 with 0 = OFF (Hugging Face's default is 50:
        pass top_k=50 for its behaviour); 0 < top_p <= 1 with 1 = off.  Ties are kept or dropped as whole groups (HF's TopPLogitsWarper splits a
        group that straddles the top-p boundary by sort order).  The uniforms are one fp32 tensor [N, max_new_tokens] in [0, 1): drawn once before
        the loop from `torch.Generator(device).manual_seed(seed)` (seed=None: torch's global generator), or given as `uniforms=` (not both); step
        s of row n consumes uniforms[n, s], so a call is a pure function of (weights, prompt, arguments, uniforms).  With do_sample=False the
        sampling arguments must stay at their defaults.  return_logprobs=True (sampling only) adds a third result: fp32 [N, n_new], ln of the
        renormalised probability each token was drawn with (0 where a finished row emitted pad_token_id).
        num_beams >= 2: beam search by the rule of Hugging Face's scorer as include/llmseg_hip.h (`llmseg_beam_step`) and tests/beam_checks.py restate it --
        per token the 2 * num_beams best continuations of a prompt's live beams, eos candidates of rank < num_beams become finished hypotheses of value
        sum / length ** length_penalty (the eos counts), a prompt is done once it holds num_beams hypotheses and (early_stopping=True, or) its worst is at
        least the step's best candidate / length ** length_penalty; the result per prompt is its best hypothesis, the live beams included when
        max_new_tokens ends the loop.  The prompt is prefilled ONCE per prompt; the decode state has N * num_beams rows; the pick is one `ops.beam_step`
        (two launches) and one small device-to-host copy per token.  beam_cache="indirect" (default): the KV cache is never moved, every beam reads key t
        from the physical row a [rows, capacity] int32 table names (`llmseg_decode_attn_beams`) and the pick re-orders the table; beam_cache="copy": the same
        loop re-orders K and V physically (`index_select` over every layer) and runs the `llmseg_decode_attn_rows` step -- the same bits, kept as the
        yardstick (profiles/beam_search.md).  Results: sequences [N, L + n_new] with n_new the longest winning length, row i = its prompt, its tokens (eos
        included), then pad_token_id; hidden [N, T + n_new - 1, H] = row i's T prefill states, the state of each fed token of the winner, then zeros;
        return_beam_scores=True adds fp32 [N], the winner's value.  weight_bits=8, weight_format="mxfp4" and use_graph work as in the greedy route.  Out of scope (ValueError):
        do_sample together with beams (beam sampling); an attention_mask that is ragged after trimming; fuse_decode=False; head_dim != 128; num_beams > 16 or
        2 * num_beams > vocab; early_stopping="never"; several returned sequences, diverse groups and constraints have no argument.  With num_beams == 1
        the other beam arguments must stay at their defaults, and not one launch of the routes above changes.
        repetition_penalty (> 0, 1 = off), no_repeat_ngram_size (>= 0, 0 = off), min_new_tokens (>= 0; needs eos_token_id) and suppress_tokens (a sequence of ids in
        [0, vocab)): Hugging Face's RepetitionPenalty / NoRepeatNGram / MinNewTokensLength / SuppressTokens logits processors, in that order, as ONE launch per token
        (`ops.logits_process`, `llmseg_logits_process`; the rule is stated in include/llmseg_hip.h and equals the HF processors on bf16 logits bit for bit) that rewrites
        the step's logits in place BEFORE the pick: the arg-max, or `ops.sample_tokens` (processors come before the warpers, HF's order; return_logprobs then refers to
        the processed distribution).  With any of the four off its default the call keeps each row's history -- its own prompt ids (the <image> placeholder stays in
        and is skipped: HF would index out of range), then every token it emitted -- in one device buffer int64 [N, Lm + max_new_tokens] that the same launch appends
        to, so Lm + max_new_tokens must not exceed `ops.LOGITS_HIST_CAP` (4096).  The history of a finished row goes on collecting pad_token_id (harmless: such a row
        emits pad whatever its logits say).  The decode step is untouched (the pick is outside the captured graph), so use_graph, fuse_decode, weight_bits,
        weight_format, attention_mask and do_sample all compose.  With all four at their defaults no history is built, `ops.logits_process` is never called and every
        route is launch for launch the one above.  Measured at Llama-7B (profiles/generation_controls.md): the four controls add 0.007 / -0.001 ms per token at 1 / 8
        sequences (inside the run-to-run spread) where Hugging Face's processor objects on the device add 0.104 / 0.122.  Out of scope (ValueError): any of the four with
        num_beams >= 2 -- HF applies processors to the log-softmax there, not to the logits: another rule and another `beam_step`.
        kv_format = "mxfp8" (opt-in; needs fuse_decode, head_dim 128 and hidden % 32 == 0): the KV cache holds OCP MXFP8 -- E4M3 bytes with one power-of-two E8M0 scale
        byte per 32 values (`ops.kv_quantize_mxfp8`; the rule is stated in include/llmseg_hip.h) -- 264 KiB instead of 512 KiB per cached token and sequence at
        Llama-7B.  The prefill is untouched (prompt positions attend among themselves in bf16) and writes K and V through the quantiser, one launch per layer and
        tensor; every decode step runs the MXFP8 instance of the decode-attention kernel (`llmseg_decode_attn_mxfp8`) on all three position routes (uniform,
        attention_mask rows, beams with either beam_cache): the new token's k / v enter the step as bf16 and are stored rounded, earlier keys are decoded on load.
        It composes with weight_bits, weight_format, do_sample, the four logits controls, num_beams and use_graph.  kv_cache = "bf16" (needs kv_format) is the
        yardstick: the same model on a bf16 cache that holds x_hat = element * 2^e (the prefill writes x_hat, each step runs the bf16 kernel and then rewrites slot
        [n][pos_n] in place, inside the captured step) -- the same bits as the packed cache at bf16 traffic.  The states of these routes are keyed apart
        (`("kv", kv_format, kv_cache)` joins the key), so a default call never meets them.  Measured at Llama-7B, 64-token prompt, 321 .. 353 keys, in one session,
        alternating (profiles/kv_mxfp8.md): the packed cache is NOT faster at these shapes -- 3.32 / 5.09 ms per token at 1 / 8 sequences against 3.33 / 5.03 with the
        bf16 cache, 5.31 / 6.60 at 3 prompts x 4 / x 16 beams against 5.19 / 6.00 (with MXFP4 weights 2.10 / 3.44 / 5.49 / 14.80 against 2.06 / 3.40 / 5.38 / 14.20): the
        kernel keeps the bf16 instance's lane mapping and spends on the unpack what it saves on the load; what the format buys today is the memory (half the cache).
        After 512 more tokens (833 .. 865 keys) the picture is the same: 3.40 / 5.66 against 3.40 / 5.53 at 1 / 8 sequences, 8.43 against 7.28 at 3 x 16 beams.
        The quantiser adds nothing measurable to the prefill.  Accuracy: E4M3 keeps four significant bits of every cached value; on the tiny test model the
        hidden states differ from the oracle by up to 0.38 (bf16 cache: 0.15) at |h| <= 6.1.
        prompt_lookup_num_tokens = k (an integer 1 .. 7; None = off, the default) with max_matching_ngram_size = g (>= 1, default 2): prompt-lookup decoding, Hugging Face's
        `generate(prompt_lookup_num_tokens=)`.  Per step and row the draft launch (`ops.lookup_draft`) finds the tail n-gram of the row's own history -- its prompt ids as
        given, then what it emitted -- earlier in that history (the longest n-gram <= g that occurs, its earliest occurrence) and drafts the up to k ids behind it; the last
        emitted token and the drafts are Q = k + 1 query rows of ONE decode step (`ops.decode_attn_chunk`: a cached K / V row is loaded once for all Q queries), and the
        accept launch (`ops.lookup_accept`) keeps the longest prefix of drafts that the step's own arg-maxes confirm plus one more token.  Semantics: every emitted token is
        the arg-max of the logits THIS call computed at the position before it, the lowest index among equal values as `torch.argmax`; the call is therefore a greedy
        continuation under the verify step's arithmetic.  It is not bit-identical to the plain route, whose GEMMs see another row count; it agrees with the plain route and
        with the oracle wherever the choice is decidable (the margin rule of tests/generate_checks.py).  Rows advance at different speeds, so both results have the
        per-row, left-aligned layouts of the attention_mask route also when the prompts are equal in length: sequences [N, Lm + n_new] with n_new the largest number of
        tokens any row emitted -- row i holds its prompt, its count_i tokens (eos included), then pad_token_id: the tokens and the shape the plain route returns -- and
        hidden [N, Tm + n_new - 1, H]: row i's T_i prefill states, the state of each token it emitted but its last, then zeros.  The plain route goes on feeding
        pad_token_id to a finished row and returns those states; this mode does not (`seg_embeddings` reads rows in front of a [SEG] only and is unaffected).  It composes
        with attention_mask, weight_bits=8, weight_format="mxfp4", use_graph, eos_token_id / pad_token_id and max_new_tokens.  The history is that of the logits controls:
        Lm + max_new_tokens must not exceed `ops.LOGITS_HIST_CAP`.  N * Q <= 8 step rows stay on the skinny GEMM and on one quantised-GEMM call -- the intended shape is
        one sequence; more rows go where `ops.gemm` and `ops.gemm_rows` send them (the tile GEMM, or 8-row chunks that stream the weights again): correct and slower.
        Out of scope (ValueError): do_sample, num_beams >= 2, the four logits controls, kv_format, fuse_decode=False, head_dim != 128.  With the argument at None not
        one launch of the routes above changes.  `_lookup_forced` (int64 [N, max_new_tokens]: the drafts of a row that has emitted c tokens are forced[n, c : c + k]) and
        `_lookup_trace` (a list that receives per step the rows' draft lengths and accepted counts) are test hooks.  Measured at Llama-7B, one sequence, 64-token prompt, alternating with the plain route in one
        session (profiles/prompt_lookup.md): a step costs 3.98 / 4.41 / 5.27 ms at k = 1 / 3 / 7 against the plain step's 3.35 (MXFP4 rows: 2.80 / 3.12 / 3.62 against 2.06), so
        with every draft accepted a token costs 2.01 / 1.11 / 0.67 ms (0.45 with MXFP4 rows at k = 7) and with none 19 / 31 / 57 % more than on the plain route; break-even is
        0.19 / 0.31 / 0.57 accepted drafts per step (MXFP4: 0.36 / 0.51 / 0.76).  At 8 sequences and k = 3 (32 rows, the tile GEMM) a step costs 5.67 ms against 5.03, and a
        batch ends with its slowest row.  The quantised routes at N * Q > 8 were not measured."""
        controls = _check_controls(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, eos_token_id, max_new_tokens, num_beams)
        _check_beams(self, num_beams, length_penalty, early_stopping, return_beam_scores, beam_cache, _beam_trace, do_sample, fuse_decode)
        sampling = _check_sampling(do_sample, temperature, top_k, top_p, seed, uniforms, return_logprobs, input_ids, max_new_tokens)
        mode = _weight_mode(weight_bits, weight_format, fuse_decode)
        kv = _check_kv(self, kv_format, kv_cache, fuse_decode)
        lookup = _check_lookup(self, prompt_lookup_num_tokens, max_matching_ngram_size, _lookup_forced, _lookup_trace, input_ids, max_new_tokens, do_sample, num_beams,
                               controls, kv, fuse_decode)
        fill = 0 if pad_token_id is None else int(pad_token_id)      # what finished rows and the padding hold
        if lookup is not None:
            return self._generate_lookup(images_clip, input_ids, attention_mask, max_new_tokens, eos_token_id, fill, use_graph, mode, lookup, _lookup_forced, _lookup_trace)
        if num_beams >= 2:
            return self._generate_beams(images_clip, input_ids, max_new_tokens, eos_token_id, fill, use_graph, mode, attention_mask, num_beams, float(length_penalty),
                                        early_stopping, return_beam_scores, beam_cache, _beam_trace, kv)
        input_ids, attention_mask, lens = _row_prompts(self, input_ids, attention_mask, fuse_decode, fill, controls, max_new_tokens)
        return self._generate_rows(images_clip, input_ids, attention_mask, lens, max_new_tokens, eos_token_id, pad_token_id, fill, use_graph, bool(fuse_decode), mode,
                                   sampling, controls, kv)

    def _generate_rows(self, images_clip, input_ids, attention_mask, lens, max_new_tokens, eos_token_id, pad_token_id, fill, use_graph, fused, mode, sampling, controls, kv=()):
        """`generate(num_beams=1)`: the arguments are checked there.  One token per row and step: the pick (`_make_pick`: arg-max or sampling, after the controls),
        the stop test, the decode step on the picked tokens; where positions, hidden states and sequences go is the layout's (uniform, or ragged: lens is not None)."""
        st, hidden_p, T, emb_w, lm_w = self._prefill(images_clip, input_ids, attention_mask, 1, max_new_tokens, mode, fused, (), kv)
        layout = _uniform_rows(st, hidden_p, lm_w, max_new_tokens) if lens is None else _ragged_rows(st, hidden_p, lm_w, max_new_tokens, lens, self.config.n_img_tokens, fill)
        logits, store, pack = layout
        seqs, n_new = [input_ids.to(self.device_)], 0
        pick, live = _make_pick(seqs[0], lens, max_new_tokens, eos_token_id, pad_token_id, sampling, controls)
        while True:
            nxt = pick(logits, n_new)
            seqs.append(nxt[:, None])
            n_new += 1
            # all rows finished (the one host synchronisation of a step; HF's loop has the same), or max_new_tokens tokens added
            if (eos_token_id is not None and int(live.unfinished.max()) == 0) or n_new == max_new_tokens:
                break
            st.x.copy_(ops.gather_rows(emb_w, nxt))
            self._decode_step(st, use_graph)
            store(st.hidden, n_new)
            logits = st.logits
        res = pack(seqs, n_new)
        return res + (torch.cat([lp[:, None] for lp in live.logprobs], 1),) if sampling is not None and sampling["return_logprobs"] else res

    def _generate_lookup(self, images_clip, input_ids, attention_mask, max_new_tokens, eos_token_id, fill, use_graph, mode, lookup, forced, trace):
        """`generate(prompt_lookup_num_tokens=k)`: the arguments are checked there.  Per step: the draft launch, the embedding gather of N * Q tokens, the decode step on
        N * Q rows (captured), the accept launch, one index_copy_ of the step's states into the packed result, one small device-to-host copy.  The first pick after the
        prefill is the accept launch with Q = 1 and no drafts: one pick rule, one eos rule."""
        k, g = lookup
        Q = k + 1
        lens = None
        if attention_mask is not None:
            input_ids, attention_mask, lens = self._ragged_prompts(input_ids, attention_mask)
        if lens is not None:
            input_ids = torch.where(attention_mask.to(input_ids.device), input_ids, torch.full_like(input_ids, fill))
        N, L = input_ids.shape
        if L + max_new_tokens > ops.LOGITS_HIST_CAP:
            raise ValueError(f"prompt_lookup_num_tokens drafts from a history of prompt + max_new_tokens = {L} + {max_new_tokens} ids per row: more than the cap of "
                             f"{ops.LOGITS_HIST_CAP}")
        # a state of its own: no other route meets its step rows or its graph
        st, hidden_p, T, emb_w, lm_w = self._prefill(images_clip, input_ids, attention_mask, 1, max_new_tokens, mode, True, ("lookup", Q), (), chunk=Q)
        dev = self.device_
        H, V, Pn = self.config.llama.hidden, self.config.llama.vocab, self.config.n_img_tokens
        if lens is None:
            lens = torch.full((N,), L, dtype=torch.int64)
        t_rows = (lens - 1 + Pn).to(dev)                       # T_i: row i's prefill length = the position of its first fed token
        st.pos_rows.copy_(t_rows.to(torch.int32))
        rows = T + max_new_tokens - 1
        flat = torch.zeros((N * rows + 1, H), device=dev, dtype=BF16)      # the packed result, row by row, and one dump row for the states of tokens that do not stand
        hidden = flat[:N * rows].view(N, rows, H)
        own = torch.arange(T, device=dev)[None, :] < t_rows[:, None]
        hidden[:, :T] = torch.where(own[:, :, None], hidden_p, torch.zeros_like(hidden_p))
        logits = ops.gemm(ops.gather_rows(hidden_p.reshape(N * T, H), torch.arange(N, device=dev) * T + t_rows - 1), lm_w)      # each row's own last prompt position
        base = torch.arange(N, device=dev) * rows + t_rows - 1           # + count + j: the flat row of `hidden` for the state of step row j
        hist = torch.zeros((N, L + max_new_tokens), dtype=torch.int64, device=dev)      # each row's history, left-aligned: its prompt, then what it emitted
        hist[:, :L] = input_ids.to(dev)
        hist_len = lens.to(torch.int32).to(dev)
        count = torch.zeros((N,), dtype=torch.int32, device=dev)
        unfinished = torch.ones((N,), dtype=torch.int32, device=dev)
        tok = torch.empty((N, Q), dtype=torch.int64, device=dev)
        draft_len = torch.empty((N,), dtype=torch.int32, device=dev)
        hmap = torch.empty((N * Q,), dtype=torch.int64, device=dev)
        rec = torch.empty((4, N), dtype=torch.int32, device=dev)
        ws = torch.empty((N * Q,), dtype=torch.int32, device=dev)
        forced = None if forced is None else forced.to(dev).contiguous()
        state = dict(hist=hist, hist_len=hist_len, pos_rows=st.pos_rows, unfinished=unfinished, count=count, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                     rec=rec, workspace=ws)
        ops.lookup_accept(logits, None, None, first=True, **state)
        while True:
            rec_h = rec.cpu()                                  # the one host synchronisation of a step
            if not bool(((rec_h[0] != 0) & (rec_h[1] < max_new_tokens)).any()):      # every row finished or full
                break
            ops.lookup_draft(hist, hist_len, count, unfinished, k, g, max_new_tokens, V, fill, forced=forced, tok=tok, draft_len=draft_len)
            st.x.copy_(ops.gather_rows(emb_w, tok.view(-1)))
            self._decode_step(st, use_graph)
            ops.lookup_accept(st.logits, tok, draft_len, base=base, dump_row=N * rows, map=hmap, **state)
            flat.index_copy_(0, hmap, st.hidden)
            if trace is not None:
                r = rec.cpu()
                trace.append(dict(draft_len=r[3].tolist(), accepted=r[2].tolist()))
        counts = rec_h[1].to(torch.int64)
        n_new = int(counts.max())
        keep = torch.arange(L + n_new)[None, :] < (lens + counts)[:, None]
        out = torch.where(keep.to(dev), hist[:, :L + n_new], torch.full_like(hist[:, :L + n_new], fill))      # row i: prompt, its count_i tokens, fill
        return out, hidden[:, :T + n_new - 1]

    def _generate_beams(self, images_clip, input_ids, max_new_tokens, eos_token_id, fill, use_graph, mode, attention_mask, B, length_penalty, early_stopping,
                        return_beam_scores, beam_cache, trace, kv=()):
        """`generate(num_beams=B >= 2)`: the arguments are checked there.  The device loop; hypotheses, the done rule and the winners are the `BeamBook`'s."""
        if attention_mask is not None:
            input_ids, attention_mask, lens = self._ragged_prompts(input_ids, attention_mask)
            if lens is not None:
                raise ValueError("num_beams >= 2 with prompts of different lengths (an attention_mask that is ragged after trimming) is out of scope")
        indirect = beam_cache == "indirect"
        # a state of its own: a greedy call on N * B sequences never meets a beam call's graph
        st, hidden_p, T, emb_w, lm_w = self._prefill(images_clip, input_ids, None, B, max_new_tokens, mode, True, ("beams", beam_cache), kv)
        dev = self.device_
        N, L = input_ids.shape
        R, H = N * B, self.config.llama.hidden
        if st.src_a is None:                                   # a new state
            st.src_a, st.src_b = (torch.zeros((R, st.cap), device=dev, dtype=torch.int32) for _ in range(2))
            st.beam_src = st.src_a if indirect else None
        st.pos_rows.fill_(T)
        logits = ops.gemm(hidden_p[:, -1].contiguous(), lm_w)      # [N, V]: the first pick reads one row per prompt
        scores = torch.zeros((N,), device=dev, dtype=torch.float32)
        done_dev = torch.zeros((N,), device=dev, dtype=torch.int32)
        # the pick's small outputs in ONE buffer, so that one copy brings them to the host: step_best [N] | fin_count [N] | fin_parent [N, B] | fin_score [N, B]
        rec = torch.zeros((2 * N + 2 * N * B,), device=dev, dtype=torch.int32)
        ws = torch.empty((R * 2 * B,), device=dev, dtype=torch.int64)
        row0 = torch.arange(R, device=dev) // B * B
        book = BeamBook(N, B, length_penalty, early_stopping, eos_token_id)
        toks, pars, hids = [], [], []
        step = 0
        while True:
            out = dict(next_token=torch.empty((R,), device=dev, dtype=torch.int64), parent=torch.empty((R,), device=dev, dtype=torch.int32),
                       next_scores=torch.empty((R,), device=dev, dtype=torch.float32), step_best=rec[:N].view(torch.float32), fin_count=rec[N:2 * N],
                       fin_parent=rec[2 * N:2 * N + N * B].view(N, B), fin_score=rec[2 * N + N * B:].view(torch.float32).view(N, B))
            ops.beam_step(logits, scores, done_dev, st.src_a, st.src_b, st.pos_rows, B, eos_token_id=eos_token_id, pad_token_id=fill, out=out, workspace=ws)
            st.src_a.copy_(st.src_b)                           # (entries at or beyond a row's position are never read: whatever they hold is copied along)
            rec_h = rec.cpu()                                  # the one host synchronisation of a step
            if trace is not None:
                trace.append(dict(logits=logits.float().cpu(), scores=scores.cpu(), done=list(book.done), next_token=out["next_token"].cpu(), parent=out["parent"].cpu(),
                                  next_scores=out["next_scores"].cpu(), rec=rec_h.clone()))
            toks.append(out["next_token"])
            pars.append(out["parent"])
            book.step(step, rec_h[:N].view(torch.float32).tolist(), rec_h[N:2 * N].tolist(), rec_h[2 * N:2 * N + N * B].view(N, B).tolist(),
                      rec_h[2 * N + N * B:].view(torch.float32).view(N, B).tolist())
            step += 1
            if all(book.done) or step == max_new_tokens:
                break
            done_dev.copy_(torch.tensor(book.done, dtype=torch.int32))
            scores = out["next_scores"]
            if not indirect:                                   # the yardstick: move every layer's K and V to the beams' new rows
                gidx = row0 + out["parent"]
                for t in (st.k, st.v) + ((st.ks, st.vs) if st.kv_packed else ()):      # (a packed cache: bytes and scale bytes)
                    t.copy_(t.index_select(1, gidx))
            st.x.copy_(ops.gather_rows(emb_w, out["next_token"]))
            self._decode_step(st, use_graph)
            hids.append(st.hidden.clone())
            logits = st.logits
        rows, values, gather = zip(*book.finish(out["next_scores"].cpu().tolist(), torch.stack(toks).cpu().tolist(), torch.stack(pars).cpu().tolist()))
        n_new = max(len(r) for r in rows)
        out_ids = torch.cat([input_ids.cpu(), torch.tensor([r + [fill] * (n_new - len(r)) for r in rows], dtype=torch.int64)], 1)      # row i: prompt, the winner, fill
        hidden = torch.zeros((N, T + n_new - 1, H), device=dev, dtype=BF16)
        hidden[:, :T] = hidden_p
        if hids:
            flat = torch.stack(hids).view(-1, H)
            for n, gi in enumerate(gather):
                if gi:
                    hidden[n, T:T + len(gi)] = flat.index_select(0, torch.tensor(gi, device=dev))
        res = (out_ids.to(dev), hidden)
        return res + (torch.tensor(values, dtype=torch.float32, device=dev),) if return_beam_scores else res

    _beam_pool_add = staticmethod(BeamBook.add)

    @staticmethod
    def _ragged_prompts(input_ids, attention_mask):
        """Checks of `generate(attention_mask=)` -> (input_ids, attention_mask, lens) trimmed to the longest prompt; (input_ids, None, None) when
        every row is full after trimming (the uniform route)."""
        if not torch.is_tensor(attention_mask) or attention_mask.dtype != torch.bool or attention_mask.shape != input_ids.shape or input_ids.dim() != 2:
            raise ValueError(f"attention_mask must be a bool tensor of input_ids' shape {tuple(input_ids.shape)}, got "
                             f"{getattr(attention_mask, 'dtype', type(attention_mask))} {tuple(getattr(attention_mask, 'shape', ()))}")
        am = attention_mask.detach().cpu()
        ids = input_ids.detach().cpu()
        lens = am.sum(1)
        if not torch.equal(am, torch.arange(am.shape[1])[None, :] < lens[:, None]):
            raise ValueError("attention_mask must be right padding: every row a prefix of True (no holes, no left padding)")
        is_img = (ids == IMAGE_TOKEN_INDEX) & am
        if not bool((is_img.sum(1) == 1).all()):
            raise ValueError("every row must hold its one <image> token inside its own prompt (attention_mask cuts it off, or the row is empty)")
        Lm = int(lens.max())
        input_ids = input_ids[:, :Lm]
        if bool((lens == Lm).all()):
            return input_ids, None, None
        return input_ids, am[:, :Lm].contiguous(), lens

    @torch.no_grad()
    def seg_embeddings(self, output_ids, hidden):
        """LISA.py:497-521: rows of `hidden` whose NEXT token is [SEG] (255 leading positions = the image-token expansion) through
        `text_hidden_fcs`; -> list (per sequence) of bf16 [n_seg, out_dim].  Gather first, then the two small GEMMs on those rows only."""
        F = _Direct
        N = output_ids.shape[0]
        Pn = self.config.n_img_tokens
        m = output_ids[:, 1:] == self.seg_token_idx
        m = torch.cat([torch.zeros((N, Pn - 1), dtype=torch.bool, device=m.device), m], 1)
        assert m.shape[1] == hidden.shape[1], (m.shape, hidden.shape)
        idx = m.reshape(-1).nonzero().flatten()
        cnt = [0] + m.sum(1).cumsum(0).tolist()
        rows = ops.gather_rows(hidden.reshape(-1, hidden.shape[-1]), idx)
        if rows.shape[0]:
            h = ops.gemm(rows, self._w("model.text_hidden_fcs.0.0.weight", F), bias=self._w("model.text_hidden_fcs.0.0.bias", F), act=ops.ACT_RELU)
            rows = ops.gemm(h, self._w("model.text_hidden_fcs.0.2.weight", F), bias=self._w("model.text_hidden_fcs.0.2.bias", F))
        else:
            rows = torch.empty((0, self.config.out_dim), device=hidden.device, dtype=BF16)
        return [rows[cnt[i]:cnt[i + 1]] for i in range(N)]
