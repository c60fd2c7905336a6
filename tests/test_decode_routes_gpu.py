"""GPU: every route of generate()'s decode step issues the kernel sequence it is known to issue, and that sequence is a pure, replayable one.
  * library launches (`llmseg_launch_count`) of ONE eager decode step on each route, against the table LAUNCHES below.  The table was filled by running
    `route_launches` -- the counting code of this file, unchanged -- on the commit BEFORE the three step bodies of generate.py were folded into one, never
    on the folded code: a route that gains or loses a launch no longer matches it.  (The mxfp4 routes: on the commit before the int8 and MXFP4 decode
    GEMMs and their host paths were folded into one.)
  * `use_graph=True` and `use_graph=False` return the same bits on every route (sequences, hidden states, beam values): a step body that allocates, branches
    or reads host state differently between its eager run and its capture does not.
The model is the tiny head_dim-128 configuration of tests/test_beam_gpu.py (LoRA rank 8, so that the unfused route runs its LoRA launches)."""
import functools

import pytest
import torch

from tests import test_beam_gpu as tb

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 0
LORA_R = 8
# route -> (prompts, arguments of generate()); the decode state has prompts * num_beams rows
ROUTES = {
    "unfused_n2": (2, dict(fuse_decode=False)),
    "fused_n1": (1, dict()),
    "fused_n2": (2, dict()),
    "ragged_n2": (2, dict(ragged=True)),
    "w8_n1": (1, dict(weight_bits=8)),
    "w8_n9": (9, dict(weight_bits=8)),                       # more than 8 rows: `ops.gemm_w8` in chunks of 8
    "mxfp4_n1": (1, dict(weight_format="mxfp4")),            # the vector-ALU stream kernel
    "mxfp4_n3": (3, dict(weight_format="mxfp4")),            # from 3 rows: the matrix-core kernel
    "mxfp4_n9": (9, dict(weight_format="mxfp4")),            # `ops.gemm_mxfp4` in chunks of 8 (8 rows on the matrix cores, 1 on the stream kernel)
    "beams2_indirect": (2, dict(num_beams=2, beam_cache="indirect")),
    "beams2_copy": (2, dict(num_beams=2, beam_cache="copy")),
}
# library launches of one eager decode step, measured on the parent commit (see the docstring)
LAUNCHES = {
    "unfused_n2": 28,
    "fused_n1": 14,
    "fused_n2": 20,
    "ragged_n2": 20,
    "w8_n1": 20,
    "w8_n9": 28,
    "mxfp4_n1": 20,
    "mxfp4_n3": 20,
    "mxfp4_n9": 28,
    "beams2_indirect": 20,
    "beams2_copy": 20,
}


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield


def generate_route(route, max_new, use_graph, **extra):
    """one generate() call of the route on the tiny model -> (model, prompts [N, L], the call's results)"""
    from llmseg_amd.generate import pad_prompts
    n, kw = ROUTES[route]
    kw = dict(kw, **extra)
    m = tb._hip_model(LORA_R)
    _, clip, ids, _ = tb._prompts()
    reps = -(-n // 3)
    clip, ids = clip.repeat(reps, 1, 1, 1)[:n], ids.repeat(reps, 1)[:n]
    if kw.pop("ragged", False):                              # rows of 24 and 17 tokens: every sequence at its own position
        ids, mask = pad_prompts([ids[0, :24], ids[1, :17]], PAD)
        kw["attention_mask"] = mask.to(DEV)
    if kw.get("num_beams", 1) >= 2:
        kw["return_beam_scores"] = True
    res = tb._guarded(route, lambda: m.generate(clip.to(DEV), ids.to(DEV), max_new_tokens=max_new, eos_token_id=None, pad_token_id=PAD, use_graph=use_graph, **kw))
    return m, ids, res


def route_launches(route):
    """library launches of one eager decode step on the state a two-token eager call of the route leaves behind (one step taken, room for more)"""
    from llmseg_amd import _lib
    lib = _lib.load()
    n, kw = ROUTES[route]
    m, ids, _ = generate_route(route, 2, False)
    T = ids.shape[1] - 1 + m.config.n_img_tokens
    cap = (T + 2 + 63) // 64 * 64
    B = kw.get("num_beams", 1)
    st = m._decode_states[(n, cap) if B == 1 else (n * B, cap, "beams", kw["beam_cache"])]
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    tb._guarded(route, lambda: m._decode_step(st, use_graph=False))
    return lib.llmseg_launch_count() - n0


@pytest.mark.parametrize("route", list(ROUTES))
def test_launches_of_one_decode_step(route):
    got = route_launches(route)
    print(f"\n{route}: {got} launches (table: {LAUNCHES[route]})")
    assert got == LAUNCHES[route]


@functools.lru_cache(maxsize=None)
def _four_tokens(route, use_graph):
    return tuple(t.cpu() for t in generate_route(route, 4, use_graph)[2])


@pytest.mark.parametrize("route", list(ROUTES))
def test_graph_replay_gives_the_bits_of_eager_steps(route):
    """max_new_tokens=4 is three decode steps: eager (the warm-up), captured and replayed, replayed.  Two prompts per call, but for the routes that ARE a row
    count (one sequence; nine rows)."""
    graph, eager = _four_tokens(route, True), _four_tokens(route, False)
    assert len(graph) == len(eager) == (3 if "beams" in route else 2)
    assert torch.equal(graph[0], eager[0]), f"{route}: sequences differ"
    for a, b in zip(graph[1:], eager[1:]):
        assert tb._same(a, b), f"{route}: hidden states or beam values differ"
