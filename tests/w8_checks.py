"""int8 weight-only decode (llmseg_amd/csrc/decode_gemm.hip, generate(weight_bits=8)): a torch restatement of the public quantiser arithmetic, hand-built rows,
a case table for `llmseg_gemm_w8` with fp64 references, PER-ELEMENT bounds, an fp32 emulation of what the kernel rounds and mutants (fp64 results of slightly
wrong problems) the bounds must reject, and the state dicts of the generation test.

Everything above `generation_case` runs on the CPU (no import of the HIP library).  tests/test_w8_decode_cpu.py proves on every case that the emulation stays
at <= EMU_MAX of the bound and that every applicable mutant exceeds it by >= MUT_MIN; tests/test_w8_decode_gpu.py holds the kernels to the same bounds.

The quantiser, per row n of W [N, K] bf16 (include/llmseg_hip.h):
    amax = max_k |w|;  scale[n] = amax / 127;  inv = 127 / amax (0 for an all-zero row), both IEEE fp32 divisions;
    q = clamp(rint(w * inv), -127, 127), the product rounded once, ties to even;  w^ = bf16_rne(q * scale).
The bound of one output element of C[m][n] = residual[m][n] + scale[n] sum_k A[m][k] q[n][k], with T the fp64 sum of the absolute values of its n terms,
    T = |scale_n| sum_k |a_k q_k| + |residual|
  fp32 outputs:  |got - ref| <= C_SUM 2^-24 sqrt(n) T
  bf16 outputs:  |got - ref| <= C_BF16 2^-8 |ref| + C_SUM 2^-24 sqrt(n) T
a_k q_k is exact in fp32 (8 + 7 significant bits): the kernel rounds the accumulation, the one multiplication by the scale, the residual add and the store."""
import functools
import math

import torch

from tests.backward_kernel_checks import C_BF16, C_SUM, EMU_MAX, MUT_MIN, Case, ratio  # noqa: F401  (re-exported to the two test files)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------------- the quantiser
def quantize_ref(w):
    """w bf16 [N, K] -> (q int8 [N, K], scale fp32 [N], w_hat bf16 [N, K]): the header's arithmetic in torch fp32 (IEEE division, one rounding per product,
    torch.round = ties to even, the bf16 cast = round to nearest even)"""
    assert w.dtype == BF and w.dim() == 2
    f = w.to(F32)
    amax = f.abs().amax(1)
    scale = amax / torch.tensor(127.0, dtype=F32)
    inv = torch.where(amax > 0, torch.tensor(127.0, dtype=F32) / amax, torch.zeros_like(amax))
    q = torch.round(f * inv[:, None]).clamp(-127, 127)
    w_hat = (q * scale[:, None]).to(BF)
    return q.to(torch.int8), scale, w_hat


HAND_ROWS = ("all_zero", "single_nonzero", "amax_negative", "amax_last_column", "ties_to_even")
TIE_E = -3            # the tie row: amax = 127 * 2^TIE_E, so inv = 2^-TIE_E exactly and w * inv = k + 1/2 exactly


def tie_k(K):
    """the integers k of the tie row's columns 1 .. K - 1 (entry = +-(k + 1/2) 2^e; k + 1/2 <= 126.5 has 8 significant bits: exact in bf16)"""
    return [(5 * j) % 127 for j in range(1, K)]


def hand_rows(K):
    """bf16 [5, K], the rows of HAND_ROWS"""
    g = torch.Generator().manual_seed(K)
    w = torch.zeros(5, K, dtype=F32)
    w[1, 3 % K] = 0.3
    w[2] = torch.randn(K, generator=g) * 0.1
    w[2, 5 % K] = -2.0
    w[3] = torch.randn(K, generator=g) * 0.1
    w[3, K - 1] = 1.5
    w[4, 0] = 127.0 * 2.0 ** TIE_E
    for j, k in enumerate(tie_k(K), start=1):
        w[4, j] = (k + 0.5) * 2.0 ** TIE_E * (-1.0 if j % 2 else 1.0)
    out = w.to(BF)
    assert torch.equal(out[4].float(), w[4]), "the tie row must be exact in bf16"
    return out


def hand_rows_expected_q(K):
    """q of the rows whose result is known without any arithmetic: all_zero, single_nonzero and the tie row (k + 1/2 -> the even neighbour)"""
    zero = torch.zeros(K, dtype=torch.int8)
    single = zero.clone()
    single[3 % K] = 127
    tie = zero.clone()
    tie[0] = 127
    for j, k in enumerate(tie_k(K), start=1):
        tie[j] = (k + 1 if k % 2 else k) * (-1 if j % 2 else 1)
    return {0: zero, 1: single, 4: tie}


QUANT_N = (1, 5, 64, 257)
QUANT_K = (16, 48, 1040, 11008)


def quant_input(N, K, pad):
    """bf16 [N, K + pad] of random rows whose first min(N, 5) rows are the hand-built ones; the padding columns hold large values the call must not read"""
    g = torch.Generator().manual_seed(N * 100003 + K)
    w = (torch.randn(N, K + pad, generator=g) * 0.05).to(BF)
    w[:, K:] = 1000.0
    h = hand_rows(K)
    w[:min(N, 5), :K] = h[5 - min(N, 5):]            # N = 1: the tie row
    return w


# ---------------------------------------------------------------------------------------------------------------------------- the GEMM's table
# The kernel (gemm_stream_kernel<I8, ..>, llmseg_amd/csrc/decode_gemm.hip): a wave owns 4 q rows and walks K in steps of 1024 columns (rows templates 4 and 8, and wherever the workgroup's waves
# split K) or 2048 (templates 1 and 2); at N <= 8192 and K >= 4096 the 4 waves of a workgroup share their rows and the workgroup's step is 4096 (resp. 4 x 1024).
W8_N = (1, 3, 4, 5, 15, 16, 17, 37)
W8_K = (16, 1008, 1024, 1040, 2032, 2048, 2064, 3056, 3072, 3088, 4080, 4096, 4112, 6128, 6144, 6160, 8176, 8192, 8208)
KSPLIT_N, KSPLIT_K = 8192, 4096
DEFAULTS = dict(f32=0, res=0, lda_pad=0, ldq_pad=0, ldr_pad=0, ldc_pad=0)


def rows_template(M):
    return 1 if M == 1 else 2 if M == 2 else 4 if M <= 4 else 8


def G(name, M, N, K, **kw):
    assert not set(kw) - set(DEFAULTS), set(kw) - set(DEFAULTS)
    p = dict(DEFAULTS, **kw)
    return Case("gemm_w8", name, 1, M=M, N=N, K=K, rows=rows_template(M), ksplit=int(N <= KSPLIT_N and K >= KSPLIT_K), **p)


EPI = (dict(), dict(res=1, ldr_pad=3, ldq_pad=16), dict(f32=1, ldq_pad=32, lda_pad=8), dict(f32=1, res=1, lda_pad=24, ldc_pad=5, ldr_pad=8, ldq_pad=16),
       dict(res=1, ldc_pad=2))


@functools.lru_cache(maxsize=1)
def cases():
    cs = []
    i = 0
    for Ms in ((1,), (2,), (3, 4), (5, 6, 7, 8)):
        for j, K in enumerate(W8_K):
            M, N, e = Ms[j % len(Ms)], W8_N[(j + i) % 8], (j + i) % len(EPI)
            cs.append(G(f"m{M}-n{N}-k{K}-e{e}", M, N, K, **EPI[e]))
            i += 1
        for j, K in enumerate((4080, 4096, 4112)):           # more than 8192 rows of q: the waves do not split K however long it is
            M = Ms[-1 - j % len(Ms)]
            cs.append(G(f"m{M}-n8196-k{K}", M, 8196, K, **EPI[(j + i) % 4]))
    for j, M in enumerate((1, 2, 4, 8)):                      # down_proj's K
        cs.append(G(f"m{M}-n64-k11008", M, 64, 11008, **EPI[j]))
    # a bf16 output of a handful of elements need not show 16 missing terms of K (see mutant_names): each such call runs once more with fp32 output
    cs += [G(c.name[len("gemm_w8-"):] + "-f32twin", c.M, c.N, c.K, **dict({k: c.p[k] for k in DEFAULTS}, f32=1)) for c in cs if not c.f32 and c.M * c.N < 64]
    assert len({c.name for c in cs}) == len(cs), "duplicate case name"
    assert {c.M for c in cs} == set(range(1, 9)) and {c.N for c in cs} >= set(W8_N)
    return cs


def dims(case):
    """lda, ldq, ldc, ldr"""
    return case.K + case.lda_pad, case.K + case.ldq_pad, case.N + case.ldc_pad, (case.N + case.ldr_pad if case.res else 0)


def inputs(case):
    """the operands as they lie in memory: a bf16 [M + 1, lda] (row M and the padding columns NaN), q int8 [N + 1, ldq] (padding 127), scale fp32 [N + 1],
    res bf16 [M, ldr]"""
    g = torch.Generator().manual_seed(case.seed)
    M, N, K = case.M, case.N, case.K
    lda, ldq, ldc, ldr = dims(case)
    a = torch.randn(M + 1, lda, generator=g).to(BF)
    a[M] = NAN                                        # one more row than the call knows of (the kernel clamps rows)
    a[:, K:] = NAN
    q = torch.randint(-127, 128, (N + 1, ldq), generator=g, dtype=torch.int32)
    q[:, K:] = 127
    idx = torch.arange(N + 1)
    q[idx, idx % K] = 127                             # q reaches both ends of its range in every row
    q[idx, (idx + 1) % K] = -127
    scale = (torch.rand(N + 1, generator=g) * 0.9 + 0.1) * (2.0 / 127) * K ** -0.5
    if N >= 3:
        scale[1] = 0.0                                # an all-zero W row
    inp = dict(a=a, q=q.to(torch.int8), scale=scale.to(F32))
    if case.res:
        inp["res"] = torch.randn(M, ldr, generator=g).to(BF)
    return inp


def compute(case, inp, mut=None, emu=False):
    """-> (c [M, N] fp64, aux).  Reference (fp64) by default; `mut` = the fp64 result of that wrong problem; `emu` = fp32 arithmetic: the 1024-column steps
    accumulated one after the other, one multiplication by the scale, the residual add, the bf16 store."""
    M, N, K = case.M, case.N, case.K
    lda, ldq, ldc, ldr = dims(case)
    D = F32 if emu else F64
    A = (inp["a"][1:M + 1] if mut == "row_m_plus_1" else inp["a"][:M])[:, :K].to(F64).clone()
    q = inp["q"]
    if mut == "ldq_ignored":
        q = q.reshape(-1)[:(N + 1) * K].reshape(N + 1, K)
    Q = q[:N, :K].to(F64)
    if mut == "q_unsigned":
        Q = torch.where(Q < 0, Q + 256, Q)
    if mut == "last_chunk_dropped":
        A[:, K - 16:] = 0
    s = (inp["scale"][1:N + 1] if mut == "scale_row_plus_1" else inp["scale"][:N]).to(D)
    if emu:
        acc = None
        for t in range(0, K, 1024):
            part = A[:, t:t + 1024].to(F32) @ Q[:, t:t + 1024].to(F32).t()
            acc = part if acc is None else acc + part
        P = acc
    else:
        P = A @ Q.t()
    res = inp["res"][:, :N].to(D) if case.res else None
    if mut == "scale_on_sum_plus_residual":
        v = (P + res) * s
    else:
        v = P * s
        if res is not None:
            v = v + res
    aux = {}
    if not (emu or mut):
        T = (A.abs() @ Q.abs().t()) * s.abs()
        if res is not None:
            T = T + res.abs()
        aux = dict(T=T, n=K + case.res)
    if emu and not case.f32:
        v = v.to(BF)
    return v.to(F64), aux


def mutant_names(case):
    # a bf16 output shows 16 missing terms of K only on an element whose |ref| is small beside them (the bound is relative, 2^-7 |ref|): that takes a few
    # elements to be certain, so the outputs of a handful of elements carry this mutant in fp32 only (their -f32twin cases)
    m = ["last_chunk_dropped"] if case.f32 or case.M * case.N >= 64 else []
    m += ["scale_row_plus_1", "q_unsigned", "row_m_plus_1"]
    if case.res:
        m.append("scale_on_sum_plus_residual")
    if case.ldq_pad and case.N >= 2:
        m.append("ldq_ignored")
    return m


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> (inputs, fp64 reference [M, N], per-element bound)"""
    inp = inputs(case)
    ref, aux = compute(case, inp)
    b = C_SUM * 2.0 ** -24 * math.sqrt(aux["n"]) * aux["T"]
    if not case.f32:
        b = b + C_BF16 * 2.0 ** -8 * ref.abs()
    return inp, ref, b


def emulation_ratio(case):
    inp, ref, bound = reference(case)
    return ratio(compute(case, inp, emu=True)[0], ref, bound)


def mutant_ratios(case):
    inp, ref, bound = reference(case)
    return {name: ratio(compute(case, inp, mut=name)[0], ref, bound) for name in mutant_names(case)}


# ---------------------------------------------------------------------------------------------------------------------------- generation
QUANTISED = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
OUTLIER = 8.0


def generation_states(cfg, seed=3):
    """-> (sd: what the model under test loads, bf16-rounded, LoRA unmerged;  sd_q: the state dict of the model generate(weight_bits=8) must run, built
    independently in torch: LoRA merged (fp64 sum, one bf16 rounding), the restated quantiser, weights := bf16(q * scale), LoRA B := 0;
    restated: {oracle weight name: (q, scale)}).  Element (n, n % K) of each of the 14 quantised matrices is multiplied by OUTLIER before the bf16 rounding:
    with rows that spread, int8 steps are wide enough to show in the hidden states."""
    from oracle import cases as ocases
    sd = ocases.tiny_lisa_state(cfg, seed)
    c = cfg.llama
    names = [f"model.layers.{i}.{m}" for i in range(c.layers) for m in QUANTISED]
    for n in names:
        w = sd[n + ".weight"]
        idx = torch.arange(w.shape[0])
        w[idx, idx % w.shape[1]] *= OUTLIER
    sd = {k: v.to(BF).float() for k, v in sd.items()}
    sd_q, restated = dict(sd), {}
    for n in names:
        w = sd[n + ".weight"].to(F64)
        a = sd.get(n + ".lora_A.default.weight")
        if a is not None and c.lora_r > 0:
            b = sd[n + ".lora_B.default.weight"]
            w = w + (c.lora_alpha / c.lora_r) * (b.to(F64) @ a.to(F64))
            sd_q[n + ".lora_B.default.weight"] = torch.zeros_like(b)
        q, s, w_hat = quantize_ref(w.to(BF))
        sd_q[n + ".weight"] = w_hat.float()
        restated[n] = (q, s)
    return sd, sd_q, restated
