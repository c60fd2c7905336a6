"""MXFP4 weight-only decode (llmseg_amd/csrc/decode_gemm.hip, generate(weight_format="mxfp4")): a torch restatement of the public quantiser arithmetic, hand-built
blocks with known codes, a case table for `llmseg_gemm_mxfp4` with fp64 references, PER-ELEMENT bounds, an fp32 emulation of what the kernel rounds and mutants
(fp64 results of slightly wrong problems) the bounds must reject, and the state dicts of the generation tests.

Everything runs on the CPU (no import of the HIP library).  tests/test_mxfp4_decode_cpu.py proves on every case that the emulation stays at <= EMU_MAX of the
bound and that every applicable mutant exceeds it by >= MUT_MIN; tests/test_mxfp4_decode_gpu.py holds the kernels to the same bounds.

The format, per row n of W [N, K] bf16 and per block of 32 consecutive columns (include/llmseg_hip.h):
    amax = max |w|;  e = the smallest integer >= -127 with amax <= 6 * 2^e (-127 for amax == 0);  scale byte = e + 127 (E8M0);
    x = w / 2^e (exact);  |x| -> the nearest of VALUES = {0, 0.5, 1, 1.5, 2, 3, 4, 6} (codes 0 .. 7), a tie to the even code;  code = sign << 3 | magnitude,
    no sign on magnitude 0;  byte j = element 2 j (low nibble) | element 2 j + 1 (high nibble);  w^ = element * 2^e, exact in bf16.
The bound of one output element of C[m][n] = residual[m][n] + sum_k A[m][k] w^[n][k], with T the fp64 sum of the absolute values of its n terms,
    T = sum_k |a_k w^_k| + |residual|
  fp32 outputs:  |got - ref| <= C_SUM 2^-24 sqrt(n) T
  bf16 outputs:  |got - ref| <= C_BF16 2^-8 |ref| + C_SUM 2^-24 sqrt(n) T
a_k w^_k is exact in fp32 (8 + 2 significant bits): the kernel rounds the accumulation, the residual add and the store."""
import functools
import math

import torch

from tests.backward_kernel_checks import C_BF16, C_SUM, EMU_MAX, MUT_MIN, Case, ratio  # noqa: F401  (re-exported to the two test files)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


# ---------------------------------------------------------------------------------------------------------------------------- the quantiser
def block_exponent(amax):
    """amax fp64 >= 0 (any shape) -> int64 e: the smallest integer >= -127 with amax <= 6 * 2^e.  frexp is exact: amax = m 2^E with m in [1, 2) gives
    E - 2 when m <= 1.5 and E - 1 otherwise"""
    m, ex = torch.frexp(amax)                          # amax = m * 2^ex, m in [0.5, 1)
    e = ex.to(torch.int64) - 1 - 2 + (2 * m > 1.5).to(torch.int64)
    return torch.where(amax > 0, e.clamp(min=-127), torch.full_like(e, -127))


def magnitude_code(x):
    """|x| fp64 in [0, 6] -> int64 code 0 .. 7 of the nearest VALUES entry; at the midpoint between codes i and i + 1 the even one wins"""
    code = torch.zeros(x.shape, dtype=torch.int64)
    for i in range(7):
        mid = (VALUES[i] + VALUES[i + 1]) / 2
        code += ((x > mid) | ((x == mid) & ((i + 1) % 2 == 0))).to(torch.int64)
    return code


def quantize_mxfp4_ref(w):
    """w bf16 [N, K], K % 32 == 0 -> (packed uint8 [N, K / 2], scale uint8 [N, K / 32], w_hat bf16 [N, K]): the header's rule in fp64, where every step is exact"""
    assert w.dtype == BF and w.dim() == 2 and w.shape[1] % BLOCK == 0
    N, K = w.shape
    f = w.to(F64).view(N, K // BLOCK, BLOCK)
    assert bool(torch.isfinite(f).all())
    amax = f.abs().amax(-1)
    e = block_exponent(amax)
    assert bool((amax <= 6 * torch.ldexp(torch.ones_like(amax), e)).all()) and int(e.max()) <= 126
    x = torch.ldexp(f, -e[..., None])
    mag = magnitude_code(x.abs())
    code = torch.where(mag > 0, mag + 8 * (f < 0).to(torch.int64), mag).view(N, K)
    packed = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    val = torch.tensor(VALUES, dtype=F64)[mag] * torch.where((f < 0) & (mag > 0), -1.0, 1.0)      # the element is what the code says: magnitude 0 is +0
    w_hat = torch.ldexp(val, e[..., None]).view(N, K)
    return packed, (e + 127).to(torch.uint8), w_hat.to(BF)


def dequantize(packed, scale, K, swap=False, no_sign=False, table=VALUES, bias=127):
    """packed uint8 [N, >= K / 2], scale uint8 [N, >= K / 32] -> W^ fp64 [N, K]; the keywords are the mutants' wrong readings"""
    p = packed[:, :K // 2].to(torch.int64)
    lo, hi = p & 15, p >> 4
    code = torch.stack((hi, lo) if swap else (lo, hi), -1).view(p.shape[0], K)
    v = torch.tensor(table, dtype=F64)[code & 7]
    if not no_sign:
        v = torch.where(code >= 8, -v, v)
    e = scale[:, :K // BLOCK].to(torch.int64) - bias
    return (v.view(-1, K // BLOCK, BLOCK) * torch.ldexp(torch.ones(e.shape, dtype=F64), e)[..., None]).view(-1, K)


def nibbles(packed):
    """packed uint8 [N, K / 2] -> the 4-bit codes int64 [N, K]"""
    p = packed.to(torch.int64)
    return torch.stack((p & 15, p >> 4), -1).view(p.shape[0], -1)


HAND_BLOCKS = ("all_zero", "single_nonzero", "amax_negative", "amax_last_column", "amax_1p5_is_element_6", "next_bf16_steps_the_scale", "all_ties_both_signs",
               "small_negative_is_plus_zero", "neighbours_2p10_apart")


def hand_blocks(K=64):
    """-> (w bf16 [9, K], codes int64 [9, K], scale bytes int64 [9, K / 32]): the rows of HAND_BLOCKS with the codes worked out BY HAND (no call of the restatement).
    The rows are laid out over two blocks; K = 32 keeps the first (blocks are independent), larger K appends all-zero blocks."""
    R, W = len(HAND_BLOCKS), max(K, 64)
    w = torch.zeros(R, W, dtype=F64)
    c = torch.zeros(R, W, dtype=torch.int64)
    s = torch.zeros(R, W // BLOCK, dtype=torch.int64)                  # an all-zero block: e = -127, byte 0

    def put(r, col, value, code):
        w[r, col], c[r, col] = value, code
    # 1: one non-zero, 1.0 = 1 * 2^0: m <= 1.5 so e = -2, x = 4 -> code 6
    put(1, 3, 1.0, 6); s[1, 0] = 125
    # 2: amax = |-2| = 1 * 2^1: e = -1;  -2 -> x = -4 -> 8 | 6;  0.5 -> 1 -> 2;  1.0 -> 2 -> 4;  -0.25 -> -0.5 -> 8 | 1
    put(2, 5, -2.0, 14); put(2, 0, 0.5, 2); put(2, 1, 1.0, 4); put(2, 2, -0.25, 9); s[2, 0] = 126
    # 3: amax in the block's last column.  3 = 1.5 * 2^1: e = -1, x = 6 -> 7; 0.5 -> 1 -> 2.  Second block: -6 = -1.5 * 2^2: e = 0, code 8 | 7
    put(3, 31, 3.0, 7); put(3, 0, 0.5, 2); s[3, 0] = 126
    put(3, 63, -6.0, 15); s[3, 1] = 127
    # 4: amax = 1.5 * 2^-3 exactly: e = -5 and the element is 6
    put(4, 7, 0.1875, 7); s[4, 0] = 122
    # 5: the next bf16 above it, (1.5 + 2^-7) * 2^-3: m > 1.5 so e = -4, x = 3.015625 -> 3 = code 5
    put(5, 7, (1.5 + 2.0 ** -7) * 0.125, 5); s[5, 0] = 123
    # 6: amax = 6 (e = 0) and every tie with both signs: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4 (codes 0 2 2 4 4 6 6)
    put(6, 0, 6.0, 7); s[6, 0] = 127
    for j, (t, code) in enumerate(zip((0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0), (0, 2, 2, 4, 4, 6, 6))):
        put(6, 1 + 2 * j, t, code)
        put(6, 2 + 2 * j, -t, code + 8 if code else 0)
    # 7: amax = 4 (e = 0); -0.125 rounds to magnitude 0 and is stored as code 0, not 8
    put(7, 10, 4.0, 6); put(7, 11, -0.125, 0); s[7, 0] = 127
    # 8: block 0 has amax 1 (e = -2), block 1 has amax 1024 (e = 8): 0.5 -> 2 -> code 4 there, 512 -> 2 -> code 4 and 1.0 -> 2^-8 -> code 0 here
    put(8, 0, 1.0, 6); put(8, 9, 0.5, 4); s[8, 0] = 125
    put(8, 40, 1024.0, 6); put(8, 41, 512.0, 4); put(8, 42, 1.0, 0); s[8, 1] = 135
    out = w.to(BF)
    assert torch.equal(out.to(F64), w), "the hand-built values must be exact in bf16"
    if K < W:
        return out[:, :K].contiguous(), c[:, :K].contiguous(), s[:, :K // BLOCK].contiguous()
    return out, c, s


QUANT_N = (1, 5, 64, 257)
QUANT_K = (32, 96, 2080, 11008)


def quant_input(N, K, pad):
    """bf16 [N, K + pad] of random rows whose blocks spread over 12 octaves and whose first min(N, 9) rows are the hand-built ones; the padding columns hold large
    values the call must not read"""
    g = torch.Generator().manual_seed(N * 100003 + K)
    w = torch.randn(N, K + pad, generator=g) * 0.05
    octave = torch.randint(-6, 7, (N, K // BLOCK), generator=g).to(F32)
    w[:, :K] = (w[:, :K].view(N, -1, BLOCK) * torch.exp2(octave)[..., None]).view(N, K)
    w = w.to(BF)
    w[:, K:] = 1000.0
    h = hand_blocks(K)[0]
    n = min(N, h.shape[0])
    w[:n, :K] = h[h.shape[0] - n:]
    return w


# ---------------------------------------------------------------------------------------------------------------------------- the GEMM's table
# The kernels (llmseg_amd/csrc/decode_gemm.hip).  M <= 2, the vector-ALU kernel: a wave owns 4 packed rows and walks K in steps of STEP = 2048 columns (a lane's
# 16-byte load is 32 weights); at N <= KSPLIT_N and K >= KSPLIT_K the 4 waves of a workgroup share their rows and take the steps in turn (wave v: steps v,
# v + 4, ...).  M >= MFMA_ROWS, the matrix-core kernel: a wave owns 16 rows, its unit is UNIT = 128 columns, the NW waves of a workgroup take the units in
# turn (NW = 16 at N <= MFMA_WIDE_N, else 4): a workgroup's step is NW * UNIT = 2048 or 512 columns.
STEP = 2048
UNIT, MFMA_ROWS, MFMA_WIDE_N = 128, 3, 8192
FP4_N = (1, 3, 4, 5, 15, 16, 17, 37)
FP4_K = (32,) + tuple(j * STEP + d for j in (1, 2, 3, 4) for d in (-32, 0, 32))
UNIT_K = (UNIT - 32, UNIT, UNIT + 32, 4 * UNIT - 32, 4 * UNIT, 4 * UNIT + 32)          # around one unit and around the narrow workgroup's step (the wide one's is STEP)
KSPLIT_N, KSPLIT_K = 8192, 8192
DEFAULTS = dict(f32=0, res=0, lda_pad=0, ldq_pad=0, lds_pad=0, ldr_pad=0, ldc_pad=0)


def rows_template(M):
    return 1 if M == 1 else 2 if M == 2 else 4 if M <= 4 else 8


def G(name, M, N, K, **kw):
    assert not set(kw) - set(DEFAULTS), set(kw) - set(DEFAULTS)
    p = dict(DEFAULTS, **kw)
    return Case("gemm_mxfp4", name, 1, M=M, N=N, K=K, rows=rows_template(M), mfma=int(M >= MFMA_ROWS), nw=16 if N <= MFMA_WIDE_N else 4,
                ksplit=int(M < MFMA_ROWS and N <= KSPLIT_N and K >= KSPLIT_K), **p)


EPI = (dict(), dict(res=1, ldr_pad=3, ldq_pad=16, lds_pad=1), dict(f32=1, ldq_pad=32, lda_pad=8), dict(f32=1, res=1, lda_pad=24, ldc_pad=5, ldr_pad=8, ldq_pad=16, lds_pad=3),
       dict(res=1, ldc_pad=2, lds_pad=2))


@functools.lru_cache(maxsize=1)
def cases():
    cs = []
    i = 0
    for Ms in ((1,), (2,), (3, 4), (5, 6, 7, 8)):
        for j, K in enumerate(FP4_K):
            M, N, e = Ms[j % len(Ms)], FP4_N[(j + i) % 8], (j + i) % len(EPI)
            cs.append(G(f"m{M}-n{N}-k{K}-e{e}", M, N, K, **EPI[e]))
            i += 1
    for j, (M, K) in enumerate(((7, KSPLIT_K), (2, KSPLIT_K + 32))):          # more than KSPLIT_N = MFMA_WIDE_N rows: no K split at 2 rows, 4 waves a workgroup at 7
        cs.append(G(f"m{M}-n8196-k{K}", M, 8196, K, **EPI[1 + 2 * j]))
    for j, K in enumerate(UNIT_K):                                # the matrix-core kernel's own steps, wide and narrow workgroup
        cs.append(G(f"m{3 + j}-n{FP4_N[j]}-k{K}-e{j % len(EPI)}", 3 + j, FP4_N[j], K, **EPI[j % len(EPI)]))
    for j, K in enumerate((4 * UNIT - 32, 4 * UNIT, 4 * UNIT + 32, 8 * UNIT + 32)):
        cs.append(G(f"m{8 - j}-n8212-k{K}", 8 - j, 8212, K, **EPI[j]))
    for j, M in enumerate((1, 2, 4, 8)):                          # down_proj's K
        cs.append(G(f"m{M}-n64-k11008", M, 64, 11008, **EPI[j]))
    # a bf16 output of a handful of elements need not show 32 missing terms of K (see mutant_names): each such call runs once more with fp32 output
    cs += [G(c.name[len("gemm_mxfp4-"):] + "-f32twin", c.M, c.N, c.K, **dict({k: c.p[k] for k in DEFAULTS}, f32=1)) for c in cs if not c.f32 and c.M * c.N < 64]
    assert len({c.name for c in cs}) == len(cs), "duplicate case name"
    assert {c.M for c in cs} == set(range(1, 9)) and {c.N for c in cs} >= set(FP4_N)
    return cs


def dims(case):
    """lda, ldq (bytes), lds, ldc, ldr"""
    return (case.K + case.lda_pad, case.K // 2 + case.ldq_pad, case.K // BLOCK + case.lds_pad, case.N + case.ldc_pad, (case.N + case.ldr_pad if case.res else 0))


def inputs(case):
    """the operands as they lie in memory: a bf16 [M + 1, lda] (row M and the padding columns NaN), q uint8 [N + 1, ldq] (every byte value; padding 0xFF),
    scale uint8 [N + 1, lds] (bytes 121 .. 132, both sides of 127; padding 0xFF, the E8M0 NaN), res bf16 [M, ldr]"""
    g = torch.Generator().manual_seed(case.seed)
    M, N, K = case.M, case.N, case.K
    lda, ldq, lds, ldc, ldr = dims(case)
    a = torch.randn(M + 1, lda, generator=g).to(BF)
    a[M] = NAN                                        # one more row than the call knows of (the kernel clamps rows)
    a[:, K:] = NAN
    q = torch.randint(0, 256, (N + 1, ldq), generator=g, dtype=torch.int32).to(torch.uint8)
    q[:, K // 2:] = 0xFF
    scale = torch.randint(121, 133, (N + 1, lds), generator=g, dtype=torch.int32).to(torch.uint8)
    scale[:, K // BLOCK - 1] = 132                    # the last block at the top of the range: 32 columns of 2^-6 would vanish in a sum of thousands at 2^5
    scale[:, K // BLOCK:] = 0xFF
    inp = dict(a=a, q=q, scale=scale)
    if case.res:
        inp["res"] = (torch.randn(M, ldr, generator=g) * 8 * math.sqrt(K)).to(BF)      # of the products' order: a * w^ has an rms near 27
    return inp


SWAP_3_4 = (0.0, 0.5, 1.0, 1.5, 2.0, 4.0, 3.0, 6.0)
ROWS = 1024                                           # W^ is built and contracted this many rows at a time (N = 8196 at K = 8224 is 0.5 GB in fp64)


def compute(case, inp, mut=None, emu=False):
    """-> (c [M, N] fp64, aux).  Reference (fp64) by default; `mut` = the fp64 result of that wrong problem; `emu` = fp32 arithmetic in the kernel's order: a
    lane's partial grows step by step (a wave's steps; with the K split, wave v takes steps v, v + 4, ... and the four waves' sums are added as (0 + 1) + (2 + 3));
    on the matrix cores wave v adds its units v, v + NW, ... one after the other and the NW tiles are added in a tree of fours; then the residual add and the
    bf16 store."""
    M, N, K = case.M, case.N, case.K
    lda, ldq, lds, ldc, ldr = dims(case)
    A = (inp["a"][1:M + 1] if mut == "row_m_plus_1" else inp["a"][:M])[:, :K].to(F64).clone()
    if mut == "last_block_dropped":
        A[:, K - BLOCK:] = 0
    q, s = inp["q"], inp["scale"]
    if mut == "ldq_ignored":
        q = q.reshape(-1)[:(N + 1) * (K // 2)].reshape(N + 1, K // 2)
    if mut == "lds_ignored":
        s = s.reshape(-1)[:(N + 1) * (K // BLOCK)].reshape(N + 1, K // BLOCK)
    if mut == "scale_block_plus_1":
        s = torch.roll(s[:, :K // BLOCK], -1, 1)
    kw = dict(swap=mut == "nibbles_swapped", no_sign=mut == "sign_ignored", table=SWAP_3_4 if mut == "table_3_4_exchanged" else VALUES,
              bias=126 if mut == "scale_bias_off_by_one" else 127)
    P = torch.empty(M, N, dtype=F64)
    T = torch.empty(M, N, dtype=F64)
    for r in range(0, N, ROWS):
        W = dequantize(q[r:min(r + ROWS, N)], s[r:min(r + ROWS, N)], K, **kw)
        if emu:
            A32, W32 = A.to(F32), W.to(F32)
            S = UNIT if case.mfma else STEP
            parts = [A32[:, t:t + S] @ W32[:, t:t + S].t() for t in range(0, K, S)]
            if case.mfma:
                waves = []
                for v in range(case.nw):
                    acc = torch.zeros(M, W.shape[0], dtype=F32)
                    for part in parts[v::case.nw]:
                        acc = acc + part
                    waves.append(acc)
                fours = [(waves[g] + waves[g + 1]) + (waves[g + 2] + waves[g + 3]) for g in range(0, case.nw, 4)]
                acc = fours[0] if case.nw == 4 else (fours[0] + fours[1]) + (fours[2] + fours[3])
            elif case.ksplit:
                waves = []
                for v in range(4):
                    acc = torch.zeros(M, W.shape[0], dtype=F32)
                    for part in parts[v::4]:
                        acc = acc + part
                    waves.append(acc)
                acc = (waves[0] + waves[1]) + (waves[2] + waves[3])
            else:
                acc = parts[0]
                for part in parts[1:]:
                    acc = acc + part
            P[:, r:r + ROWS] = acc.to(F64)
        else:
            P[:, r:r + ROWS] = A @ W.t()
            if not mut:
                T[:, r:r + ROWS] = A.abs() @ W.abs().t()
    v = P.to(F32) if emu else P
    if case.res:
        res = inp["res"][:, :N].to(F32 if emu else F64)
        v = v + (2 * res if mut == "residual_scaled" else res)
    aux = {}
    if not (emu or mut):
        if case.res:
            T = T + inp["res"][:, :N].to(F64).abs()
        aux = dict(T=T, n=K + case.res)
    if emu and not case.f32:
        v = v.to(BF)
    return v.to(F64), aux


def mutant_names(case):
    # a bf16 output shows 32 missing terms of K only on an element whose |ref| is small beside them (the bound is relative, 2^-7 |ref|): that takes a few
    # elements to be certain, so the outputs of a handful of elements carry this mutant in fp32 only (their -f32twin cases)
    m = ["last_block_dropped"] if case.f32 or case.M * case.N >= 64 else []
    m += ["nibbles_swapped", "sign_ignored", "scale_bias_off_by_one", "table_3_4_exchanged", "row_m_plus_1"]
    if case.K >= 2 * BLOCK:                           # one block: there is no other block's scale to take
        m.append("scale_block_plus_1")
    if case.res:
        m.append("residual_scaled")
    if case.ldq_pad and case.N >= 2:
        m.append("ldq_ignored")
    if case.lds_pad and case.N >= 2:
        m.append("lds_ignored")
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
MEMBERS = (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("self_attn.o_proj.weight", ("self_attn.o_proj",)),
           ("gate_up", ("mlp.gate_proj", "mlp.up_proj")), ("mlp.down_proj.weight", ("mlp.down_proj",)))      # generate()'s matrix names and the oracle weights in them


def generation_states_mxfp4(cfg, seed=3):
    """-> (sd: what the model under test loads -- `w8_checks.generation_states`' own, bf16-rounded, LoRA unmerged;  sd_q: the state dict of the model
    generate(weight_format="mxfp4") must run, built independently in torch: LoRA merged (fp64 sum, one bf16 rounding), the restated quantiser, weights := W^,
    LoRA B := 0;  sd_8: the int8 mode's model on the same weights;  restated: {oracle weight name: (packed, scale)}).  The tests do not write to any of them."""
    from tests import w8_checks as wc
    sd, sd_8, _ = wc.generation_states(cfg, seed)
    c = cfg.llama
    sd_q, restated = dict(sd), {}
    for n in [f"model.layers.{i}.{m}" for i in range(c.layers) for m in QUANTISED]:
        w = sd[n + ".weight"].to(F64)
        a = sd.get(n + ".lora_A.default.weight")
        if a is not None and c.lora_r > 0:
            b = sd[n + ".lora_B.default.weight"]
            w = w + (c.lora_alpha / c.lora_r) * (b.to(F64) @ a.to(F64))
            sd_q[n + ".lora_B.default.weight"] = torch.zeros_like(b)
        packed, scale, w_hat = quantize_mxfp4_ref(w.to(BF))
        sd_q[n + ".weight"] = w_hat.float()
        restated[n] = (packed, scale)
    return sd, sd_q, sd_8, restated
