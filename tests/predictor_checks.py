"""SAM predictor (llmseg_amd/predictor.py; kernels llmseg_sam_dense_prompt / llmseg_sam_prompt_tokens): fp64 restatements, cases and bounds shared by
tests/test_predictor_cpu.py (which validates the restatements against the reference and the bounds on an fp32 evaluation) and tests/test_predictor_gpu.py.

Restated in fp64 (reference model/segment_anything): `PromptEncoder._embed_points` / `_embed_boxes` (modeling/prompt_encoder.py:78-109,203-238),
`mask_downscaling` (prompt_encoder.py:56-64 with LayerNorm2d, common.py:31-43), `ResizeLongestSide.apply_coords` / `apply_boxes`
(utils/transforms.py:36-60).  Weights: `oracle.cases.sam_decoder_state()` + seeded `mask_downscaling` tensors, all rounded to bf16 (what the model stores).

BOUNDS (per element; nothing here was tuned on a kernel's output).  r is the fp64 value of an output element, u = 2^-24 the unit roundoff of fp32: one
fp32 operation returns its exact result times (1 + d), |d| <= u, and a sum of n products evaluated in any order (fused or not) is within n u sum |terms|
(first order).  A kernel that evaluates every stage in fp32 and rounds once to bf16 returns bf16(r + e) with |e| <= E, so

    |out - r| <= E + 2^-8 (|r| + E)            (bf16 keeps 8 significant bits: half an ulp of x is at most 2^-8 |x|)

E is propagated through the chain in absolute values, stage by stage, alongside the fp64 values:

  conv (n products + bias)   e_out = sum |w| e_in + (n + 1) u (|bias| + sum |w| |x|)
  LayerNorm over C channels  mean:  e_mu = mean e_in + C u mean |x|
                             centred d = x - mu:  e_d = e_in + e_mu + u |d|
                             variance v = mean d^2:  e_v = mean (2 |d| e_d + e_d^2) + (C + 2) u v
                             rs = 1 / sqrt(v + eps) (add, sqrt, divide: 3 u):  relative error rr = e_v / (2 (v + eps - e_v)) + 3 u
                             y = g d rs + beta:  e_y = |g| rs (e_d + |d| rr) + 3 u (|g d rs| + |beta|)
  GELU f(y) = y (1 + erf(y / sqrt 2)) / 2   |f'| <= 1.13 (its maximum, 1.129, is at y = 1.41); erf is taken to be good to 4 ulp of a value <= 1, so 1 + erf
                             carries <= 8 u absolute, the argument's scaling one more rounding, the two products 3 u relative:
                             e_f = 1.13 e_y + 5 u |y| + 3 u |f(y)|
  + feats                    one more rounding: + u |r|

The zero patch (cell 0) and the constant patch (cell 4095) make every stage-1 pixel of a cell equal; the channel variance of LayerNorm2d(4) is then the
variance of (bias_c + const sum w_c), which the distinct seeded biases keep away from 0: v + eps - e_v stays positive (asserted in `ln_bound`).

Tokens: c = 2 ((x + 0.5) / 1024) - 1 costs the rounding of x + 0.5 (the division and the doubling are exact) and of the subtraction:
e_c = u |x + 0.5| / 512 + u |c|;  v = cx G0 + cy G1 (two products, one sum): e_v = |G0| e_cx + |G1| e_cy + 3 u (|cx G0| + |cy G1|);  the argument a = 2 pi v:
fl(2 pi) is within u of 2 pi and the product rounds once: e_a = 2 pi e_v + 2 u |a| -- "the rounding of an argument of that magnitude", ~ 1e-5 at |a| = 80;
sin / cos have slope <= 1 and are taken to be good to 4 ulp of a value <= 1: e_s = e_a + 4 u;  + the label embedding: + u |r|.  A label -1 row is the
not_a_point vector alone: E = 0 there.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cases, seeded

PFX = "model.visual_model."
PE = PFX + "prompt_encoder."
MD = PE + "mask_downscaling."
U = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ weights
def prompt_shapes():
    return {MD + "0.weight": (4, 1, 2, 2), MD + "0.bias": (4,), MD + "1.weight": (4,), MD + "1.bias": (4,), MD + "3.weight": (16, 4, 2, 2), MD + "3.bias": (16,),
            MD + "4.weight": (16,), MD + "4.bias": (16,), MD + "6.weight": (256, 16, 1, 1), MD + "6.bias": (256,)}


@functools.lru_cache(maxsize=None)
def state():
    """fp32 state dict whose every value is a bf16 number: the seeded decoder + seeded mask_downscaling (LayerNorm weights in [0.75, 1.25), biases distinct)."""
    sd = dict(cases.sam_decoder_state())
    for i, (name, shp) in enumerate(prompt_shapes().items()):
        if name.endswith(("1.weight", "4.weight")):
            t = seeded.uniform(shp, 9100 + i, 0.75, 1.25)
        elif name.endswith("6.bias"):
            t = seeded.uniform(shp, 9100 + i, -0.25, 0.25)
        elif name.endswith("bias"):                              # a seeded ordering of evenly spaced values: distinct and non-zero after the bf16 rounding too
            n = shp[0]
            rank = seeded.uniform(shp, 9100 + i).argsort().argsort().float()
            t = (rank - (n - 1) / 2 + 0.25) * (0.4 / n)
        else:
            fan_in = shp[1] * shp[2] * shp[3]
            t = seeded.uniform(shp, 9100 + i, -1.0, 1.0) * (1.7 / fan_in ** 0.5)
        sd[name] = t
    sd = {k: v.to(BF).float() for k, v in sd.items()}
    for k in (MD + "0.bias", MD + "3.bias", MD + "1.bias", MD + "4.bias"):
        assert sd[k].unique().numel() == sd[k].numel() and bool((sd[k] != 0).all()), k
    for k in (MD + "1.weight", MD + "4.weight"):
        assert sd[k].unique().numel() > 1, k
    return sd


def as_dtype(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ restatements (dtype follows the state dict)
def pe_encoding(sd, coords01):
    """PositionEmbeddingRandom._pe_encoding: coords in [0, 1]^2 [..., 2] -> [..., 256]"""
    G = sd[PE + "pe_layer.positional_encoding_gaussian_matrix"]
    c = 2 * coords01 - 1
    if c.dtype != G.dtype:
        c = c.to(G.dtype)
    c = c @ G
    c = 2 * np.pi * c
    return torch.cat([torch.sin(c), torch.cos(c)], -1)


def forward_with_coords(sd, coords, image_size=(1024, 1024)):
    c = coords.clone()
    c[:, :, 0] = c[:, :, 0] / image_size[1]
    c[:, :, 1] = c[:, :, 1] / image_size[0]
    return pe_encoding(sd, c.to(torch.float))                      # the reference normalises in the input's precision, then casts to fp32 (prompt_encoder.py:238)


def embed_points(sd, points, labels, pad):
    """PromptEncoder._embed_points: points [b, n, 2], labels [b, n] -> [b, n + pad, 256]"""
    points = points + 0.5
    if pad:
        points = torch.cat([points, torch.zeros((points.shape[0], 1, 2), dtype=points.dtype)], 1)
        labels = torch.cat([labels, -torch.ones((labels.shape[0], 1), dtype=labels.dtype)], 1)
    e = forward_with_coords(sd, points)
    e[labels == -1] = 0.0
    e[labels == -1] += sd[PE + "not_a_point_embed.weight"]
    e[labels == 0] += sd[PE + "point_embeddings.0.weight"]
    e[labels == 1] += sd[PE + "point_embeddings.1.weight"]
    return e


def embed_boxes(sd, boxes):
    """PromptEncoder._embed_boxes: boxes [b, 4] -> [b, 2, 256]"""
    e = forward_with_coords(sd, (boxes + 0.5).reshape(-1, 2, 2))
    e[:, 0, :] += sd[PE + "point_embeddings.2.weight"]
    e[:, 1, :] += sd[PE + "point_embeddings.3.weight"]
    return e


def sparse_tokens(sd, coords, labels, boxes):
    """PromptEncoder.forward's sparse half: points (padded when there are no boxes), then box corners."""
    dt = sd[PE + "not_a_point_embed.weight"].dtype
    parts = []
    if coords is not None and coords.shape[1] > 0:
        parts.append(embed_points(sd, coords.to(dt), labels, pad=boxes is None))
    if boxes is not None:
        parts.append(embed_boxes(sd, boxes.to(dt)))
    return torch.cat(parts, 1)


def layernorm2d(x, w, b, eps=1e-6):
    mu = x.mean(1, keepdim=True)
    s = (x - mu).pow(2).mean(1, keepdim=True)
    x = (x - mu) / torch.sqrt(s + eps)
    return w[:, None, None] * x + b[:, None, None]


def mask_downscaling(sd, masks):
    """PromptEncoder._embed_masks: masks [b, 1, 256, 256] -> [b, 256, 64, 64]"""
    x = F.conv2d(masks, sd[MD + "0.weight"], sd[MD + "0.bias"], stride=2)
    x = F.gelu(layernorm2d(x, sd[MD + "1.weight"], sd[MD + "1.bias"]))
    x = F.conv2d(x, sd[MD + "3.weight"], sd[MD + "3.bias"], stride=2)
    x = F.gelu(layernorm2d(x, sd[MD + "4.weight"], sd[MD + "4.bias"]))
    return F.conv2d(x, sd[MD + "6.weight"], sd[MD + "6.bias"])


def preprocess_shape(h, w, long_side=1024):
    sc = long_side * 1.0 / max(h, w)
    return int(h * sc + 0.5), int(w * sc + 0.5)


def apply_coords(coords, original_size, long_side=1024):
    old_h, old_w = original_size
    new_h, new_w = preprocess_shape(old_h, old_w, long_side)
    c = np.array(coords).astype(float)
    c[..., 0] = c[..., 0] * (new_w / old_w)
    c[..., 1] = c[..., 1] * (new_h / old_h)
    return c


def apply_boxes(boxes, original_size, long_side=1024):
    return apply_coords(np.asarray(boxes).reshape(-1, 2, 2), original_size, long_side).reshape(-1, 4)


def to_nested(m):
    """[..., 256, 256] -> [..., 65536] in the mask decoder's row order (the permutation of tests/sam_decoder_checks.py)"""
    lead = m.shape[:-2]
    k = len(lead)
    return m.reshape(*lead, 64, 2, 2, 64, 2, 2).permute(*range(k), k, k + 3, k + 1, k + 4, k + 2, k + 5).reshape(*lead, 65536)


def to_raster(m):
    lead = m.shape[:-1]
    k = len(lead)
    return m.reshape(*lead, 64, 64, 2, 2, 2, 2).permute(*range(k), k, k + 2, k + 4, k + 1, k + 3, k + 5).reshape(*lead, 256, 256)


# ------------------------------------------------------------------------------------------------ bounds
def store_bound(r, E):
    """|bf16(r + e) - r| for |e| <= E"""
    return E + 2.0 ** -8 * (r.abs() + E)


def conv_bound(x, ex, w, bias, stride):
    n = w[0].numel()
    mag = F.conv2d(x.abs(), w.abs(), bias.abs(), stride=stride)
    return F.conv2d(ex, w.abs(), None, stride=stride) + (n + 1) * U * mag


def ln_bound(x, ex, g, beta, eps=1e-6):
    """-> (y, e_y) of LayerNorm2d over dim 1"""
    C = x.shape[1]
    mu = x.mean(1, keepdim=True)
    e_mu = ex.mean(1, keepdim=True) + C * U * x.abs().mean(1, keepdim=True)
    d = x - mu
    e_d = ex + e_mu + U * d.abs()
    v = d.pow(2).mean(1, keepdim=True)
    e_v = (2 * d.abs() * e_d + e_d.pow(2)).mean(1, keepdim=True) + (C + 2) * U * v
    assert bool((v + eps - e_v > 0.5 * (v + eps)).all()), "a LayerNorm variance is not resolved in fp32: the first-order bound does not apply"
    rs = 1 / torch.sqrt(v + eps)
    rr = e_v / (2 * (v + eps - e_v)) + 3 * U
    g, beta = g[:, None, None], beta[:, None, None]
    y = g * d * rs + beta
    e_y = g.abs() * rs * (e_d + d.abs() * rr) + 3 * U * ((g * d * rs).abs() + beta.abs())
    return y, e_y


def gelu_bound(y, e_y):
    f = F.gelu(y)
    return f, 1.13 * e_y + 5 * U * y.abs() + 3 * U * f.abs()


def dense_reference(sd64, feats, masks):
    """fp64: feats [256, 64, 64], masks [b, 1, 256, 256] -> (r [b, 4096, 256] = feats + mask_downscaling(masks) as channels-last rows, its bound)"""
    g = lambda n: sd64[MD + n]
    x = F.conv2d(masks, g("0.weight"), g("0.bias"), stride=2)
    e = conv_bound(masks, torch.zeros_like(masks), g("0.weight"), g("0.bias"), 2)
    x, e = gelu_bound(*ln_bound(x, e, g("1.weight"), g("1.bias")))
    x2 = F.conv2d(x, g("3.weight"), g("3.bias"), stride=2)
    e = conv_bound(x, e, g("3.weight"), g("3.bias"), 2)
    x, e = gelu_bound(*ln_bound(x2, e, g("4.weight"), g("4.bias")))
    d = F.conv2d(x, g("6.weight"), g("6.bias"))
    e = conv_bound(x, e, g("6.weight"), g("6.bias"), 1)
    ref = mask_downscaling(sd64, masks)                           # the restatement itself is the reference value; `d` differs from it in fp64 roundings only
    assert float((d - ref).abs().max()) <= 1e-11
    r = feats[None] + ref
    e = e + U * r.abs()
    rows = lambda t: t.flatten(2).permute(0, 2, 1).contiguous()
    return rows(r), rows(store_bound(r, e)), rows(e)


def token_reference(sd64, coords, labels, boxes):
    """fp64 tokens [b, T, 256] and their bound (coords / boxes are fp32 tensors: the kernel's inputs)."""
    r = sparse_tokens(sd64, None if coords is None else coords.to(F64), labels, None if boxes is None else boxes.to(F64))
    G = sd64[PE + "pe_layer.positional_encoding_gaussian_matrix"]
    pts, alone = [], []
    if coords is not None and coords.shape[1] > 0:
        pts.append(coords.to(F64))
        alone.append(labels == -1)
        if boxes is None:
            pts.append(torch.zeros((coords.shape[0], 1, 2), dtype=F64))
            alone.append(torch.ones((coords.shape[0], 1), dtype=torch.bool))
    if boxes is not None:
        pts.append(boxes.to(F64).reshape(-1, 2, 2))
        alone.append(torch.zeros((boxes.shape[0], 2), dtype=torch.bool))
    p, alone = torch.cat(pts, 1) + 0.5, torch.cat(alone, 1)
    c = 2 * (p / 1024) - 1
    e_c = U * p.abs() / 512 + U * c.abs()
    mag = c[..., :1].abs() * G[0].abs() + c[..., 1:].abs() * G[1].abs()
    e_v = e_c[..., :1] * G[0].abs() + e_c[..., 1:] * G[1].abs() + 3 * U * mag
    a = 2 * math.pi * (c @ G)
    e_s = 2 * math.pi * e_v + 2 * U * a.abs() + 4 * U
    E = torch.cat([e_s, e_s], -1) + U * r.abs()
    E = torch.where(alone[..., None], torch.zeros_like(E), E)
    return r, store_bound(r, E), E


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def feats():
    """the structured embedding of the everything-mode tests, as the bf16 numbers the encoder would emit: fp32 [256, 64, 64]"""
    return cases.amg_embedding_case()[0].to(BF).float()


DENSE_B = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def dense_masks(b):
    """fp32 [b, 1, 256, 256] logits at SAM's scale (+-20), a 4 x 4 patch of zeros at cell 0 and a constant patch at cell 4095 of every prompt"""
    m = seeded.uniform((b, 1, 256, 256), 9200 + b, -20.0, 20.0)
    m[:, :, :4, :4] = 0.0
    m[:, :, 252:, 252:] = 7.5
    return m


@functools.lru_cache(maxsize=None)
def dense_case(b):
    """-> (masks fp32 [b, 1, 256, 256], r fp64 [b, 4096, 256], bound, fp32 term)"""
    m = dense_masks(b)
    r, bound, E = dense_reference(as_dtype(state(), F64), feats().to(F64), m.to(F64))
    return m, r, bound, E


def _coords(b, n, seed):
    c = seeded.uniform((b, n, 2), seed, -100.0, 1200.0)
    flat = c.view(-1)
    for i, v in enumerate((0.0, 1023.5, -30.25, 1500.75, 1023.5, 0.0)):          # at 0, at 1023.5, outside the frame
        if i < flat.numel():
            flat[i] = v
    return c


def _boxes(b, seed):
    x = seeded.uniform((b, 4), seed, -50.0, 1100.0)
    x[0] = torch.tensor([0.0, 0.0, 1023.5, 1023.5])
    if b > 1:
        x[1] = torch.tensor([-40.5, 17.25, 1300.0, 1023.5])
    return x


_LABELS5 = [[1, 0, -1, 1, 0], [0, 0, 1, -1, -1], [-1, 1, 1, 0, 1]]
_LABELS2 = [[1, 0], [-1, 1], [0, -1]]
#               b  n  boxes
SPARSE_CASES = [(1, 1, False), (2, 2, False), (3, 5, False), (1, 5, False), (1, 0, True), (3, 0, True), (2, 1, True), (3, 2, True), (2, 5, True)]
SPARSE_IDS = [f"b{b}_n{n}_{'boxes' if bx else 'pad'}" for b, n, bx in SPARSE_CASES]


@functools.lru_cache(maxsize=None)
def sparse_inputs(ci):
    """-> (coords fp32 [b, n, 2] or None, labels int32 [b, n] or None, boxes fp32 [b, 4] or None)"""
    b, n, bx = SPARSE_CASES[ci]
    coords = labels = None
    if n:
        coords = _coords(b, n, 9300 + ci)
        labels = torch.tensor({1: [[1], [0], [-1]], 2: _LABELS2, 5: _LABELS5}[n][:b], dtype=torch.int32)
    return coords, labels, (_boxes(b, 9400 + ci) if bx else None)


@functools.lru_cache(maxsize=None)
def sparse_case(ci):
    coords, labels, boxes = sparse_inputs(ci)
    r, bound, E = token_reference(as_dtype(state(), F64), coords, labels, boxes)
    return coords, labels, boxes, r, bound, E


GOLDEN_CELLS = 512


def golden_cells():
    """the 512 seeded cells (of b * 4096) whose dense embedding tests/golden/sam_prompts.pt stores"""
    return (seeded.uniform((GOLDEN_CELLS,), 9500, 0.0, 1.0) * (2 * 4096)).long().clamp(max=2 * 4096 - 1)


def golden_prompt():
    """the one predict_torch call of the fixture: a positive + a negative point and a box on prompt 0, a mask prompt, single-mask output"""
    return dict(coords=torch.tensor([[[500.0, 375.0], [120.5, 640.25]]]), labels=torch.tensor([[1, 0]], dtype=torch.int32),
                boxes=torch.tensor([[100.0, 80.0, 800.5, 700.0]]), mask=dense_masks(2)[:1].clone())
