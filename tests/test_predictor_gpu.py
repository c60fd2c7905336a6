"""GPU: the SAM predictor (llmseg_amd/predictor.py) and its two kernels against the fp64 restatements and bounds of tests/predictor_checks.py (validated on
the CPU by tests/test_predictor_cpu.py), and end to end against the decoder oracle under the project's decoder policy (tests/sam_decoder_checks.py:
max(2e-2 scale, 1.5 e_lo) with e_lo the bf16-CPU oracle's own error on the same inputs)."""
import functools

import numpy as np
import pytest
import torch

from oracle import cases, sam_decoder as osd
from tests import predictor_checks as pk

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
GUARD = 512                      # canary elements on each side of an output (a multiple of 8: the output stays 16-byte aligned)
INPUT_SIZE, ORIGINAL_SIZE = (683, 1024), (427, 640)
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield
    for kind in sorted(_WORST):
        print(f"\npredictor kernels: worst |kernel - fp64| / bound, {kind}: {_WORST[kind]:.3f}")


@pytest.fixture(autouse=True)
def _fault_guard():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                            # a device fault: nothing more may be started on this GPU
        pytest.exit(f"device fault: {e}", returncode=3)


def _worst(kind, ratio):
    _WORST[kind] = max(_WORST.get(kind, 0.0), ratio)


def _canary(n, dtype=BF):
    """-> (whole buffer of NaN, the view of n elements in its middle)"""
    big = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV, dtype=dtype)
    return big, big[GUARD:GUARD + n]


def _untouched(big, n):
    return bool(big[:GUARD].isnan().all()) and bool(big[GUARD + n:].isnan().all())


@functools.lru_cache(maxsize=None)
def _model():
    """the tiny SAM model of tests/sam_decoder_checks.py::_model with sam_prompts=True and the seeded mask_downscaling tensors"""
    from llmseg_amd import lisa as hip_lisa
    from tests import model_checks as mc
    hcfg = mc.to_hip_cfg(cases.tiny_lisa_cfg("sam"))
    hcfg.sam_decoder = True
    hcfg.sam_prompts = True
    m = hip_lisa.LISAForCausalLM(hcfg, device=DEV).init_random(seed=1)
    missing, unexpected = m.load_state_dict(pk.state(), strict=False)
    assert not unexpected and not [k for k in missing if ".prompt_encoder." in k or ".mask_decoder." in k]
    return m


@functools.lru_cache(maxsize=None)
def _feats_cl():
    return pk.feats().reshape(256, 4096).t().contiguous().to(DEV, BF)


def _weights():
    return _model().mask_downscaling_weights()


def _launches():
    from llmseg_amd import _lib
    return _lib.load().llmseg_launch_count()


# ------------------------------------------------------------------------------------------------ kernels against fp64
@pytest.mark.parametrize("nested", [False, True], ids=["raster", "nested"])
@pytest.mark.parametrize("b", pk.DENSE_B)
def test_dense_prompt_kernel_against_fp64(b, nested):
    from llmseg_amd import ops
    m, r, bound, _ = pk.dense_case(b)
    mask = (pk.to_nested(m[:, 0]) if nested else m.reshape(b, 65536)).contiguous().to(DEV)
    n = b * 4096 * 256
    big, out = _canary(n)
    before = _launches()
    got = ops.sam_dense_prompt(_feats_cl(), mask, weights=_weights(), nested=nested, out=out.view(b * 4096, 256))
    assert _launches() - before == 1
    torch.cuda.synchronize()
    assert _untouched(big, n)
    err = (got.view(b, 4096, 256).double().cpu() - r).abs()
    assert bool(torch.isfinite(err).all())
    ratio = float((err / bound).max())
    print(f"dense prompt b={b} {'nested' if nested else 'raster'}: worst error / bound {ratio:.3f}")
    _worst("dense prompt", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("ci", range(len(pk.SPARSE_CASES)), ids=pk.SPARSE_IDS)
def test_prompt_tokens_kernel_against_fp64(ci):
    from llmseg_amd import ops
    coords, labels, boxes, r, bound, _ = pk.sparse_case(ci)
    P, S = _model().params, _model()._samdec()
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    n = r.numel()
    big, out = _canary(n)
    before = _launches()
    got = ops.sam_prompt_tokens(dev(coords), dev(labels), dev(boxes), S["G"].contiguous(), [P[f"{pk.PE}point_embeddings.{i}.weight"] for i in range(4)],
                                P[pk.PE + "not_a_point_embed.weight"], out=out.view(r.shape))
    assert _launches() - before == 1
    torch.cuda.synchronize()
    assert _untouched(big, n) and got.shape == r.shape
    err = (got.double().cpu() - r).abs()
    assert bool(torch.isfinite(err).all())
    ratio = float((err / bound).max())
    print(f"prompt tokens {pk.SPARSE_IDS[ci]}: worst error / bound {ratio:.3f}")
    _worst("prompt tokens", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("b", [1, 3])
def test_dense_prompt_without_mask_is_add_rows(b):
    from llmseg_amd import ops
    f = _feats_cl()
    no_mask = _model().params[pk.PE + "no_mask_embed.weight"]
    n = b * 4096 * 256
    big, out = _canary(n)
    before = _launches()
    got = ops.sam_dense_prompt(f, None, no_mask=no_mask, b=b, out=out.view(b * 4096, 256))
    assert _launches() - before == 1
    ref = ops.add_rows(f.repeat(b, 1), no_mask)
    torch.cuda.synchronize()
    assert _untouched(big, n)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_sam_decode_without_mask_input_is_unchanged():
    m = _model()
    text = cases.sam_decoder_case(b=2)[1].to(DEV, BF)
    low0, iou0 = m.sam_decode(_feats_cl(), text)                                     # positionally, as every caller did before the keyword existed
    before = _launches()
    low1, iou1 = m.sam_decode(_feats_cl(), text, None, False, mask_input=None, mask_nested=False)
    n_none = _launches() - before
    assert torch.equal(low0, low1) and torch.equal(iou0, iou1)
    sparse = m.embed_points(torch.tensor([[100.0, 200.0], [640.5, 30.0]]))
    a = m.sam_decode(_feats_cl(), None, sparse=sparse, multimask_output=True)
    c = m.sam_decode(_feats_cl(), None, sparse=sparse, multimask_output=True, mask_input=None)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # with a mask the keys cost one launch (the dense-prompt kernel) where the route above spends one (add_rows)
    before = _launches()
    m.sam_decode(_feats_cl(), text, mask_input=pk.dense_masks(2).reshape(2, 65536).to(DEV))
    assert _launches() - before == n_none


# ------------------------------------------------------------------------------------------------ predictor end to end
def _predictor():
    p = _model().predictor()
    p.features, p.input_size, p.original_size, p.is_image_set = _feats_cl(), INPUT_SIZE, ORIGINAL_SIZE, True      # what set_image leaves, for a known embedding
    return p


def _oracle(coords, labels, boxes, mask, multimask):
    """fp32 oracle and its bf16-CPU twin on the restated tokens (and emb + restated dense prompt with no_mask_embed zeroed) -> (r_low, r_iou, e_lo, e_io)"""
    out = []
    for dt in (torch.float32, BF):
        sd = dict(pk.as_dtype(pk.state(), dt))
        cast = lambda t: None if t is None else t.to(dt)
        sparse = pk.sparse_tokens(sd, cast(coords), labels, cast(boxes))
        emb = pk.feats().to(dt)[None]
        if mask is not None:
            emb = emb + pk.mask_downscaling(sd, mask.to(dt))
            sd[pk.PE + "no_mask_embed.weight"] = torch.zeros_like(sd[pk.PE + "no_mask_embed.weight"])
            low, iou = zip(*[osd.decode_masks(sd, emb[i:i + 1], None, sparse=sparse[i:i + 1], multimask_output=multimask) for i in range(emb.shape[0])])
            low, iou = torch.cat(low), torch.cat(iou)
        else:
            low, iou = osd.decode_masks(sd, emb, None, sparse=sparse, multimask_output=multimask)
        out.append((low.float(), iou.float()))
    (r_low, r_iou), (l_low, l_iou) = out
    return r_low, r_iou, float((l_low - r_low).abs().max()), float((l_iou - r_iou).abs().max())


def _check_against_oracle(name, got, coords, labels, boxes, mask, multimask):
    masks, iou, low = got
    with torch.no_grad():
        r_low, r_iou, e_lo, e_io = _oracle(coords, labels, boxes, mask, multimask)
    b, C = r_low.shape[:2]
    assert low.shape == (b, C, 256, 256) and low.dtype == torch.float32 and iou.shape == (b, C) and masks.shape == (b, C) + ORIGINAL_SIZE and masks.dtype == torch.bool
    scale = max(1.0, float(r_low.abs().max()))
    tol = max(2e-2 * scale, 1.5 * e_lo)
    err, err_iou = float((low.cpu() - r_low).abs().max()), float((iou.cpu() - r_iou).abs().max())
    print(f"{name}: low-res err {err:.3e} tol {tol:.3e} (bf16-CPU err {e_lo:.2e}, |ref| {scale:.2e}); iou err {err_iou:.3e} tol {max(2e-2, 1.5 * e_io):.3e}")
    assert err <= tol and err_iou <= max(2e-2, 1.5 * e_io)
    rm = osd.postprocess_masks(r_low, INPUT_SIZE, ORIGINAL_SIZE)
    flips = ((masks.cpu() != (rm > 0)) & (rm.abs() > tol)).sum()
    assert int(flips) == 0, f"{name}: {int(flips)} binary-mask pixels differ outside the band"


_PTS = torch.tensor([[[500.0, 375.0], [120.5, 640.25]], [[1023.5, 0.0], [300.0, 512.0]]])
_BOX = torch.tensor([[100.0, 80.0, 800.5, 700.0], [0.0, 0.0, 1023.5, 682.5]])
_COMBOS = {
    "points_multimask": dict(coords=_PTS, labels=torch.tensor([[1, 1], [1, 0]], dtype=torch.int32), multimask=True),
    "points_single": dict(coords=_PTS, labels=torch.tensor([[1, 1], [1, 0]], dtype=torch.int32), multimask=False),
    "boxes": dict(boxes=_BOX, multimask=False),
    "box_negative_point": dict(coords=_PTS[:, :1].contiguous(), labels=torch.tensor([[0], [0]], dtype=torch.int32), boxes=_BOX, multimask=True),
    "box_mask_input": dict(boxes=_BOX, mask=True, multimask=False),
}


@pytest.mark.parametrize("combo", list(_COMBOS))
def test_predict_torch_against_the_decoder_oracle(combo):
    c = _COMBOS[combo]
    coords, labels, boxes = c.get("coords"), c.get("labels"), c.get("boxes")
    mask = pk.dense_masks(2) if c.get("mask") else None
    dev = lambda t: None if t is None else t.to(DEV)
    got = _predictor().predict_torch(dev(coords), dev(labels), dev(boxes), dev(mask), multimask_output=c["multimask"])
    _check_against_oracle(combo, got, coords, labels, boxes, mask, c["multimask"])


def test_refinement_round_feeds_nested_logits_back():
    from llmseg_amd import predictor as hp
    p = _predictor()
    coords, labels = _PTS[:, :1].contiguous(), torch.tensor([[1], [1]], dtype=torch.int32)
    _, _, low1 = p.predict_torch(coords.to(DEV), labels.to(DEV), multimask_output=False, low_res_nested=True)
    assert low1.shape == (2, 1, 65536) and low1.dtype == torch.float32
    fed = low1[:, 0].contiguous()
    got = p.predict_torch(coords.to(DEV), labels.to(DEV), mask_input=fed, multimask_output=False)
    raster = hp.nested_to_raster(fed)[:, None].contiguous()                          # [2, 1, 256, 256]
    _check_against_oracle("refinement round 2 (teacher-forced)", got, coords, labels, None, raster.cpu(), False)
    again = p.predict_torch(coords.to(DEV), labels.to(DEV), mask_input=raster, multimask_output=False)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "the raster and the nested form of one mask prompt give different bits"
    # and the nested low-res output is the raster one, re-ordered
    nested_out = p.predict_torch(coords.to(DEV), labels.to(DEV), mask_input=fed, multimask_output=False, low_res_nested=True)[2]
    assert torch.equal(hp.nested_to_raster(nested_out), got[2])


@pytest.mark.parametrize("size", [(427, 640), (96, 72)], ids=["427x640", "96x72"])
def test_predict_numpy_equals_predict_torch_on_transformed_prompts(size):
    H, W = size
    p = _model().predictor()
    img = torch.as_tensor(cases.amg_image_case(H, W)).to(DEV)
    with pytest.raises(RuntimeError, match="set_image"):
        p.predict(np.array([[1.0, 2.0]]), np.array([1]))
    p.set_image(img)
    assert p.original_size == (H, W) and p.input_size == pk.preprocess_shape(H, W) and p.get_image_embedding().shape == (1, 256, 64, 64)
    pts, labs = np.array([[W * 0.3, H * 0.6], [W - 1.0, 0.0]]), np.array([1, 0])
    box = np.array([W * 0.1, H * 0.2, W * 0.9, H * 0.75])
    mask = pk.dense_masks(1)[0].numpy()                                               # [1, 256, 256]
    for kw in (dict(point_coords=pts, point_labels=labs), dict(box=box, multimask_output=False), dict(point_coords=pts[:1], point_labels=labs[:1], box=box, mask_input=mask)):
        masks, iou, low = p.predict(**kw)
        mm = kw.get("multimask_output", True)
        c_t = None if "point_coords" not in kw else torch.as_tensor(pk.apply_coords(kw["point_coords"], size), dtype=torch.float32)[None].to(DEV)
        l_t = None if "point_labels" not in kw else torch.as_tensor(kw["point_labels"], dtype=torch.int32)[None].to(DEV)
        b_t = None if "box" not in kw else torch.as_tensor(pk.apply_boxes(kw["box"], size), dtype=torch.float32).to(DEV)
        m_t = None if "mask_input" not in kw else torch.as_tensor(kw["mask_input"])[None].to(DEV)
        t_masks, t_iou, t_low = p.predict_torch(c_t, l_t, b_t, m_t, multimask_output=mm)
        C = 3 if mm else 1
        assert masks.shape == (C, H, W) and masks.dtype == np.bool_ and iou.shape == (C,) and low.shape == (C, 256, 256)
        assert torch.equal(torch.as_tensor(masks), t_masks[0].cpu()) and torch.equal(torch.as_tensor(iou), t_iou[0].cpu()) and torch.equal(torch.as_tensor(low), t_low[0].cpu())
        logits = p.predict(return_logits=True, **kw)[0]
        assert logits.dtype == np.float32 and np.array_equal(logits > 0, masks)       # SAM's mask_threshold = 0
    p.reset_image()
    with pytest.raises(RuntimeError, match="set_image"):
        p.predict_torch(None, None, boxes=torch.tensor([[0.0, 0.0, 5.0, 5.0]]))
    with pytest.raises(RuntimeError, match="set_image"):
        p.get_image_embedding()


def test_prompt_validation():
    from tests import image_frontend_checks as fc
    p = _predictor()
    with pytest.raises(ValueError):
        p.predict_torch(_PTS.to(DEV), None)                                           # coordinates without labels
    with pytest.raises(ValueError):
        p.predict(point_coords=np.array([[1.0, 2.0]]))
    with pytest.raises(ValueError):
        p.predict_torch(_PTS.to(DEV), torch.ones((2, 3), dtype=torch.int32))          # labels of another n
    with pytest.raises(ValueError):
        p.predict_torch(_PTS.to(DEV), torch.ones((2, 2), dtype=torch.int32), boxes=_BOX[:1])      # boxes of another b
    with pytest.raises(ValueError):
        p.predict_torch(None, None, boxes=_BOX, mask_input=torch.zeros((2, 1, 128, 128)))
    with pytest.raises(ValueError):
        p.predict_torch(None, None, boxes=_BOX, mask_input=torch.zeros((3, 65536)))
    plain = fc.tiny_model().predictor()                                               # the suite's tiny SAM model: built without sam_prompts
    plain.features, plain.input_size, plain.original_size, plain.is_image_set = _feats_cl(), INPUT_SIZE, ORIGINAL_SIZE, True
    with pytest.raises(ValueError, match="sam_prompts=True"):
        plain.predict_torch(None, None, boxes=_BOX, mask_input=torch.zeros((2, 1, 256, 256)))
    masks, iou, low = plain.predict_torch(None, None, boxes=_BOX.to(DEV), multimask_output=False)      # everything but the mask prompt works there
    assert masks.shape == (2, 1) + ORIGINAL_SIZE and bool(torch.isfinite(low).all())
