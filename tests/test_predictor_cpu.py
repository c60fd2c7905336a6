"""CPU: the SAM predictor's references and bounds (tests/predictor_checks.py) stand on their own.
  * every bound holds, with half of it to spare, for a plain fp32 torch evaluation in the reference's own operation order;
  * the fp64 restatements equal the imported reference modules (when the reference tree is present) and the committed fixture made from them;
  * the nested <-> raster permutation round-trips and is the one the post-processing reads;
  * `sam_prompts=False` leaves the parameter set exactly as it was; the flag is validated."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import ref_harness as rh, sam_decoder as osd
from tests import predictor_checks as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _rows(t):
    return t.flatten(2).permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------ bounds on the reference alone
@pytest.mark.parametrize("b", pk.DENSE_B)
def test_dense_bound_holds_for_fp32_reference_with_half_to_spare(b):
    m, r, bound, E = pk.dense_case(b)
    sd32 = pk.state()
    with torch.no_grad():
        got = _rows(pk.feats()[None] + pk.mask_downscaling(sd32, m)).double()      # F.conv2d / F.gelu in fp32
    err = (got - r).abs()
    ratio_fp32, ratio = float((err / E).max()), float((err / bound).max())
    print(f"dense b={b}: fp32 torch error / fp32 term {ratio_fp32:.3f}, / full bound {ratio:.4f}; bf16-rounded / bound "
          f"{float(((got.float().to(torch.bfloat16).double() - r).abs() / bound).max()):.3f}")
    assert ratio_fp32 <= 0.5 and ratio <= 0.5
    # the same evaluation rounded to bf16 -- what a kernel stores -- is inside the full bound
    assert bool(((got.float().to(torch.bfloat16).double() - r).abs() <= bound).all())
    # the bound is not slack beyond the format: the worst-case fp32 term (a few thousand u after two LayerNorms and three convolutions at +-20 logits)
    # stays a minor part of it, the bf16 rounding of r is the rest
    assert float((bound / (2.0 ** -8 * r.abs()).clamp_min(1e-30)).median()) < 1.25


@pytest.mark.parametrize("ci", range(len(pk.SPARSE_CASES)), ids=pk.SPARSE_IDS)
def test_token_bound_holds_for_fp32_reference_with_half_to_spare(ci):
    coords, labels, boxes, r, bound, E = pk.sparse_case(ci)
    with torch.no_grad():
        got = pk.sparse_tokens(pk.state(), coords, labels, boxes).double()         # fp32 matmul, sin, cos
    assert got.shape == r.shape == (pk.SPARSE_CASES[ci][0], pk.SPARSE_CASES[ci][1] + (2 if boxes is not None else 1), 256)
    err = (got - r).abs()
    exact = E == 0
    assert bool((err[exact] == 0).all())                                             # not_a_point rows: the vector alone
    ratio = float((err[~exact] / E[~exact]).max()) if bool((~exact).any()) else 0.0
    print(f"tokens {pk.SPARSE_IDS[ci]}: fp32 torch error / fp32 term {ratio:.3f}")
    assert ratio <= 0.5
    assert bool(((got.float().to(torch.bfloat16).double() - r).abs() <= bound).all())


def test_cases_cover_what_they_claim():
    for b in pk.DENSE_B:
        m = pk.dense_masks(b)
        assert float(m.abs().max()) > 19 and bool((m[:, :, :4, :4] == 0).all()) and bool((m[:, :, 252:, 252:] == 7.5).all())
    ns, labs, flat = set(), set(), []
    for ci, (b, n, bx) in enumerate(pk.SPARSE_CASES):
        coords, labels, boxes = pk.sparse_inputs(ci)
        ns.add((n, bx))
        if labels is not None:
            labs |= {tuple(sorted(set(row.tolist()))) for row in labels}
            flat += coords.flatten().tolist()
    assert {(0, True), (1, False), (2, False), (5, False), (1, True), (2, True), (5, True)} <= ns
    assert (-1, 0, 1) in labs                                                        # all three labels in one row
    assert 0.0 in flat and 1023.5 in flat and min(flat) < 0 and max(flat) > 1024
    assert {b for b, _, _ in pk.SPARSE_CASES} == {1, 2, 3}


# ------------------------------------------------------------------------------------------------ restatements == reference
def _tool():
    spec = importlib.util.spec_from_file_location("make_sam_prompts_golden", os.path.join(ROOT, "tools", "make_sam_prompts_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _restated():
    sd64 = pk.as_dtype(pk.state(), F64)
    tokens = []
    for ci in range(len(pk.SPARSE_CASES)):
        coords, labels, boxes = pk.sparse_inputs(ci)
        tokens.append(pk.sparse_tokens(sd64, None if coords is None else coords.double(), labels, None if boxes is None else boxes.double()))
    dense = pk.mask_downscaling(sd64, pk.dense_masks(2).double())
    return sd64, tokens, dense


def _decode_golden_prompt(sd64, dtype=F64):
    """the fixture's predict_torch call through the restatements + the decoder oracle (dense prompt handed over as emb + dense, no_mask_embed zeroed)"""
    g = pk.golden_prompt()
    sd = dict(pk.as_dtype(sd64, dtype))
    sparse = pk.sparse_tokens(sd, g["coords"].to(dtype), g["labels"], g["boxes"].to(dtype))
    dense = pk.mask_downscaling(sd, g["mask"].to(dtype))
    sd[pk.PE + "no_mask_embed.weight"] = torch.zeros_like(sd[pk.PE + "no_mask_embed.weight"])
    return osd.decode_masks(sd, pk.feats().to(dtype)[None] + dense, None, sparse=sparse, multimask_output=False)


def test_restatements_equal_the_imported_reference():
    if not os.path.isdir(os.path.join(rh.REF, "model", "segment_anything")):
        pytest.skip("the reference tree is absent")
    ref = _tool().reference_results()
    sd64, tokens, dense = _restated()
    with torch.no_grad():
        for ci, t in enumerate(tokens):
            assert t.shape == ref["tokens"][ci].shape
            assert float((t - ref["tokens"][ci]).abs().max()) <= 1e-12, pk.SPARSE_IDS[ci]
        cells = _rows(dense).reshape(2 * 4096, 256)[pk.golden_cells()]
        assert float((cells - ref["dense_cells"]).abs().max()) <= 1e-12
        for t in ref["transforms"]:
            assert np.abs(pk.apply_coords(t["coords"], t["size"]) - t["coords_out"]).max() <= 1e-12
            assert np.abs(pk.apply_boxes(t["boxes"], t["size"]) - t["boxes_out"]).max() <= 1e-12
        low, iou = _decode_golden_prompt(sd64)
        # the decoder oracle builds its positional encoding in fp32 (oracle/sam_decoder.py::dense_pe): this comparison is at that resolution
        assert float((low - ref["low_res"]).abs().max()) <= 1e-4 * max(1.0, float(ref["low_res"].abs().max()))
        assert float((iou - ref["iou"]).abs().max()) <= 1e-4


def test_restatements_equal_the_committed_fixture(golden):
    g = golden("sam_prompts.pt")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sam_prompts.pt")) < max(
        os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "sam_prompts.pt")
    sd64, tokens, dense = _restated()
    with torch.no_grad():
        for ci, t in enumerate(tokens):
            assert float((t - g["tokens"][ci]).abs().max()) <= 1e-12, pk.SPARSE_IDS[ci]
        assert torch.equal(g["cells"], pk.golden_cells())
        cells = _rows(dense).reshape(2 * 4096, 256)[g["cells"]]
        assert float((cells - g["dense_cells"].double()).abs().max()) <= 2.0 ** -24 * float(cells.abs().max())       # stored as fp32
        p, q = g["prompt"], pk.golden_prompt()
        assert all(torch.equal(p[k], q[k]) for k in p) and sorted(p) == ["boxes", "coords", "labels"]        # the mask prompt is seeded: pk.dense_masks(2)[:1]
        for t in g["transforms"]:
            size = tuple(int(v) for v in t["size"])
            assert np.abs(pk.apply_coords(t["coords"].numpy(), size) - t["coords_out"].numpy()).max() <= 1e-12
            assert np.abs(pk.apply_boxes(t["boxes"].numpy(), size) - t["boxes_out"].numpy()).max() <= 1e-12
        low, iou = _decode_golden_prompt(sd64)
        scale = max(1.0, float(g["low_res_sub"].abs().max()))
        assert float((low[:, :, ::2, ::2] - g["low_res_sub"].double()).abs().max()) <= 1e-4 * scale
        assert abs(float(low.sum() - g["low_res_sum"])) <= 1e-4 * scale * low.numel() ** 0.5
        assert float((iou - g["iou"]).abs().max()) <= 1e-4


def test_product_transforms_are_the_restated_ones():
    from llmseg_amd import predictor as hp
    for size in ((427, 640), (96, 72), (1365, 1024)):
        c = np.array([[0.0, 0.0], [size[1] - 1.0, size[0] - 1.0], [17.5, 3.25], [-4.0, 200.0]])
        bx = np.array([[3.0, 5.0, size[1] - 2.0, size[0] - 0.5], [10.0, 20.0, 30.0, 40.0]])
        assert np.array_equal(hp.apply_coords(c, size), pk.apply_coords(c, size))
        assert np.array_equal(hp.apply_boxes(bx, size), pk.apply_boxes(bx, size))
        assert np.array_equal(c, np.array([[0.0, 0.0], [size[1] - 1.0, size[0] - 1.0], [17.5, 3.25], [-4.0, 200.0]]))      # inputs are not modified


# ------------------------------------------------------------------------------------------------ layout
def test_nested_raster_permutation_round_trips():
    from llmseg_amd import predictor as hp
    from tests import amg_kernel_checks as ak
    m = torch.arange(2 * 3 * 65536, dtype=torch.float32).reshape(2, 3, 256, 256)
    n = hp.raster_to_nested(m)
    assert n.shape == (2, 3, 65536) and torch.equal(hp.nested_to_raster(n), m)
    assert torch.equal(n, pk.to_nested(m)) and torch.equal(pk.to_raster(n), m)
    assert np.array_equal(ak.to_nested(m[0].numpy()), n[0].numpy())                   # the order the post-processing kernels read
    # the kernel's statement of the layout: the 16 logits of cell p are contiguous at 16 p, sub-index (dy1 2 + dx1) 4 + dy2 2 + dx2
    for y, x, dy1, dx1, dy2, dx2 in ((0, 0, 0, 0, 0, 0), (63, 63, 1, 1, 1, 1), (5, 40, 1, 0, 0, 1), (17, 2, 0, 1, 1, 0)):
        Y, X = 4 * y + 2 * dy1 + dy2, 4 * x + 2 * dx1 + dx2
        assert float(n[1, 2, 16 * (y * 64 + x) + (dy1 * 2 + dx1) * 4 + dy2 * 2 + dx2]) == float(m[1, 2, Y, X])


# ------------------------------------------------------------------------------------------------ parameters
# tensors that LisaConfig(sam_decoder=True) adds under model.visual_model. on the parent commit (prompt encoder + mask decoder)
_PROMPT_ENCODER = ["pe_layer.positional_encoding_gaussian_matrix", "no_mask_embed.weight", "not_a_point_embed.weight"] + [f"point_embeddings.{i}.weight" for i in range(4)]


def _parent_decoder_keys():
    keys = ["prompt_encoder." + k for k in _PROMPT_ENCODER] + ["mask_decoder.iou_token.weight", "mask_decoder.mask_tokens.weight"]
    attn = lambda p: [f"{p}{n}.{w}" for n in ("q_proj", "k_proj", "v_proj", "out_proj") for w in ("weight", "bias")]
    t = "mask_decoder.transformer."
    for i in range(2):
        p = f"{t}layers.{i}."
        keys += attn(p + "self_attn.") + attn(p + "cross_attn_token_to_image.") + attn(p + "cross_attn_image_to_token.")
        keys += [f"{p}{n}.{w}" for n in ("norm1", "norm2", "norm3", "norm4", "mlp.lin1", "mlp.lin2") for w in ("weight", "bias")]
    keys += attn(t + "final_attn_token_to_image.") + [t + "norm_final_attn.weight", t + "norm_final_attn.bias"]
    keys += [f"mask_decoder.output_upscaling.{k}.{w}" for k in (0, 1, 3) for w in ("weight", "bias")]
    keys += [f"mask_decoder.output_hypernetworks_mlps.{i}.layers.{j}.{w}" for i in range(4) for j in range(3) for w in ("weight", "bias")]
    keys += [f"mask_decoder.iou_prediction_head.layers.{j}.{w}" for j in range(3) for w in ("weight", "bias")]
    return sorted(pk.PFX + k for k in keys)


def test_flag_off_leaves_the_key_set_alone_and_flag_on_adds_ten():
    from llmseg_amd import params
    assert sorted(params.sam_decoder_shapes()) == _parent_decoder_keys() == sorted(osd.decoder_shapes())
    assert len(_parent_decoder_keys()) == 127
    small = dict(llama=params.LlamaConfig(hidden=64, inter=128, layers=1, heads=2, vocab=40), clip=params.VitConfig(dim=32, layers=1, heads=2, mlp=64),
                 sam=params.SamConfig(dim=32, depth=1, heads=2, global_idx=(0,)), backbone="sam", build_unused_towers=False)
    base = params.lisa_shapes(params.LisaConfig(**small))
    off = params.lisa_shapes(params.LisaConfig(sam_decoder=True, **small))
    assert params.LisaConfig(**small).sam_prompts is False
    assert sorted(set(off) - set(base)) == _parent_decoder_keys()
    on = params.lisa_shapes(params.LisaConfig(sam_decoder=True, sam_prompts=True, **small))
    assert list(on)[:len(off)] == list(off) and all(on[k] == off[k] for k in off)
    extra = {k: on[k] for k in on if k not in off}
    assert extra == params.sam_prompt_shapes() == pk.prompt_shapes()
    assert not set(extra) & set(params.sam_decoder_shapes())


def test_flag_validation():
    from llmseg_amd import params
    with pytest.raises(ValueError, match="sam_decoder=True"):
        params.LisaConfig(sam_prompts=True)
    cfg = params.LisaConfig(backbone="sam", build_unused_towers=False)
    cfg.sam_prompts = True                                                            # set after construction: caught when the shapes are built
    with pytest.raises(ValueError, match="sam_decoder=True"):
        params.lisa_shapes(cfg)
    cfg.sam_decoder = True
    assert pk.MD + "6.weight" in params.lisa_shapes(cfg)


# ------------------------------------------------------------------------------------------------ loading (the HIP model has no CPU path: a stand-in holds its parameter tree)
class _Holder:
    def __init__(self, cfg):
        from llmseg_amd import params
        self.config, self.shapes = cfg, params.lisa_shapes(cfg)
        self.params = params.ParamTree(self.shapes, torch.device("cpu"), torch.bfloat16, params.fused_groups(cfg))
        for p in self.params.parameters():
            p.data.fill_(7.0)

    def _invalidate_derived(self):
        pass

    def state_dict(self):
        return {n: p.data for n, p in self.params.named_parameters()}

    def load_state_dict(self, sd, strict=True):
        own = dict(self.params.named_parameters())
        with torch.no_grad():
            for n, p in own.items():
                if n in sd:
                    p.copy_(sd[n].to(p.dtype))
        return [n for n in own if n not in sd], [n for n in sd if n not in own]


def _tiny_cfg(**kw):
    from llmseg_amd import params
    return params.LisaConfig(llama=params.LlamaConfig(hidden=32, inter=48, layers=1, heads=2, vocab=40), clip=params.VitConfig(dim=16, layers=1, heads=2, mlp=32, patch=14, img=28),
                             sam=params.SamConfig(img=64, patch=16, dim=32, depth=1, heads=2, window=2, global_idx=(0,), out_chans=256), backbone="sam",
                             build_unused_towers=False, **kw)


def test_sam_checkpoint_and_resume_carry_the_tensors_only_with_the_flag(tmp_path):
    import inspect
    from llmseg_amd import checkpoint, lisa, params, pretrained
    g = torch.Generator().manual_seed(5)
    cfg_on, cfg_off = _tiny_cfg(sam_decoder=True, sam_prompts=True), _tiny_cfg(sam_decoder=True)
    sam = {"image_encoder." + k: torch.randn(s, generator=g) for k, s in params.sam_shapes(cfg_on.sam, pfx="").items()}
    sam.update({k[len(pk.PFX):]: torch.randn(s, generator=g) for k, s in {**params.sam_decoder_shapes(), **params.sam_prompt_shapes()}.items()})
    f = str(tmp_path / "sam_vit_h_4b8939.pth")
    torch.save(sam, f)
    md_keys = sorted(k[len(pk.PFX):] for k in params.sam_prompt_shapes())
    on, off = _Holder(cfg_on), _Holder(cfg_off)
    rep_on, rep_off = pretrained.load_sam(on, f), pretrained.load_sam(off, f)
    assert sorted(rep_off["ignored"]) == md_keys and not rep_on["ignored"] and not rep_on["missing"] and not rep_off["missing"]      # flag off: dropped and reported, as before
    assert sorted(set(rep_on["loaded"]) - set(rep_off["loaded"])) == sorted(params.sam_prompt_shapes())
    for k in params.sam_prompt_shapes():
        assert torch.equal(on.params[k], sam[k[len(pk.PFX):]].to(torch.bfloat16)) and k not in off.params.flat
    for k in off.state_dict():
        assert torch.equal(off.params[k], on.params[k]), k                                                                       # every other tensor is the same
    # save -> resume in the reference's layout
    d = checkpoint.save_checkpoint(str(tmp_path / "ckpt"), on, global_step=3)
    blob = torch.load(f"{d}/mp_rank_00_model_states.pt", map_location="cpu", weights_only=True)["module"]
    assert all(checkpoint.PEFT_PREFIX + k in blob for k in params.sam_prompt_shapes())
    fresh_on, fresh_off = _Holder(cfg_on), _Holder(cfg_off)
    info_on, info_off = checkpoint.load_reference_checkpoint(fresh_on, str(tmp_path / "ckpt")), checkpoint.load_reference_checkpoint(fresh_off, str(tmp_path / "ckpt"))
    assert not info_on["missing"] and not info_on["ignored"] and sorted(info_off["ignored"]) == sorted(params.sam_prompt_shapes())
    assert all(torch.equal(fresh_on.params[k], on.params[k]) for k in on.state_dict())
    # from_pretrained hands the flag to the configuration
    assert inspect.signature(lisa.LISAForCausalLM.from_pretrained).parameters["sam_prompts"].default is False
    src = inspect.getsource(lisa.LISAForCausalLM.from_pretrained)
    assert "sam_prompts=sam_prompts" in src
