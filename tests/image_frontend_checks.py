"""The raw-image front end of inference (csrc/image.hip: BICUBIC resize, CLIP preprocessing, mask union; llmseg_amd/segment.py): restatements,
case lists and the GPU checks.

Restatements (numpy, CPU): Pillow's 8-bit BICUBIC `Image.resize` -- oracle/pil_resize.py's structure with `bicubic_filter` (Resample.c, a = -0.5,
support 2) -- pinned against `PIL.Image.resize` by tests/test_image_frontend_cpu.py, and `CLIPImageProcessor.preprocess` in float64 on top of it,
pinned there against transformers' processor."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)        # openai/clip-vit-large-patch14 preprocessor_config.json

# (h, w, out_h, out_w): up-scaling with support 2 and both edge clamps; odd sizes; the CLIP shapes; both passes skipped; one axis with 145 taps
RESIZE_CASES = [(8, 8, 224, 224), (37, 53, 224, 320), (225, 300, 224, 298), (300, 225, 298, 224), (427, 640, 224, 335), (113, 97, 260, 224),
                (224, 1000, 224, 1000), (224, 224, 224, 224), (1, 7, 3, 20), (3600, 8, 100, 8)]
# (h, w, S): landscape with an odd crop offset (335 -> left 55), portrait with an even one (298 -> top 37), square, a height / width that is S
# already (one pass skipped, window read in place), up-scaling, and the same at a tiny configuration's S
CLIP_CASES = [(427, 640, 224), (300, 225, 224), (256, 256, 224), (224, 1000, 224), (500, 224, 224), (224, 224, 224), (37, 53, 224),
              (427, 640, 28), (61, 45, 28), (97, 97, 28)]


def bicubic_filter(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """-> (xmin int32 [out], count int32 [out], k int32 [out, ksize]) of Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` for BICUBIC."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int32); cnt = np.zeros(out_size, np.int32); kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        w = [bicubic_filter((x + lo - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], cnt[xx] = lo, n
        kk[xx, :n] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return xmin, cnt, kk


def _pass(img, out_size, axis):
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    xmin, cnt, kk = coeffs(src.shape[0], out_size)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        n = int(cnt[xx])
        acc = np.tensordot(kk[xx, :n].astype(np.int64), src[xmin[xx]:xmin[xx] + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bicubic_u8(img, out_h, out_w):
    """img uint8 [H, W, C] -> uint8 [out_h, out_w, C], bit-identical to `np.array(PIL.Image.fromarray(img).resize((out_w, out_h), BICUBIC))`."""
    h, w = img.shape[:2]
    x = img
    if out_w != w:
        x = _pass(x, out_w, 1)
    if out_h != h:
        x = _pass(x, out_h, 0)
    return x if x is not img else img.copy()


def clip_resized_size(h, w, size):
    """transformers `get_resize_output_image_size(image, size, default_to_square=False)`."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def clip_window(img, size):
    """uint8 [size, size, 3]: the processor's resize + centre crop."""
    nh, nw = clip_resized_size(img.shape[0], img.shape[1], size)
    rs = resize_bicubic_u8(img, nh, nw)
    top, left = (nh - size) // 2, (nw - size) // 2
    return rs[top:top + size, left:left + size]


def clip_preprocess_f64(img, size, mean=CLIP_MEAN, std=CLIP_STD):
    """`CLIPImageProcessor.preprocess` in float64: -> [3, size, size]."""
    x = clip_window(img, size).astype(np.float64) * (1.0 / 255.0)
    x = (x - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def block_image(h, w, axis, block=5):
    """0 / 255 steps along `axis`: the negative lobes overshoot below 0 and above 255 at every edge."""
    idx = (np.arange(h)[:, None] if axis == 0 else np.arange(w)[None, :]) // block
    return np.ascontiguousarray(np.broadcast_to(((idx % 2) * 255).astype(np.uint8)[..., None], (h, w, 3)))


# ---------------------------------------------------------------- GPU checks: lists of (name, error, bound) ----------------------------------------------------------------
DEV = "cuda"


def check_bicubic():
    import torch
    from llmseg_amd import ops
    res = []
    for n, (h, w, oh, ow) in enumerate(RESIZE_CASES):
        a = random_image(h, w, 100 + n)
        got = ops.image_resize_u8(torch.as_tensor(a).to(DEV), oh, ow, resample="bicubic").cpu().numpy()
        res.append((f"bicubic {h}x{w} -> {oh}x{ow} (bytes that differ)", float((got != resize_bicubic_u8(a, oh, ow)).sum()), 0.0))
    big = random_image(300, 400, 7)
    x0, y0, x1, y1 = 149, 99, 400, 300
    got = ops.image_resize_u8(torch.as_tensor(big).to(DEV), 224, 279, (x0, y0, x1, y1), resample="bicubic").cpu().numpy()
    res.append(("bicubic on a crop_box window (bytes that differ)", float((got != resize_bicubic_u8(big[y0:y1, x0:x1], 224, 279)).sum()), 0.0))
    for axis, (oh, ow) in ((0, (224, 150)), (1, (97, 224)), (0, (31, 40)), (1, (31, 40))):
        a = block_image(90, 120, axis)
        got = ops.image_resize_u8(torch.as_tensor(a).to(DEV), oh, ow, resample="bicubic").cpu().numpy()
        ref = resize_bicubic_u8(a, oh, ow)
        assert ref.min() == 0 and ref.max() == 255
        res.append((f"bicubic 0/255 blocks along axis {axis} -> {oh}x{ow} (bytes that differ)", float((got != ref).sum()), 0.0))
    try:
        from PIL import Image
        a = random_image(427, 640, 11)
        ref = np.array(Image.fromarray(a).resize((335, 224), Image.BICUBIC))
        got = ops.image_resize_u8(torch.as_tensor(a).to(DEV), 224, 335, resample="bicubic").cpu().numpy()
        res.append(("bicubic == PIL.Image.resize itself (bytes that differ)", float((got != ref).sum()), 0.0))
    except ImportError:
        pass
    return res


def check_bilinear_route():
    """resample="bilinear" is the existing entry point: same bits through the keyword, the default and the filter argument of the C ABI."""
    import torch
    from llmseg_amd import _lib, ops
    res = []
    lib = _lib.load()
    for n, (h, w, oh, ow) in enumerate([(333, 517, 100, 91), (1, 7, 3, 20), (50, 50, 50, 80), (240, 320, 1024, 768)]):
        a = torch.as_tensor(random_image(h, w, 200 + n)).to(DEV)
        ref = ops.image_resize_u8(a, oh, ow)
        nb = lib.llmseg_image_resize_filter_workspace(h, w, oh, ow, 3, 0)
        assert nb == lib.llmseg_image_resize_workspace(h, w, oh, ow, 3)
        ws = torch.empty((nb,), device=DEV, dtype=torch.uint8)
        out = torch.empty_like(ref)
        _lib.check(lib.llmseg_image_resize_u8_filter(a.data_ptr(), w * 3, out.data_ptr(), h, w, oh, ow, 3, 0, ws.data_ptr(), nb, ops._stream()), "resize")
        bad = int((ops.image_resize_u8(a, oh, ow, resample="bilinear") != ref).sum()) + int((out != ref).sum())
        res.append((f"bilinear route {h}x{w} -> {oh}x{ow} (bytes that differ from llmseg_image_resize_u8)", float(bad), 0.0))
    return res


def clip_bound():
    """|v| < 4 for every normalised value ((0 - 0.48) / 0.26 = -1.8 .. (1 - 0.41) / 0.26 = 2.3), where bf16 (8 significant bits) is spaced 2^-6 apart at
    most: half a spacing for the one rounding to bf16, plus 1e-6 for the fp32 steps in front of it (three roundings at |v| < 4: 3 * 2^-22 = 7e-7)."""
    return 2.0 ** -7 + 1e-6


def check_clip_preprocess():
    import torch
    from llmseg_amd import ops
    res = []
    mean32, std32 = torch.tensor(CLIP_MEAN, dtype=torch.float32).view(3, 1, 1), torch.tensor(CLIP_STD, dtype=torch.float32).view(3, 1, 1)
    for n, (h, w, S) in enumerate(CLIP_CASES):
        a = random_image(h, w, 300 + n)
        d = torch.as_tensor(a).to(DEV)
        got = ops.clip_preprocess(d, S, CLIP_MEAN, CLIP_STD)
        assert got.shape == (1, 3, S, S) and got.dtype == torch.bfloat16
        ref = clip_preprocess_f64(a, S)
        assert np.abs(ref).max() < 4.0
        res.append((f"clip_preprocess {h}x{w} -> {S} vs float64", float(np.abs(got[0].double().cpu().numpy() - ref).max()), clip_bound()))
        # resize fully on the device, crop, normalise with the same fp32 formula: the windowed resampling must not have skipped anything
        nh, nw = ops.clip_resized_size(h, w, S)
        top, left = ops.clip_crop_origin(nh, nw, S)
        full = ops.image_resize_u8(d, nh, nw, resample="bicubic").cpu()[top:top + S, left:left + S]
        r = (full.permute(2, 0, 1).double() * (1.0 / 255.0)).float()
        chained = ((r - mean32) / std32).to(torch.bfloat16)
        res.append((f"clip_preprocess {h}x{w} -> {S} == normalise(crop(resize)) (elements that differ)",
                    float((got[0].cpu().view(torch.int16) != chained.view(torch.int16)).sum()), 0.0))
    return res


def check_mask_union():
    import torch
    from llmseg_amd import ops
    g = torch.Generator().manual_seed(9)
    res = []
    for (K, h, w) in ((12, 97, 130), (5, 64, 48), (3, 1, 7)):                       # a width / area that is no multiple of 16; an aligned one; less than one chunk
        masks = (torch.rand((K, h, w), generator=g) > 0.8).to(torch.uint8) * torch.randint(1, 256, (K, 1, 1), generator=g).to(torch.uint8)    # non-zero, not only 1
        masks[0] = 0
        sel = torch.zeros((3, K), dtype=torch.uint8)
        sel[1] = 1
        sel[2] = (torch.rand((K,), generator=g) > 0.5).to(torch.uint8)
        rows = {"none / all / random": sel, "one": torch.eye(K, dtype=torch.uint8)[[K - 1, 0, 1]]}
        for name, s in rows.items():
            got = ops.mask_union(masks.to(DEV), s.to(DEV)).cpu()
            ref = torch.stack([masks[s[c].bool()].any(0) if s[c].any() else torch.zeros((h, w), dtype=torch.bool) for c in range(s.shape[0])]).to(torch.uint8)
            res.append((f"mask_union K={K} {h}x{w}, selections {name} (pixels that differ)", float((got != ref).sum()), 0.0))
        got1 = ops.mask_union(masks.to(DEV), sel[2].to(DEV)).cpu()
        res.append((f"mask_union K={K} {h}x{w}, one selection row as a vector", float((got1 != masks[sel[2].bool()].any(0).to(torch.uint8)).sum()) if sel[2].any() else float(got1.sum()), 0.0))
    return res


_MODEL = {}


def tiny_model():
    """The suite's tiny SAM-backbone model (tests/sam_decoder_checks.py::_model), built once per process."""
    if "m" not in _MODEL:
        from tests import sam_decoder_checks as sc
        _MODEL["m"] = sc._model()[0]
    return _MODEL["m"]


def check_prepare_image():
    import torch
    from llmseg_amd import amg, ops
    from oracle import amg as oamg
    m = tiny_model()
    a = random_image(201, 251, 5)
    d = torch.as_tensor(a).to(DEV)
    p = m.prepare_image(d)
    S, c = m.config.sam.img, m.config.clip.img
    nh, nw = oamg.preprocess_shape(201, 251, S)
    ok = p["resize"] == (nh, nw) and p["original_size"] == (201, 251) and p["images"].shape == (1, 3, S, S) and p["images_clip"].shape == (1, 3, c, c)
    ref = ops.sam_preprocess(ops.image_resize_u8(d, nh, nw), S, amg.PIXEL_MEAN, amg.PIXEL_STD)
    return [("prepare_image: resize / original_size / shapes", 0.0 if ok else 1.0, 0.0),
            ("prepare_image: images == sam_preprocess(image_resize_u8)", float((p["images"].view(torch.int16) != ref.view(torch.int16)).sum()), 0.0),
            ("prepare_image: images_clip == clip_preprocess", float((p["images_clip"].view(torch.int16) != ops.clip_preprocess(d, c, CLIP_MEAN, CLIP_STD).view(torch.int16)).sum()), 0.0)]


SENTENCES = ["the thing that matters ", "what the person would sit on"]
MODES = ("argmax", "threshold", "iou_iop", "top5")


def blob_proposals(H, W, K=12):
    """K rectangles of distinct areas (two pairs overlap), one of them empty: uint8 [K, H, W]."""
    import torch
    masks = torch.zeros((K, H, W), dtype=torch.uint8)
    for k in range(1, K):
        y0, x0 = (7 * k) % (H // 2), (11 * k) % (W // 2)
        masks[k, y0:y0 + 4 + 3 * k, x0:x0 + 5 + 2 * k] = 1
    return masks


def rule(mode, sim, iou, threshold):
    """The four selection rules of the reference's validation loops (training.py:627-634, 712-718, 872-967, 969-1078) in torch: sim, iou [K] -> uint8 [K]."""
    import torch
    if mode == "argmax":
        sel = torch.zeros_like(sim, dtype=torch.uint8)
        sel[torch.argmax(sim)] = 1
    elif mode == "threshold":
        sel = (iou > threshold).to(torch.uint8)
    elif mode == "iou_iop":
        sel = (iou > threshold).to(torch.uint8)
        sel[torch.argmax(sim)] = 1
    else:
        idx = torch.topk(sim, min(5, sim.shape[-1]), dim=0).indices
        sel = torch.zeros_like(iou, dtype=torch.uint8)
        sel[idx] = (iou[idx] > threshold).to(torch.uint8)
    return sel


def hand_chain(m, d_img, masks, areas, tok, top=50):
    """The public calls `segment` chains, one by one, with `model_forward` encoding the image itself: -> (segs_origin, [(sim [K], iou [K]) per sentence])."""
    from llmseg_amd import collate, targets
    p = m.prepare_image(d_img)
    t = targets.proposals_and_targets_dense(masks, areas, [], top=top, want_origin=True)
    scores = []
    for s in SENTENCES:
        sample = collate.inference_sample(p["images"][0], p["images_clip"][0], [s], t, p["original_size"], resize=p["resize"])
        col = collate.dict_to_cuda(collate.collate_fn_new([sample], tokenizer=tok), device=DEV)
        out = m.model_forward(**collate.model_kwargs(col))
        scores.append((out["pred_similarity"][0][0], out["pred_iou"][0][0]))
    return t["segs_origin"], scores


def _median_threshold(scores):
    """A threshold that splits the first sentence's predicted IoUs (the tiny random model's scores sit in a narrow band, 0.5 would select all or none)."""
    import torch
    v = torch.sort(scores[0][1].float().cpu()).values
    return float((v[len(v) // 2 - 1] + v[len(v) // 2]) / 2)


def _compare(tag, got, segs, scores, mode, thr):
    import torch
    res = []
    sel = torch.stack([rule(mode, sim, iou, thr) for sim, iou in scores])
    exp = torch.stack([segs[s.bool()].any(0) if bool(s.any()) else torch.zeros_like(segs[0], dtype=torch.bool) for s in sel]).to(torch.uint8)
    res.append((f"{tag} [{mode}]: selected proposals that differ", float((got["selected"] != sel).sum()), 0.0))
    res.append((f"{tag} [{mode}]: mask pixels that differ", float((got["masks"] != exp).sum()), 0.0))
    bits = lambda a: a.contiguous().view(torch.int32)
    res.append((f"{tag} [{mode}]: pred_iou / pred_similarity bits that differ",
                float((bits(got["pred_iou"]) != bits(torch.stack([i for _, i in scores]))).sum() + (bits(got["pred_similarity"]) != bits(torch.stack([s for s, _ in scores]))).sum()), 0.0))
    return res


def check_segment_given_proposals():
    """(i) synthetic dense proposals, all four modes; (iii) the records list they encode to; (iv) K = 0."""
    import torch
    from llmseg_amd import amg
    from oracle.stub_tokenizer import StubTokenizer
    m, tok = tiny_model(), StubTokenizer()
    H, W = 201, 251
    d_img = torch.as_tensor(random_image(H, W, 5)).to(DEV)
    masks = blob_proposals(H, W).to(DEV)
    areas = masks.flatten(1).sum(1)
    segs, scores = hand_chain(m, d_img, masks, areas, tok)
    thr = _median_threshold(scores)
    res = [("segment: the threshold splits the proposals", 0.0 if 0 < int(rule("threshold", *scores[0], thr).sum()) < masks.shape[0] else 1.0, 0.0)]
    for mode in MODES:
        got = m.segment(d_img, SENTENCES, tok, mode=mode, threshold=thr, proposals=masks)
        assert got["masks"].shape == (2, H, W) and got["masks"].dtype == torch.uint8 and got["selected"].shape == (2, masks.shape[0])
        res += _compare("segment(proposals=dense)", got, segs, scores, mode, thr)
        res.append((f"segment(proposals=dense) [{mode}]: proposals returned", float((got["proposals"] != segs).sum()), 0.0))
    dense = m.segment(d_img, SENTENCES, tok, mode="iou_iop", threshold=thr, proposals=masks)
    recs = amg.to_records(dict(masks=masks, boxes=torch.zeros((masks.shape[0], 4), dtype=torch.int64), areas=areas, iou_preds=torch.zeros(masks.shape[0]),
                               stability_score=torch.zeros(masks.shape[0]), points=torch.zeros((masks.shape[0], 2), dtype=torch.float64)), (H, W))
    rec = m.segment(d_img, SENTENCES, tok, mode="iou_iop", threshold=thr, proposals=recs)
    res.append(("segment(proposals=records) == segment(proposals=dense): mask pixels that differ", float((rec["masks"] != dense["masks"]).sum()), 0.0))
    res.append(("segment(proposals=records) == segment(proposals=dense): selections that differ", float((rec["selected"] != dense["selected"]).sum()), 0.0))
    empty = m.segment(d_img, SENTENCES, tok, proposals=masks[:0])
    ok = (empty["masks"].shape == (2, H, W) and int(empty["masks"].sum()) == 0 and empty["selected"].shape == (2, 0) and empty["pred_iou"].shape == (2, 0)
          and empty["pred_similarity"].shape == (2, 0))
    res.append(("segment with K = 0: zero masks, empty scores", 0.0 if ok else 1.0, 0.0))
    return res


def check_segment_generated():
    """(ii) proposals=None: SAM everything mode inside `segment` against hand-chained `generate_masks`; one shared ViT embedding against
    `model_forward` encoding the image itself (the hand chain)."""
    import torch
    from oracle import cases
    from oracle.stub_tokenizer import StubTokenizer
    m, tok = tiny_model(), StubTokenizer()
    d_img = torch.as_tensor(cases.amg_image_case()).to(DEV)
    kw = dict(points_per_side=8, points_per_batch=24, **cases.amg_thresholds())
    gen = m.generate_masks(d_img, **kw)
    res = [("segment(proposals=None): the generator yields proposals", 0.0 if gen["masks"].shape[0] > 0 else 1.0, 0.0)]
    segs, scores = hand_chain(m, d_img, gen["masks"], gen["areas"], tok)
    thr = _median_threshold(scores)
    for mode in ("threshold", "argmax"):
        got = m.segment(d_img, SENTENCES, tok, mode=mode, threshold=thr, **kw)
        res += _compare("segment(proposals=None)", got, segs, scores, mode, thr)
    return res


def check_segment_needs_sam():
    import pytest
    import torch
    from llmseg_amd import lisa as hip_lisa
    from oracle import cases
    from oracle.stub_tokenizer import StubTokenizer
    from tests import model_checks as mc
    m = hip_lisa.LISAForCausalLM(mc.to_hip_cfg(cases.tiny_lisa_cfg("dinov2")), device=DEV).init_random(seed=1)
    d_img = torch.as_tensor(random_image(40, 56, 5)).to(DEV)
    with pytest.raises(ValueError, match="proposals"):
        m.segment(d_img, SENTENCES, StubTokenizer())
    with pytest.raises(ValueError, match="mode"):
        m.segment(d_img, SENTENCES, StubTokenizer(), mode="best", proposals=blob_proposals(40, 56).to(DEV))
    return [("segment without proposals on a non-SAM backbone raises", 0.0, 0.0)]
