"""Raw-image inference: a picture and sentences in, one mask per sentence out (`SegmentMixin.segment`), over the pieces the path already has.

    image uint8 [H, W, 3] --prepare_image--> images (backbone frame) + images_clip
        --generate_masks (SAM everything mode) | the caller's proposals--> masks uint8 [K, H, W]
        --targets.proposals_and_targets_dense--> the 256 x 256 proposal maps
        --collate.inference_sample -> collate_fn_new -> dict_to_cuda--> the prompt of the validation datasets
        --model_forward(inference=True), one conversation at a time--> predicted IoU / similarity per proposal
        --one of the four selection rules of the validation loops--> select uint8 [C, K] --ops.mask_union--> masks uint8 [C, H, W]

The image front end is on the device: `ResizeLongestSide.apply_image` + the datasets' `preprocess` (utils/llm_seg_dataset.py:100-110,183) are
`llmseg_image_resize_u8` + `llmseg_sam_preprocess`, `CLIPImageProcessor.preprocess` (:127) is `llmseg_clip_preprocess`.  Only decoding the
file stays on the host (`load_image`, used by the command line below).

The frozen towers run ONCE per image: the backbone's embedding feeds the proposal generator and, through `tower_visual=`, every
`model_forward`; the CLIP tokens go in through `tower_clip=`.  The forward itself runs once per sentence, the shape of the reference's validation
loops (one image, one conversation): with several conversations the reference's inference branch scores the predicted IoU of the first one only
(LISA.py:394-403), which would leave every later sentence without its `threshold` rule.

    python -m llmseg_amd.segment --image photo.jpg --query "the thing to sit on" --out masks.npy --version <LLaVA dir> --vision_pretrained sam_vit_h_4b8939.pth
"""
import argparse
import sys

import numpy as np
import torch

from . import amg, collate, ops, targets

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # openai/clip-vit-large-patch14 preprocessor_config.json
MODES = ("argmax", "threshold", "iou_iop", "top5")
TOP_SIMILAR = 5                                                   # `validate_threshold_from_topIoU` (training.py:969-1078)


def select_proposals(mode, similarity, pred_iou, threshold=0.5):
    """similarity, pred_iou fp32 [K] -> uint8 [K]: which proposals form the prediction, by the rule of the reference's validation loop --
    "argmax": `validate` (training.py:627-634), "threshold": `validate_threshold` (:712-718), "iou_iop": `validate_iou_iop` (:872-967),
    "top5": `validate_threshold_from_topIoU` (:969-1078).  The same proposals `llmseg_amd.validate`'s loops select."""
    if mode == "argmax":
        select = torch.zeros_like(similarity, dtype=torch.uint8)
        select[torch.argmax(similarity)] = 1
    elif mode == "threshold":
        select = (pred_iou > threshold).to(torch.uint8)
    elif mode == "iou_iop":
        select = (pred_iou > threshold).to(torch.uint8)
        select[torch.argmax(similarity)] = 1
    elif mode == "top5":
        idx = torch.topk(similarity, min(TOP_SIMILAR, similarity.shape[-1]), dim=0).indices
        select = torch.zeros_like(pred_iou, dtype=torch.uint8)
        select[idx] = (pred_iou[idx] > threshold).to(torch.uint8)
    else:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    return select


class SegmentMixin:
    def backbone_frame(self):
        """Side of the segmentation backbone's square input: SAM's image size, or the DINOv2 input size of the config."""
        c = self.config
        return c.sam.img if c.backbone == "sam" else c.dino.img

    @torch.no_grad()
    def prepare_image(self, image_u8):
        """image uint8 [H, W, 3] (RGB, on the device) -> dict(images bf16 [1, 3, S, S], images_clip bf16 [1, 3, c, c], resize (nh, nw),
        original_size (H, W)) as the reference's datasets prepare them (utils/llm_seg_dataset.py:127,183,100-110)."""
        assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.shape[2] == 3 and image_u8.is_cuda, "image: uint8 [H, W, 3] on the device"
        image_u8 = image_u8.contiguous()
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        S = self.backbone_frame()
        nh, nw = amg.preprocess_shape(H, W, S)
        images = ops.sam_preprocess(ops.image_resize_u8(image_u8, nh, nw), S, amg.PIXEL_MEAN, amg.PIXEL_STD)
        images_clip = ops.clip_preprocess(image_u8, self.config.clip.img, CLIP_MEAN, CLIP_STD)
        return {"images": images, "images_clip": images_clip, "resize": (nh, nw), "original_size": (H, W)}

    @torch.no_grad()
    def segment(self, image_u8, sentences, tokenizer, is_sentence=True, mode="threshold", threshold=0.5, top=50, proposals=None, **amg_kwargs):
        """image uint8 [H, W, 3] on the device + C sentences -> dict(masks uint8 [C, H, W], selected uint8 [C, K], pred_iou fp32 [C, K],
        pred_similarity fp32 [C, K], proposals uint8 [K, H, W] -- the `top` largest, by area).
        proposals: None = SAM everything mode on this image (`generate_masks(**amg_kwargs)`; SAM backbone only), device masks uint8 [K, H, W],
        or the records list of `amg.to_records` / the reference's preparation scripts.  mode: see `select_proposals`."""
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if proposals is None and self.config.backbone != "sam":
            raise ValueError(f"segment(proposals=None) generates proposals with SAM, but this model's backbone is {self.config.backbone!r}: pass proposals= "
                             "(device masks uint8 [K, H, W] or a records list)")
        sentences = list(sentences)
        C = len(sentences)
        p = self.prepare_image(image_u8)
        H, W = p["original_size"]
        dev = image_u8.device

        def result(segs, selected, iou, sim):
            return {"masks": ops.mask_union(segs, selected) if segs.shape[0] else torch.zeros((C, H, W), device=dev, dtype=torch.uint8),
                    "selected": selected, "pred_iou": iou, "pred_similarity": sim, "proposals": segs}

        def empty():
            z = torch.zeros((C, 0), device=dev, dtype=torch.float32)
            return result(torch.zeros((0, H, W), device=dev, dtype=torch.uint8), z.to(torch.uint8), z, z.clone())

        if C == 0 or (proposals is not None and len(proposals) == 0):
            return empty()
        tower_visual, tower_clip = self.encode_towers(p["images"], p["images_clip"])
        if proposals is None:
            def encode(img, cb):                                   # the whole image's embedding is the one above; deeper crop layers embed their window
                if tuple(cb) == (0, 0, W, H):
                    return tower_visual, p["resize"], p["original_size"]
                return self.set_image(img, cb)
            gen = self.generate_masks(image_u8.contiguous(), encode=encode, **amg_kwargs)
            if gen["masks"].shape[0] == 0:
                return empty()
            t = targets.proposals_and_targets_dense(gen["masks"], gen["areas"], [], top=top, want_origin=True)
        elif torch.is_tensor(proposals):
            assert proposals.dtype == torch.uint8 and proposals.dim() == 3 and tuple(proposals.shape[1:]) == (H, W) and proposals.is_cuda, \
                "proposals: uint8 [K, H, W] on the device, at the image's size"
            masks = proposals.contiguous()
            t = targets.proposals_and_targets_dense(masks, (masks != 0).flatten(1).sum(1), [], top=top, want_origin=True)
        else:
            t = targets.proposals_and_targets(list(proposals), [], dev, top=top)
            assert tuple(t["segs_origin"].shape[1:]) == (H, W), "proposal records of another image size"
        sims, ious, selected = [], [], []
        for s in sentences:
            sample = collate.inference_sample(p["images"][0], p["images_clip"][0], [s], t, (H, W), is_sentence=is_sentence, resize=p["resize"])
            col = collate.dict_to_cuda(collate.collate_fn_new([sample], tokenizer=tokenizer, use_mm_start_end=self.use_mm_start_end), device=dev)
            out = self.model_forward(**collate.model_kwargs(col), tower_visual=tower_visual, tower_clip=tower_clip)
            sims.append(out["pred_similarity"][0][0])
            ious.append(out["pred_iou"][0][0])
            selected.append(select_proposals(mode, sims[-1], ious[-1], threshold))
        return result(t["segs_origin"], torch.stack(selected), torch.stack(ious), torch.stack(sims))


# ---------------------------------------------------------------------------------------------------------------- command line
def load_image(path):
    """-> uint8 [H, W, 3] RGB array: a `.npy` file as it is, anything else through Pillow (imported only then)."""
    if str(path).endswith(".npy"):
        a = np.load(path)
    else:
        from PIL import Image
        a = np.asarray(Image.open(path).convert("RGB"))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{path}: expected a uint8 [H, W, 3] RGB image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def parse_args(argv=None):
    """-> (the flags of this tool, `run.parse_args` of everything else: the model-loading flags of the training driver)."""
    from . import run
    p = argparse.ArgumentParser(description="LLM-Seg inference on one image (llmseg_amd): image + queries -> masks",
                                epilog="Every other flag is a model-loading flag of llmseg_amd.run (--version, --vision_pretrained, --vision_tower, --backbone, --weight, ...).")
    p.add_argument("--image", required=True, help="a .npy file (uint8 [H, W, 3] RGB) or any file Pillow reads")
    p.add_argument("--query", action="append", required=True, help="a sentence to segment; repeat for several masks")
    p.add_argument("--mode", default="threshold", choices=MODES)
    p.add_argument("--threshold", default=0.5, type=float)
    p.add_argument("--phrase", action="store_true", default=False, help='the queries are short phrases ("What is {} in this image?")')
    p.add_argument("--out", default="masks.npy", help="where the uint8 [n_queries, H, W] masks go")
    args, rest = p.parse_known_args(argv)
    return args, run.parse_args(rest)


def main(argv=None, *, model=None, tokenizer=None, device=None):
    from . import checkpoint as ck
    from . import run
    from .lisa import LISAForCausalLM
    args, margs = parse_args(argv)
    device = torch.device("cuda", margs.local_rank) if device is None else torch.device(device)
    if tokenizer is None:
        tokenizer = run.init_tokenizer(margs)
    if model is None:
        model = LISAForCausalLM.from_pretrained(
            margs.version, device=device, backbone=margs.backbone, lora_r=margs.lora_r, lora_alpha=margs.lora_alpha, lora_dropout=margs.lora_dropout,
            seed=margs.seed, vocab_size=len(tokenizer), seg_token_idx=run.seg_token_index(tokenizer), out_dim=margs.out_dim,
            vision_pretrained=margs.vision_pretrained or None, vision_tower=margs.vision_tower, use_mm_start_end=margs.use_mm_start_end,
            sam_decoder=margs.backbone == "sam")
        if margs.weight:
            ck.load_reference_checkpoint(model, margs.weight)
    model.eval()
    image = torch.as_tensor(load_image(args.image)).to(device)
    out = model.segment(image, args.query, tokenizer, is_sentence=not args.phrase, mode=args.mode, threshold=args.threshold)
    np.save(args.out, out["masks"].cpu().numpy())
    for q, m, s in zip(args.query, out["masks"], out["selected"]):
        print(f"{q!r}: {int(s.sum())} of {s.numel()} proposals, {int(m.sum())} pixels")
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
