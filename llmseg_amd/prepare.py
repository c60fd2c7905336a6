"""Offline proposal preparation as a device stage: a directory of images in, the `masks.json` the training datasets read out.

    image file --segment.load_image--> uint8 [H, W, 3] --upload--> (longer side > --max_side: ops.image_resize_u8)
        --generate_masks (SAM everything mode)--> dense uint8 masks on the device
        --amg.to_records (llmseg_rle_encode: COCO RLE on the device, only the strings cross to the host)--> records
        --write_masks_json--> [{"image": file name, "target_size": [h, w], "masks": records}, ...]

This is the reference's prepare_datasets/prepare_ReasonSeg.py:32-97 followed by convert_h5_to_json.py: one JSON list with string `counts`,
what `SAM_Mask_Reader.read_mask_json` (here `targets.SamMaskReader`) loads.  There is no h5 intermediate: the JSON is what training reads.

Deviation from the reference: it shrinks an image whose longer side exceeds 1024 with cv2 `INTER_AREA` (prepare_ReasonSeg.py:32-40); here the
resize is the device's Pillow-BILINEAR kernel (`ops.image_resize_u8`, Pillow's `Image.resize` bit for bit) to the same `(int(W s), int(H s))`.
Pillow's BILINEAR widens its filter support when it shrinks, so it averages too, but the pixels are not cv2's: proposals of a resized image can
differ from the reference's files.  Images within `--max_side` are untouched and take the reference's route exactly.

    python -m llmseg_amd.prepare --image_dir images/ --out masks.json --version <LLaVA dir> --vision_pretrained sam_vit_h_4b8939.pth
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import amg, ops
from .segment import load_image

GENERATOR_FLAGS = (("points_per_side", int, 32), ("points_per_batch", int, 256), ("pred_iou_thresh", float, 0.88), ("stability_score_thresh", float, 0.95),
                   ("stability_score_offset", float, 1.0), ("box_nms_thresh", float, 0.7), ("crop_n_layers", int, 0), ("crop_nms_thresh", float, 0.7),
                   ("crop_overlap_ratio", float, 512 / 1500), ("crop_n_points_downscale_factor", int, 1), ("min_mask_region_area", int, 0))


def list_images(image_dir):
    """File names of `image_dir` that `load_image` reads -- `.npy` and every extension Pillow has a reader for -- sorted."""
    from PIL import Image
    types = (".npy",) + tuple(ext for ext, fmt in Image.registered_extensions().items() if fmt in Image.OPEN)
    return sorted(f for f in os.listdir(image_dir) if f.lower().endswith(types) and os.path.isfile(os.path.join(image_dir, f)))


def resize_to_max_side(image, max_side):
    """image uint8 [H, W, 3] on the device -> the same, or (longer side > max_side) resized to (int(H s), int(W s)), s = max_side / longer side
    (prepare_ReasonSeg.py:32-40, with the device's Pillow-BILINEAR resize in place of cv2 INTER_AREA)."""
    H, W = int(image.shape[0]), int(image.shape[1])
    if max(H, W) <= max_side:
        return image
    s = float(max_side) / max(H, W)
    return ops.image_resize_u8(image.contiguous(), int(H * s), int(W * s))


def prepare_image(model, image, max_side=1024, **generator_kwargs):
    """image uint8 [H, W, 3] on the device -> ((h, w) of the image the proposals live on, its records)."""
    image = resize_to_max_side(image, max_side).contiguous()
    h, w = int(image.shape[0]), int(image.shape[1])
    return (h, w), amg.to_records(model.generate_masks(image, **generator_kwargs), (h, w))


def write_masks_json(samples, path):
    """samples: [{"image": str, "target_size": [h, w], "masks": records with string `counts`}] -> one JSON file (convert_h5_to_json.py's output)."""
    for s in samples:
        assert set(s) >= {"image", "target_size", "masks"}, sorted(s)
        assert all(isinstance(m["segmentation"]["counts"], str) for m in s["masks"]), "masks.json stores the compressed counts as strings"
    with open(path, "w") as f:
        json.dump(samples, f)


def parse_args(argv=None):
    """-> (the flags of this tool, `run.parse_args` of everything else: the model-loading flags of the training driver)."""
    from . import run
    p = argparse.ArgumentParser(description="SAM everything-mode proposals for a directory of images (llmseg_amd): images -> masks.json",
                                epilog="Every other flag is a model-loading flag of llmseg_amd.run (--version, --vision_pretrained, --weight, ...).")
    p.add_argument("--image_dir", required=True, help="every .npy (uint8 [H, W, 3] RGB) and every image file Pillow reads in it, sorted by name")
    p.add_argument("--out", default="masks.json", help="where the JSON list of {image, target_size, masks} goes")
    p.add_argument("--max_side", default=1024, type=int, help="images whose longer side exceeds this are shrunk to it first")
    for name, typ, default in GENERATOR_FLAGS:
        p.add_argument("--" + name, default=default, type=typ, help="SamAutomaticMaskGenerator's argument of that name")
    args, rest = p.parse_known_args(argv)
    return args, run.parse_args(rest)


def main(argv=None, *, model=None, device=None):
    from . import checkpoint as ck
    from . import run
    from .lisa import LISAForCausalLM
    args, margs = parse_args(argv)
    device = torch.device("cuda", margs.local_rank) if device is None else torch.device(device)
    if model is None:
        tokenizer = run.init_tokenizer(margs)
        model = LISAForCausalLM.from_pretrained(
            margs.version, device=device, backbone="sam", lora_r=margs.lora_r, lora_alpha=margs.lora_alpha, lora_dropout=margs.lora_dropout,
            seed=margs.seed, vocab_size=len(tokenizer), seg_token_idx=run.seg_token_index(tokenizer), out_dim=margs.out_dim,
            vision_pretrained=margs.vision_pretrained or None, vision_tower=margs.vision_tower, use_mm_start_end=margs.use_mm_start_end,
            sam_decoder=True)
        if margs.weight:
            ck.load_reference_checkpoint(model, margs.weight)
    model.eval()
    kw = {name: getattr(args, name) for name, _, _ in GENERATOR_FLAGS}
    samples = []
    for name in list_images(args.image_dir):
        image = torch.from_numpy(np.array(load_image(os.path.join(args.image_dir, name)))).to(device)      # np.array: Pillow's buffer is read-only
        (h, w), recs = prepare_image(model, image, args.max_side, **kw)
        samples.append({"image": name, "target_size": [h, w], "masks": recs})
        print(f"{name}: {h} x {w}, {len(recs)} proposals")
    write_masks_json(samples, args.out)
    return samples


if __name__ == "__main__":
    main(sys.argv[1:])
