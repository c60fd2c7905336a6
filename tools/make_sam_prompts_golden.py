"""Write tests/golden/sam_prompts.pt by running the IMPORTED reference (build container only: needs the reference tree that `oracle.ref_harness` points at;
`python tools/make_sam_prompts_golden.py`).  The reference's `PromptEncoder`, `MaskDecoder`, `SamPredictor` and `ResizeLongestSide` are imported, cast to
double and driven with the seeded cases of tests/predictor_checks.py; the fixture holds data only: the prompt inputs, the sparse tokens of every case, the
dense embedding at 512 seeded cells, and `low_res` / `iou` of one `predict_torch` call.  `reference_results()` is also what tests/test_predictor_cpu.py
compares the fp64 restatements with when the reference tree is present."""
import functools
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402
from tests import predictor_checks as pk  # noqa: E402

INPUT_SIZE, ORIGINAL_SIZE = (683, 1024), (427, 640)


def reference_modules():
    """The reference's prompt encoder / mask decoder in fp64 with the seeded state, and a `SamPredictor` whose image embedding is set by hand."""
    rh.setup()
    from model.segment_anything.modeling import MaskDecoder, PromptEncoder, TwoWayTransformer
    from model.segment_anything.modeling.sam import Sam
    from model.segment_anything.predictor import SamPredictor
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16)
    md = MaskDecoder(num_multimask_outputs=3, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                     transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    sd = pk.state()
    pe.load_state_dict({k[len(pk.PE):]: v for k, v in sd.items() if k.startswith(pk.PE)}, strict=True)
    md.load_state_dict({k[len(pk.PFX + "mask_decoder."):]: v for k, v in sd.items() if ".mask_decoder." in k}, strict=True)
    pe, md = pe.double().eval(), md.double().eval()
    enc = types.SimpleNamespace(img_size=1024)
    # the reference's predictor calls its prompt encoder without the `text_embeds` argument its own PromptEncoder.forward requires: supply None
    with_none = lambda points, boxes, masks: pe(points=points, boxes=boxes, masks=masks, text_embeds=None)
    model = types.SimpleNamespace(image_encoder=enc, prompt_encoder=with_none, mask_decoder=md, mask_threshold=0.0, image_format="RGB", device=torch.device("cpu"))
    with_none.get_dense_pe = pe.get_dense_pe
    model.postprocess_masks = functools.partial(Sam.postprocess_masks, types.SimpleNamespace(image_encoder=enc))
    pred = SamPredictor(model)
    pred.features = pk.feats().double()[None]
    pred.input_size, pred.original_size, pred.is_image_set = INPUT_SIZE, ORIGINAL_SIZE, True
    return pe, md, pred


@torch.no_grad()
def reference_results():
    pe, md, pred = reference_modules()
    out = {"tokens": [], "input_size": INPUT_SIZE, "original_size": ORIGINAL_SIZE}
    for ci in range(len(pk.SPARSE_CASES)):
        coords, labels, boxes = pk.sparse_inputs(ci)
        pts = None if coords is None else (coords.double(), labels)
        sparse, _ = pe(points=pts, boxes=None if boxes is None else boxes.double(), masks=None, text_embeds=None)
        out["tokens"].append(sparse.clone())
    dense = pe._embed_masks(pk.dense_masks(2).double())                                   # [2, 256, 64, 64]
    out["dense_cells"] = dense.flatten(2).permute(0, 2, 1).reshape(2 * 4096, 256)[pk.golden_cells()].clone()
    g = pk.golden_prompt()
    out["prompt"] = g
    masks, iou, low = pred.predict_torch(g["coords"].double(), g["labels"], g["boxes"].double(), g["mask"].double(), multimask_output=False, return_logits=True)
    out["low_res"], out["iou"], out["masks_sum"] = low.clone(), iou.clone(), masks.sum()
    # ResizeLongestSide on the predictor: apply_coords / apply_boxes at two image sizes
    out["transforms"] = []
    for size in ((427, 640), (96, 72)):
        c = np.array([[0.0, 0.0], [size[1] - 1.0, size[0] - 1.0], [17.5, 3.25], [-4.0, 200.0]])
        bx = np.array([[3.0, 5.0, size[1] - 2.0, size[0] - 0.5], [10.0, 20.0, 30.0, 40.0]])
        out["transforms"].append(dict(size=size, coords=c, boxes=bx, coords_out=pred.transform.apply_coords(c, size), boxes_out=pred.transform.apply_boxes(bx, size)))
    return out


def main():
    r = reference_results()
    fx = {"tokens": r["tokens"], "dense_cells": r["dense_cells"].float(), "cells": pk.golden_cells(), "prompt": {k: v for k, v in r["prompt"].items() if k != "mask"},
          "low_res_sub": r["low_res"][:, :, ::2, ::2].float().clone(), "low_res_sum": r["low_res"].sum(), "iou": r["iou"], "masks_sum": r["masks_sum"],
          "input_size": r["input_size"], "original_size": r["original_size"],
          "transforms": [{k: (torch.as_tensor(v) if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in r["transforms"]]}
    path = os.path.join(ROOT, "tests", "golden", "sam_prompts.pt")
    torch.save(fx, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
