"""`SamPredictor` on the device (reference `model/segment_anything/predictor.py`): point, box and mask prompts against one image embedding.

`set_image` embeds the image once through the path's SAM encoder (`AmgMixin.set_image`: Pillow-exact resize, normalise, pad).  Every `predict_torch`
then costs two prompt-encoder launches -- `llmseg_sam_prompt_tokens` (points / box corners, prompt_encoder.py:78-109) and `llmseg_sam_dense_prompt`
(the mask prompt folded into the decoder's keys, prompt_encoder.py:56-64,111-114) -- plus the mask decoder (`SamDecoderMixin.sam_decode`) and the fused
post-processing (`llmseg_sam_postprocess`).  Prompts stay on the device: no label is read on the host.

Low-resolution logits can be kept in the decoder's own (nested) row order between refinement rounds (`low_res_nested=True` -> `mask_input` [b, 65536]):
the dense-prompt kernel and the post-processing both index that order directly, so the loop never re-orders a mask.
"""
import numpy as np
import torch

from . import ops
from .amg import preprocess_shape

BF16 = torch.bfloat16
PFX = "model.visual_model.prompt_encoder."
MASK_THRESHOLD = 0.0          # Sam.mask_threshold (modeling/sam.py:18)


def nested_to_raster(low):
    """[..., 65536] in the mask decoder's row order ((y 64 + x) 16 + (dy1 2 + dx1) 4 + dy2 2 + dx2) -> [..., 256, 256]."""
    lead = low.shape[:-1]
    k = len(lead)
    v = low.reshape(*lead, 64, 64, 2, 2, 2, 2)                                   # y, x, dy1, dx1, dy2, dx2
    return v.permute(*range(k), k, k + 2, k + 4, k + 1, k + 3, k + 5).reshape(*lead, 256, 256)


def raster_to_nested(mask):
    """[..., 256, 256] -> [..., 65536] in the mask decoder's row order (the inverse of `nested_to_raster`)."""
    lead = mask.shape[:-2]
    k = len(lead)
    v = mask.reshape(*lead, 64, 2, 2, 64, 2, 2)                                  # y, dy1, dy2, x, dx1, dx2
    return v.permute(*range(k), k, k + 3, k + 1, k + 4, k + 2, k + 5).reshape(*lead, 65536)


def apply_coords(coords, original_size, long_side=1024):
    """`ResizeLongestSide.apply_coords` (utils/transforms.py:36-50): [..., 2] (x, y) in original-image pixels -> the input frame, float64."""
    old_h, old_w = int(original_size[0]), int(original_size[1])
    new_h, new_w = preprocess_shape(old_h, old_w, long_side)
    c = np.array(coords, copy=True).astype(float)
    c[..., 0] = c[..., 0] * (new_w / old_w)
    c[..., 1] = c[..., 1] * (new_h / old_h)
    return c


def apply_boxes(boxes, original_size, long_side=1024):
    """`ResizeLongestSide.apply_boxes` (utils/transforms.py:52-60): [b, 4] XYXY -> the input frame."""
    return apply_coords(np.asarray(boxes).reshape(-1, 2, 2), original_size, long_side).reshape(-1, 4)


class SamPredictor:
    def __init__(self, model, max_batch=256):
        """model: a `LISAForCausalLM` with `backbone="sam"` and `LisaConfig(sam_decoder=True)`; mask prompts also need `sam_prompts=True`.
        max_batch: prompts per decoder pass (each holds 4096 x 256 keys; more are chunked)."""
        if model.config.backbone != "sam" or not model.config.sam_decoder:
            raise ValueError("SamPredictor needs a model built with backbone='sam' and LisaConfig(sam_decoder=True)")
        self.model = model
        self.max_batch = int(max_batch)
        self.reset_image()

    @property
    def device(self):
        return self.model.device_

    def reset_image(self):
        self.is_image_set = False
        self.features = None
        self.original_size = None
        self.input_size = None

    @torch.no_grad()
    def set_image(self, image):
        """image uint8 [H, W, 3] RGB on the device -> the embedding every later `predict` uses."""
        if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3):
            raise ValueError("set_image takes a uint8 [H, W, 3] tensor")
        self.reset_image()
        feats, input_size, original_size = self.model.set_image(image.to(self.device).contiguous())
        self.features, self.input_size, self.original_size = feats, tuple(input_size), tuple(original_size)
        self.is_image_set = True

    def get_image_embedding(self):
        """[1, 256, 64, 64] (a view of the channels-last rows the decoder reads)."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        g = self.model.config.sam.grid
        return self.features.t().reshape(1, self.features.shape[1], g, g)

    def _tokens(self, coords, labels, boxes, b):
        m = self.model
        if coords is None and boxes is None:
            return torch.empty((b, 0, 256), device=self.device, dtype=BF16)
        P, S = m.params, m._samdec()
        return ops.sam_prompt_tokens(coords, labels, boxes, S["G"].contiguous(), [P[f"{PFX}point_embeddings.{i}.weight"] for i in range(4)],
                                     P[PFX + "not_a_point_embed.weight"], frame=m.config.sam.img)

    @torch.no_grad()
    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True, return_logits=False, low_res_nested=False):
        """Prompts in the input frame (after `apply_coords` / `apply_boxes`): point_coords [b, n, 2] (x, y), point_labels [b, n] (1 foreground, 0
        background, -1 ignored), boxes [b, 4] XYXY, mask_input [b, 1, 256, 256] raster logits or [b, 65536] in the nested order `low_res_nested=True`
        returns.  -> (masks [b, C, H, W] bool (`> 0`) or fp32 logits with return_logits, iou fp32 [b, C], low_res fp32 [b, C, 256, 256] or -- low_res_nested --
        [b, C, 65536]); C = 3 with multimask_output, else 1."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        dev = self.device
        b = None
        if (point_coords is None) != (point_labels is None):
            raise ValueError("point_coords and point_labels must be given together")
        if point_coords is not None:
            point_coords = torch.as_tensor(point_coords).to(dev, torch.float32).contiguous()
            point_labels = torch.as_tensor(point_labels).to(dev, torch.int32).contiguous()
            if point_coords.dim() != 3 or point_coords.shape[2] != 2 or tuple(point_labels.shape) != tuple(point_coords.shape[:2]):
                raise ValueError(f"point_coords must be [b, n, 2] and point_labels [b, n], got {tuple(point_coords.shape)} and {tuple(point_labels.shape)}")
            b = int(point_coords.shape[0])
            if point_coords.shape[1] == 0:
                point_coords = point_labels = None
        if boxes is not None:
            boxes = torch.as_tensor(boxes).to(dev, torch.float32).contiguous()
            if boxes.dim() != 2 or boxes.shape[1] != 4 or (b is not None and boxes.shape[0] != b):
                raise ValueError(f"boxes must be [b, 4] with the points' b, got {tuple(boxes.shape)}")
            b = int(boxes.shape[0])
        nested = False
        if mask_input is not None:
            self.model.mask_downscaling_weights()                              # ValueError on a model built without sam_prompts=True
            mask_input = torch.as_tensor(mask_input).to(dev, torch.float32)
            if mask_input.dim() == 4 and tuple(mask_input.shape[1:]) == (1, 256, 256):
                mask_input = mask_input.reshape(mask_input.shape[0], 65536)
            elif mask_input.dim() == 2 and mask_input.shape[1] == 65536:
                nested = True
            else:
                raise ValueError(f"mask_input must be [b, 1, 256, 256] (raster) or [b, 65536] (nested), got {tuple(mask_input.shape)}")
            if b is not None and mask_input.shape[0] != b:
                raise ValueError(f"mask_input holds {mask_input.shape[0]} masks for {b} prompts")
            b = int(mask_input.shape[0])
            mask_input = mask_input.contiguous()
        if b is None:
            b = 1                                                              # no prompt at all: PromptEncoder._get_batch_size
        if b == 0:
            raise ValueError("empty prompt batch")
        lows, ious = [], []
        for i in range(0, b, self.max_batch):
            sl = slice(i, min(b, i + self.max_batch))
            nb = sl.stop - sl.start
            sparse = self._tokens(None if point_coords is None else point_coords[sl].contiguous(), None if point_labels is None else point_labels[sl].contiguous(),
                                  None if boxes is None else boxes[sl].contiguous(), nb)
            low, iou = self.model.sam_decode(self.features, None, sparse=sparse, multimask_output=multimask_output,
                                             mask_input=None if mask_input is None else mask_input[sl], mask_nested=nested)
            lows.append(low.view(nb, -1, 65536))
            ious.append(iou.float())
        low = torch.cat(lows, 0) if len(lows) > 1 else lows[0]                  # [b, C, 65536] nested
        iou = torch.cat(ious, 0) if len(ious) > 1 else ious[0]
        C = low.shape[1]
        H, W = self.original_size
        masks = ops.sam_postprocess(low.reshape(b * C, 65536), self.input_size, (H, W), img_size=self.model.config.sam.img).view(b, C, H, W)
        if not return_logits:
            masks = masks > MASK_THRESHOLD
        return masks, iou, (low if low_res_nested else nested_to_raster(low).contiguous())

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output=True, return_logits=False):
        """numpy prompts in ORIGINAL-image pixels (predictor.py:93-175): point_coords [n, 2], point_labels [n], box [4], mask_input [1, 256, 256]
        -> (masks [C, H, W], iou [C], low_res [C, 256, 256]) as numpy."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        coords_t = labels_t = box_t = mask_t = None
        img = self.model.config.sam.img
        if point_coords is not None:
            if point_labels is None:
                raise ValueError("point_labels must be supplied if point_coords is supplied.")
            coords_t = torch.as_tensor(apply_coords(np.asarray(point_coords), self.original_size, img), dtype=torch.float32)[None]
            labels_t = torch.as_tensor(np.asarray(point_labels), dtype=torch.int32)[None]
        elif point_labels is not None:
            raise ValueError("point_coords must be supplied if point_labels is supplied.")
        if box is not None:
            box_t = torch.as_tensor(apply_boxes(np.asarray(box), self.original_size, img), dtype=torch.float32)
        if mask_input is not None:
            mask_t = torch.as_tensor(np.asarray(mask_input), dtype=torch.float32)[None]
        masks, iou, low = self.predict_torch(coords_t, labels_t, box_t, mask_t, multimask_output, return_logits=return_logits)
        return masks[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()
