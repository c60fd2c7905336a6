"""GPU: `python -m llmseg_amd.prepare` end to end on a directory of small images with the suite's tiny SAM model: the JSON it writes, read back by
`targets.SamMaskReader`, holds the proposals a direct `generate_masks` of the same (resized) image yields."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}
MAX_SIDE = 192


def test_prepare_writes_the_proposals_of_every_image(tmp_path):
    from PIL import Image
    from llmseg_amd import ops, prepare, targets as ht
    from oracle import cases
    from tests import image_frontend_checks as fc
    model = fc.tiny_model()
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    images = {"b_small.png": cases.amg_image_case(150, 190), "a_small.png": cases.amg_image_case(180, 140), "c_large.png": cases.amg_image_case(200, 250)}
    for name, a in images.items():
        Image.fromarray(a).save(str(img_dir / name))
    (img_dir / "notes.txt").write_text("not an image")
    th = cases.amg_thresholds()
    kw = dict(points_per_side=8, points_per_batch=24, **th)
    argv = ["--image_dir", str(img_dir), "--out", str(tmp_path / "masks.json"), "--max_side", str(MAX_SIDE), "--points_per_side", "8", "--points_per_batch", "24"]
    for n, v in th.items():
        argv += ["--" + n, str(v)]
    samples = prepare.main(argv, model=model, device=DEV)
    assert [s["image"] for s in samples] == sorted(images)
    reader = ht.SamMaskReader(str(tmp_path / "masks.json"))
    assert reader.mask_list == samples
    n_proposals = 0
    for name, a in images.items():
        d = torch.as_tensor(a).to(DEV)
        H, W = a.shape[:2]
        if max(H, W) > MAX_SIDE:
            s = float(MAX_SIDE) / max(H, W)
            d = ops.image_resize_u8(d, int(H * s), int(W * s))
            assert name == "c_large.png" and tuple(d.shape[:2]) == (153, 192)
        h, w = int(d.shape[0]), int(d.shape[1])
        sample = reader.mask_list[reader.get_sam_mask_index(name)]
        assert sample["target_size"] == [h, w]
        assert all(set(m) == FIELDS and m["segmentation"]["size"] == [h, w] and type(m["segmentation"]["counts"]) is str for m in sample["masks"])
        gen = model.generate_masks(d.contiguous(), **kw)
        assert len(sample["masks"]) == gen["masks"].shape[0]
        n_proposals += len(sample["masks"])
        if not sample["masks"]:
            continue
        assert [m["area"] for m in sample["masks"]] == gen["areas"].tolist()
        got = reader.extract_sam_segs(name, DEV)["segs_origin"]
        order = torch.argsort(gen["areas"], descending=True, stable=True)[:50]
        want = gen["masks"][order]
        # equal areas may be ordered differently by the two sorts: compare as sets keyed by the mask bytes
        key = lambda segs: sorted(bytes(s.cpu().numpy().tobytes()) for s in segs)
        assert got.shape == want.shape and key(got) == key(want)
    assert n_proposals > 0, "no image yielded a proposal: the comparison above checked nothing"
