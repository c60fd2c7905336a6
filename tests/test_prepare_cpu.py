"""CPU: the proposal file -- `prepare.write_masks_json` writes what the reference's convert_h5_to_json.py writes, `targets.SamMaskReader` reads it as
the reference's `SAM_Mask_Reader` does -- and the host routes of the codec stay what they were."""
import json

import numpy as np
import pytest
import torch


def _samples():
    from llmseg_amd import amg
    rng = np.random.default_rng(2)
    out = []
    for name, (h, w, k) in (("b.png", (20, 31, 3)), ("a.jpg", (17, 12, 2)), ("none.npy", (9, 9, 0))):
        masks = torch.from_numpy((rng.random((k, h, w)) > 0.5).astype(np.uint8))
        gen = dict(masks=masks, boxes=torch.arange(4 * k).reshape(k, 4), iou_preds=torch.linspace(0.9, 1.0, k), stability_score=torch.linspace(0.95, 1.0, k),
                   points=torch.arange(2.0 * k, dtype=torch.float64).reshape(k, 2), areas=masks.flatten(1).sum(1))
        out.append({"image": name, "target_size": [h, w], "masks": amg.to_records(gen, (h, w))})
    return out


def test_masks_json_round_trip_and_reader_index(tmp_path):
    from llmseg_amd import prepare, targets as ht
    samples = _samples()
    path = str(tmp_path / "masks.json")
    prepare.write_masks_json(samples, path)
    loaded = json.load(open(path))
    assert loaded == samples and isinstance(loaded, list)
    for s in loaded:
        assert set(s) == {"image", "target_size", "masks"}
        for m in s["masks"]:
            assert set(m) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}
            assert type(m["segmentation"]["counts"]) is str and m["segmentation"]["size"] == s["target_size"]
    r = ht.SamMaskReader(path)
    assert r.mask_list == samples and r.sam_mask_index == {"b.png": 0, "a.jpg": 1, "none.npy": 2}
    assert r.read_mask_json(path) == samples and r.build_sam_mask_index() == r.sam_mask_index
    assert r.get_sam_mask_index("a.jpg") == 1
    with pytest.raises(ValueError, match="missing.jpg"):
        r.get_sam_mask_index("missing.jpg")
    with pytest.raises(ValueError):
        r.extract_sam_segs("missing.jpg", "cpu")


def test_write_masks_json_refuses_uncompressed_counts(tmp_path):
    from llmseg_amd import prepare
    s = _samples()[:1]
    s[0]["masks"][0]["segmentation"]["counts"] = [1, 2, 3]
    with pytest.raises(AssertionError, match="strings"):
        prepare.write_masks_json(s, str(tmp_path / "bad.json"))


def test_prepare_flags_mirror_the_generator():
    """Every generator flag of the command line is an argument of `generate_masks` with the same default."""
    import inspect
    from llmseg_amd import amg, prepare
    sig = inspect.signature(amg.AmgMixin.generate_masks).parameters
    for name, typ, default in prepare.GENERATOR_FLAGS:
        assert sig[name].default == default and isinstance(default, typ), name
    args, margs = prepare.parse_args(["--image_dir", "d", "--points_per_side", "8", "--max_side", "192", "--lora_r", "4"])
    assert args.image_dir == "d" and args.points_per_side == 8 and args.max_side == 192 and args.out == "masks.json" and margs.lora_r == 4


def test_decode_rles_on_a_cpu_device_keeps_the_host_parse(monkeypatch):
    """`host_parse=False` on a CPU device: the host route up to the device call (the codec kernels need a GPU; the parse does not)."""
    from llmseg_amd import _lib, targets as ht
    from oracle import targets as ot
    m = (np.random.default_rng(0).random((2, 11, 7)) > 0.5).astype(np.uint8)
    recs = [ot.rle_encode(x) for x in m]
    seen = {}

    class Lib:
        def llmseg_rle_decode(self, ends, offs, out, K, H, W, hwk, stream):
            seen.update(K=K, H=H, W=W, hwk=hwk)
            return 0

        def llmseg_rle_parse(self, *a):
            raise AssertionError("the device parse was called for a CPU device")

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(ht, "_stream", lambda: None)
    for kw in (dict(), dict(host_parse=False), dict(host_parse=True)):
        out = ht.decode_rles(recs, "cpu", **kw)
        assert out.shape == (2, 11, 7) and out.device.type == "cpu" and seen == dict(K=2, H=11, W=7, hwk=0)
    assert ht.decode_rles(recs, torch.device("cpu"), hwk=True).shape == (11, 7, 2)
    # the host encoder is what it was: CPU tensors and arrays never touch the library
    assert ht.rle_encode_masks(torch.from_numpy(m)) == recs == ht.rle_encode_masks(m)
