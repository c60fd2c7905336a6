"""CPU: the restatements behind the image front end's GPU tests (tests/image_frontend_checks.py) against the libraries they restate, the size /
crop helpers, and the command line of `python -m llmseg_amd.segment`."""
import numpy as np
import pytest

from tests import image_frontend_checks as fc


def test_bicubic_restatement_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    cases = [(a, None) for a in fc.RESIZE_CASES] + [((90, 120, 224, 150), 0), ((90, 120, 97, 224), 1), ((90, 120, 31, 40), 0), ((90, 120, 31, 40), 1)]
    for n, ((h, w, oh, ow), axis) in enumerate(cases):
        a = fc.random_image(h, w, 100 + n) if axis is None else fc.block_image(h, w, axis)
        ref = np.array(Image.fromarray(a).resize((ow, oh), Image.BICUBIC))
        assert np.array_equal(fc.resize_bicubic_u8(a, oh, ow), ref), (h, w, oh, ow, axis)


def test_block_images_reach_both_ends_of_clip8():
    """The unclipped sums of the 0 / 255 block cases leave [0, 255] on both sides: the negative lobes are exercised."""
    xmin, cnt, kk = fc.coeffs(120, 150)
    assert (kk < 0).any()
    col = fc.block_image(90, 120, 1)[0, :, 0].astype(np.int64)
    acc = np.array([(col[xmin[i]:xmin[i] + cnt[i]] * kk[i, :cnt[i]]).sum() + (1 << 21) for i in range(150)]) >> 22
    assert acc.min() < 0 and acc.max() > 255


def test_tap_count_of_the_long_axis_case_exceeds_the_bilinear_array():
    assert fc.coeffs(3600, 100)[2].shape[1] == 145


def test_clip_restatement_equals_transformers():
    pytest.importorskip("PIL.Image")
    try:
        from transformers import CLIPImageProcessor
        proc = CLIPImageProcessor(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, image_mean=list(fc.CLIP_MEAN), image_std=list(fc.CLIP_STD))
    except Exception as e:                                                     # absent, or no usable image backend
        pytest.skip(f"transformers' CLIP image processor is not usable here: {e}")
    for n, (h, w, S) in enumerate(c for c in fc.CLIP_CASES if c[2] == 224):
        a = fc.random_image(h, w, 300 + n)
        ref = np.asarray(proc.preprocess(a, return_tensors="np")["pixel_values"][0], dtype=np.float64)
        got = fc.clip_preprocess_f64(a, S)
        assert got.shape == ref.shape == (3, S, S)
        assert np.abs(got - ref).max() < 1e-6, (h, w, np.abs(got - ref).max())         # the processor computes in fp32: |v| < 4 -> a few 2^-22


def test_resized_size_and_crop_origin():
    from llmseg_amd import ops
    for (h, w, S, size, origin) in [(427, 640, 224, (224, 335), (0, 55)), (640, 427, 224, (335, 224), (55, 0)), (300, 225, 224, (298, 224), (37, 0)),
                                    (333, 333, 224, (224, 224), (0, 0)), (1, 7, 28, (28, 196), (0, 84)), (1500, 2250, 224, (224, 336), (0, 56)),
                                    (97, 113, 28, (28, 32), (0, 2)), (113, 97, 7, (8, 7), (0, 0))]:
        assert ops.clip_resized_size(h, w, S) == size == fc.clip_resized_size(h, w, S), (h, w, S)
        assert ops.clip_crop_origin(*size, S) == origin, (h, w, S)
    for h in range(1, 40):                                                     # int(S * long / short), not round: never below S, never past the next integer
        for w in range(1, 40):
            nh, nw = ops.clip_resized_size(h, w, 13)
            assert min(nh, nw) == 13 and max(nh, nw) == 13 * max(h, w) // min(h, w)


def test_clip_bound_is_half_a_bf16_spacing_below_four():
    import torch
    x = torch.tensor([3.99], dtype=torch.float32)
    spacing = float(torch.nextafter(x.to(torch.bfloat16).float(), torch.tensor([8.0])).to(torch.bfloat16).float() - x.to(torch.bfloat16).float())
    assert spacing <= 2.0 ** -6 and fc.clip_bound() == 2.0 ** -7 + 1e-6


def test_segment_cli_arguments_and_npy_load(tmp_path):
    from llmseg_amd import segment
    img = fc.random_image(5, 7, 1)
    path = tmp_path / "image.npy"
    np.save(path, img)
    args, margs = segment.parse_args(["--image", str(path), "--query", "the cup", "--query", "what holds water", "--mode", "top5", "--threshold", "0.4",
                                      "--out", str(tmp_path / "m.npy"), "--version", "llava-dir", "--vision_pretrained", "sam.pth", "--backbone", "sam"])
    assert args.query == ["the cup", "what holds water"] and args.mode == "top5" and args.threshold == 0.4 and args.out.endswith("m.npy")
    assert margs.version == "llava-dir" and margs.vision_pretrained == "sam.pth" and margs.backbone == "sam"
    assert np.array_equal(segment.load_image(str(path)), img)
    np.save(path, img[..., 0])
    with pytest.raises(ValueError):
        segment.load_image(str(path))
    with pytest.raises(SystemExit):
        segment.parse_args(["--image", str(path), "--query", "x", "--mode", "best"])


def test_selection_rules_are_those_of_the_validation_loops():
    """`select_proposals` on the CPU against the rules as tests/image_frontend_checks.py states them, ties and an all-below-threshold row included."""
    import torch
    from llmseg_amd import segment
    g = torch.Generator().manual_seed(0)
    for K in (1, 3, 12):
        sim, iou = torch.rand(K, generator=g), torch.rand(K, generator=g)
        for thr in (0.0, 0.5, 2.0):
            for mode in fc.MODES:
                assert torch.equal(segment.select_proposals(mode, sim, iou, thr), fc.rule(mode, sim, iou, thr)), (K, thr, mode)
    with pytest.raises(ValueError):
        segment.select_proposals("best", sim, iou)
