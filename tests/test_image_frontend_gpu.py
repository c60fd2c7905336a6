"""GPU: the raw-image front end -- BICUBIC resize, CLIP preprocessing and mask union (csrc/image.hip), `prepare_image` and `segment`
(llmseg_amd/segment.py).  The checks and their case lists live in tests/image_frontend_checks.py."""
import pytest

pytestmark = pytest.mark.gpu


def _assert(res):
    for name, err, tol in res:
        print(f"{name}: {err:.3e} (bound {tol:.3e})")
    bad = [(n, e, t) for n, e, t in res if not e <= t]
    assert not bad, bad


def test_bicubic_resize_is_pillows_bit_for_bit():
    from tests import image_frontend_checks as fc
    _assert(fc.check_bicubic())


def test_bilinear_route_keeps_its_bits():
    from tests import image_frontend_checks as fc
    _assert(fc.check_bilinear_route())


def test_bicubic_rejects_what_the_table_cannot_hold():
    import torch
    from llmseg_amd import ops
    img = torch.zeros((6500, 2, 3), device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="down-scaling by more than"):
        ops.image_resize_u8(img, 100, 2, resample="bicubic")
    with pytest.raises(ValueError):
        ops.image_resize_u8(img, 100, 2, resample="lanczos")


def test_clip_preprocess():
    from tests import image_frontend_checks as fc
    _assert(fc.check_clip_preprocess())


def test_mask_union():
    from tests import image_frontend_checks as fc
    _assert(fc.check_mask_union())


def test_prepare_image():
    from tests import image_frontend_checks as fc
    _assert(fc.check_prepare_image())


def test_segment_given_proposals():
    from tests import image_frontend_checks as fc
    _assert(fc.check_segment_given_proposals())


def test_segment_generates_proposals_with_one_shared_embedding():
    from tests import image_frontend_checks as fc
    _assert(fc.check_segment_generated())


def test_segment_without_proposals_needs_the_sam_backbone():
    from tests import image_frontend_checks as fc
    _assert(fc.check_segment_needs_sam())
