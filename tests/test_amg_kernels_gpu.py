"""GPU: the seven device steps of SAM "everything" mode on the tables of tests/amg_kernel_checks.py, against the references and bounds that
tests/test_amg_kernels_cpu.py validates.  sam_postprocess / sam_mask_stats / sam_binarize: the statistics and the binary masks are EXACTLY the reductions
of sam_postprocess's own output, the values are inside the derived fp64 bound and bit-equal to the fp32 emulation; nms, mask_small_regions, mask_boxes and
sam_preprocess are exact against their oracles.  Every call is checked to leave the bytes around its output alone where the test owns the buffer."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import amg as oamg
from tests import amg_kernel_checks as ak

pytestmark = pytest.mark.gpu

DEV = "cuda"
GEOMS = list(range(len(ak.GEOMETRIES)))
GIDS = [ak.geometry_id(g) for g in ak.GEOMETRIES]
GUARD = 256
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield
    if _WORST:
        print("\npost-processing: worst |kernel - fp64| / bound per geometry, elements that differ from the fp32 emulation in bits")
        for k in sorted(_WORST):
            print(f"  {k:44s} {_WORST[k][0]:.3f}  {_WORST[k][1]}")


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                            # a device fault: nothing more may be started on this GPU
        pytest.exit(f"device fault: {e}", returncode=3)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _emulation(gi):
    return ak.post_emulation(ak.logits(gi), ak.GEOMETRIES[gi])


def _reductions(P, thr, off):
    """the seven statistics of a [n, oh, ow] fp32 tensor, by torch on the device: int32 [n, 7]"""
    n, oh, ow = P.shape
    t_hi, t_lo = float(np.float32(thr) + np.float32(off)), float(np.float32(thr) - np.float32(off))
    m = P > thr
    rows, cols = m.any(2), m.any(1)
    ys, xs = torch.arange(oh, device=P.device), torch.arange(ow, device=P.device)
    big, neg = torch.tensor(2 ** 31 - 1, device=P.device), torch.tensor(-1, device=P.device)
    out = [(P > t_hi).flatten(1).sum(1), (P > t_lo).flatten(1).sum(1), m.flatten(1).sum(1),
           torch.where(cols, xs, big).min(1).values, torch.where(rows, ys, big).min(1).values,
           torch.where(cols, xs, neg).max(1).values, torch.where(rows, ys, neg).max(1).values]
    return torch.stack(out, 1).to(torch.int32)


# ------------------------------------------------------------- post-processing -------------------------------------------------------------
@pytest.mark.parametrize("nested", [False, True], ids=["raster", "nested"])
@pytest.mark.parametrize("gi", GEOMS, ids=GIDS)
def test_postprocess_stats_binarize(gi, nested):
    from llmseg_amd import ops
    g = ak.GEOMETRIES[gi]
    img, inp, orig = g[:3]
    low = ak.logits(gi)
    d = _dev(ak.to_nested(low) if nested else low)
    ref, bound = ak.reference(gi), ak.post_bound(low)
    P = ops.sam_postprocess(d, inp, orig, img, nested=nested)
    got = P.cpu().numpy()
    assert got.shape == ref.shape
    ratio = float(np.abs(got - ref).max() / bound)
    emu = _emulation(gi)
    n_bits = int((got.view(np.int32) != emu.view(np.int32)).sum())
    _WORST[f"{gi} {GIDS[gi]} {'nested' if nested else 'raster'}"] = (ratio, n_bits)
    print(f"\n{GIDS[gi]} nested={nested}: {ratio:.3f} of the bound, {n_bits} of {got.size} elements differ from the fp32 emulation")
    assert ratio <= 1.0, f"sam_postprocess is at {ratio:.3f} of the fp64 bound"
    assert n_bits == 0, f"{n_bits} elements are not the fp32 emulation's bits"
    ones = torch.ones((ak.N_LOGITS,), device=DEV)
    sel = torch.tensor(ak.SEL, device=DEV, dtype=torch.int32)
    for thr, off in ak.THRESHOLDS:
        st = ops.sam_mask_stats(d, ones, -1.0, inp, orig, img, thr, off, nested=nested)
        want = _reductions(P, thr, off)
        assert torch.equal(st, want), f"thresholds ({thr}, {off}): statistics {st.tolist()} are not the reductions of sam_postprocess {want.tolist()}"
        assert st[2].tolist() == ak.STATS_INIT, "the all -5 mask is empty: the wrapper's initial row"
        bad = ak.stats_agree(st.cpu().numpy(), ref, thr, off, bound)
        assert bad == [], bad
        bm = ops.sam_binarize(d, sel, inp, orig, img, thr, nested=nested)
        assert bm.dtype == torch.uint8 and torch.equal(bm, (P[sel.long()] > thr).to(torch.uint8)), f"threshold {thr}: sam_binarize is not sam_postprocess > thr"


@pytest.mark.parametrize("gi", [0, 5], ids=[GIDS[0], GIDS[5]])
def test_mask_stats_filter(gi):
    from llmseg_amd import ops
    img, inp, orig = ak.GEOMETRIES[gi][:3]
    d = _dev(ak.to_nested(ak.logits(gi)))
    thresh = float(np.float32(0.88))
    init = torch.tensor(ak.STATS_INIT, device=DEV, dtype=torch.int32)
    full = ops.sam_mask_stats(d, torch.ones((4,), device=DEV), -1.0, inp, orig, img, 0.0, 1.0)
    assert int(full[0, 2]) > 0 and int(full[1, 2]) > 0 and int(full[3, 2]) > 0         # smooth, frame, all +5: not empty (all -5 is)
    # (above, EQUAL, NaN, below), then (NaN, above, below, equal): only `iou > thresh` passes, the rows of the others stay as the wrapper made them
    for iou, passes in (([0.95, thresh, float("nan"), 0.5], 0), ([float("nan"), 0.9, 0.5, thresh], 1)):
        st = ops.sam_mask_stats(d, torch.tensor(iou, device=DEV, dtype=torch.float32), thresh, inp, orig, img, 0.0, 1.0)
        for k in range(4):
            if k == passes:
                assert torch.equal(st[k], full[k]), f"candidate {k} passes: {st[k].tolist()} is not the unfiltered {full[k].tolist()}"
            else:
                assert torch.equal(st[k], init), f"candidate {k} (iou {iou[k]}) fails iou > {thresh}: its row must stay the initial one, got {st[k].tolist()}"


def test_post_refusals_launch_nothing():
    from llmseg_amd import _lib
    lib = _lib.load()
    low = torch.zeros((2, 65536), device=DEV)
    out = torch.zeros((2, 8, 8), device=DEV)
    st = torch.zeros((2, 7), device=DEV, dtype=torch.int32)
    iou = torch.ones((2,), device=DEV)
    sel = torch.zeros((1,), device=DEV, dtype=torch.int32)
    bm = torch.zeros((1, 8, 8), device=DEV, dtype=torch.uint8)
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    s = _stream()
    post = lambda lo=_p(low), o=_p(out), n=2, im=1024, ih=683, iw=1024, oh=8, ow=8: lib.llmseg_sam_postprocess(lo, o, n, im, ih, iw, oh, ow, 0, s)
    stats = lambda lo=_p(low), t=_p(st), n=2, im=1024, ih=683, iw=1024, oh=8, ow=8: lib.llmseg_sam_mask_stats(lo, _p(iou), 0.5, t, n, im, ih, iw, oh, ow, 0, 0.0, 1.0, s)
    binz = lambda lo=_p(low), se=_p(sel), o=_p(bm), n=1, im=1024, ih=683, iw=1024, oh=8, ow=8: lib.llmseg_sam_binarize(lo, se, o, n, im, ih, iw, oh, ow, 0, 0.0, s)
    for name, fn in (("sam_postprocess", post), ("sam_mask_stats", stats), ("sam_binarize", binz)):
        for kw in (dict(n=0), dict(n=-1), dict(ih=1025), dict(iw=1025), dict(ih=0), dict(oh=0), dict(ow=-3), dict(im=0), dict(lo=None), dict(o=None) if name != "sam_mask_stats" else dict(t=None)):
            assert fn(**kw) == -1, f"{name} accepted {kw}"
            assert name.encode() in lib.llmseg_last_error(), lib.llmseg_last_error()
    assert binz(se=None) == -1
    assert stats(n=65536) == -1 and b"grid limit" in lib.llmseg_last_error()
    assert lib.llmseg_launch_count() == n0, "a refused call launched a kernel"
    # the same calls with good arguments go through (the input size equal to img_size is allowed)
    assert post(ih=1024) == 0 and stats(ih=1024) == 0 and binz(ih=1024) == 0, lib.llmseg_last_error()
    assert lib.llmseg_launch_count() == n0 + 3


# ------------------------------------------------------------------- NMS -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ak.NMS_CASES))
def test_nms_keeps_what_the_oracle_keeps(name):
    from llmseg_amd import ops
    b, order, thr, _ = ak.NMS_CASES[name]
    db, do = _dev(b), _dev(order)
    k1 = ops.nms(db, do, thr)
    k2 = ops.nms(db, do, thr)
    assert k1.dtype == torch.uint8 and k1.shape == (len(order),) and int(k1.max()) <= 1
    assert torch.equal(k1, k2), "two runs on the same input differ"
    got = order[k1.cpu().numpy().astype(bool)]
    want = ak.nms_oracle(name)
    assert got.tolist() == want.tolist(), f"{name}: {len(got)} kept, the oracle keeps {len(want)}"


def test_nms_refuses_more_than_the_limit_before_any_launch():
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    n = ak.NMS_LIMIT + 1
    b = torch.zeros((n, 4), device=DEV)
    order = torch.arange(n, device=DEV, dtype=torch.int32)
    torch.cuda.synchronize()
    n0 = lib.llmseg_launch_count()
    with pytest.raises(RuntimeError, match="8192"):
        ops.nms(b, order, 0.5)
    keep = torch.zeros((4,), device=DEV, dtype=torch.uint8)
    assert lib.llmseg_nms(_p(b), _p(order), 0, 0.5, _p(keep), _stream()) == -1
    assert lib.llmseg_nms(None, _p(order), 4, 0.5, _p(keep), _stream()) == -1
    assert lib.llmseg_nms(_p(b), _p(order), 4, 0.5, None, _stream()) == -1
    assert lib.llmseg_launch_count() == n0


# ------------------------------------------------------------- small regions -------------------------------------------------------------
def _guarded_masks(ms):
    """the masks inside a larger buffer filled with 0xA5: -> (buffer, the [K, H, W] view the kernels get)"""
    K, H, W = ms.shape
    buf = torch.full((2 * GUARD + K * H * W,), 0xA5, device=DEV, dtype=torch.uint8)
    view = buf[GUARD:GUARD + K * H * W].view(K, H, W)
    view.copy_(_dev(ms))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + GUARD
    return buf, view


def _guard_untouched(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


@pytest.mark.parametrize("shape", ak.SHAPES, ids=[f"{h}x{w}" for h, w in ak.SHAPES])
def test_small_regions_and_boxes(shape):
    from llmseg_amd import ops
    names, ms = ak.region_masks(shape)
    K = len(names)
    # boxes and pixel sums of the patterns themselves: 0 / 255 storage and the empty mask included
    bx, ar = ops.mask_boxes(_dev(ms))
    assert bx.cpu().tolist() == oamg.masks_to_boxes(torch.from_numpy(ms != 0)).long().tolist()
    assert ar.cpu().tolist() == (ms != 0).reshape(K, -1).sum(1).tolist()
    assert bx[names.index("empty")].tolist() == [0, 0, 0, 0] and int(ar[names.index("empty")]) == 0
    for a in ak.MIN_AREAS:
        a = ak.min_area_of(a, shape)
        ref, ch_ref, box_ref, area_ref = ak.region_reference(shape, a)
        buf, view = _guarded_masks(ms)
        ch = ops.mask_small_regions_(view, a)
        assert _guard_untouched(buf), f"min_area {a}: bytes around the masks changed"
        got = view.cpu().numpy()
        wrong = [(names[k], int(((got[k] != 0) != ref[k]).sum())) for k in range(K) if not np.array_equal(got[k] != 0, ref[k])]
        assert wrong == [], f"min_area {a}: pixels that differ from the oracle {wrong}"
        assert ch.cpu().bool().tolist() == ch_ref.tolist(), f"min_area {a}: changed flags"
        bx, ar = ops.mask_boxes(view)
        assert bx.cpu().tolist() == box_ref.tolist() and ar.cpu().tolist() == area_ref.tolist(), f"min_area {a}: boxes / areas of the cleaned masks"
        buf2, view2 = _guarded_masks(ms)
        ch2 = ops.mask_small_regions_(view2, a)
        assert torch.equal(buf2, buf) and torch.equal(ch2, ch), f"min_area {a}: a second run gives other bytes"


def test_small_regions_chunks_are_the_single_call(monkeypatch):
    from llmseg_amd import _lib, ops
    lib = _lib.load()
    shape = (64, 257)
    names, ms = ak.region_masks(shape)
    ms = ms[[names.index(n) for n in ("blobs", "exact_sizes", "small_tie_of_two", "blobs_as_0_255", "serpentine", "small_tie_of_three", "zigzag")]]
    assert len(ms) == 7
    per = int(lib.llmseg_mask_small_regions_workspace(1, *shape))
    for a in (4, 30):
        buf1, v1 = _guarded_masks(ms)
        torch.cuda.synchronize()
        n0 = lib.llmseg_launch_count()
        c1 = ops.mask_small_regions_(v1, a)
        single = lib.llmseg_launch_count() - n0
        with monkeypatch.context() as mp:
            mp.setattr(ops, "SMALL_REGIONS_WS_BYTES", 3 * per + per // 2)          # chunks of 3, 3, 1
            buf2, v2 = _guarded_masks(ms)
            n0 = lib.llmseg_launch_count()
            c2 = ops.mask_small_regions_(v2, a)
            assert lib.llmseg_launch_count() - n0 == 3 * single, "7 masks under a budget of 3 must go in three calls"
        assert torch.equal(buf1, buf2) and torch.equal(c1, c2)
        assert _guard_untouched(buf2)


# -------------------------------------------------------------- sam_preprocess --------------------------------------------------------------
@pytest.mark.parametrize("hw,S", ak.PRE_SIZES, ids=[f"{h}x{w}-in-{S}" for (h, w), S in ak.PRE_SIZES])
def test_preprocess_bits(hw, S):
    from llmseg_amd import _lib, ops
    h, w = hw
    img = _dev(ak.pre_image(h, w))
    ref = ak.pre_reference(h, w, S)
    got = ops.sam_preprocess(img, S, oamg.PIXEL_MEAN, oamg.PIXEL_STD)
    assert got.shape == (1, 3, S, S) and got.dtype == torch.bfloat16
    bits = got.view(torch.int16)[0].cpu().numpy()
    assert (bits[:, h:, :] == 0).all() and (bits[:, :, w:] == 0).all(), "padding must be +0.0"
    diff = np.argwhere(bits != ref)
    assert len(diff) == 0, f"{len(diff)} elements differ from the fp64 reference rounded once, first at (c, y, x) = {diff[:3].tolist()}"
    # the same through the C entry point into a buffer of our own: the bytes around the output stay
    lib = _lib.load()
    buf = torch.full((2 * GUARD + 3 * S * S,), 0x5A5A, device=DEV, dtype=torch.int16)
    m3, s3 = (C.c_float * 3)(*oamg.PIXEL_MEAN), (C.c_float * 3)(*oamg.PIXEL_STD)
    rc = lib.llmseg_sam_preprocess(_p(img), C.c_void_p(buf.data_ptr() + 2 * GUARD), h, w, S, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), _stream())
    assert rc == 0, lib.llmseg_last_error()
    assert bool((buf[:GUARD] == 0x5A5A).all()) and bool((buf[-GUARD:] == 0x5A5A).all())
    assert np.array_equal(buf[GUARD:-GUARD].view(3, S, S).cpu().numpy(), ref)
    assert lib.llmseg_sam_preprocess(_p(img), C.c_void_p(buf.data_ptr()), S + 1, w, S, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), _stream()) == -1


# --------------------------------------------------------------- the pipeline ---------------------------------------------------------------
def test_generate_proposals_with_nothing_passing_returns_the_empty_records(monkeypatch):
    from llmseg_amd import ops
    from oracle import cases
    from tests import sam_decoder_checks as sc
    m, _ = sc._model()
    emb = cases.amg_embedding_case().to(torch.bfloat16).float()
    f_cl = emb[0].reshape(256, 4096).t().contiguous().to(DEV, torch.bfloat16)

    def never(*a, **k):
        raise AssertionError("no candidate passes: neither NMS nor binarize may run")
    monkeypatch.setattr(ops, "nms", never)
    monkeypatch.setattr(ops, "sam_binarize", never)
    thr = dict(cases.amg_thresholds(), pred_iou_thresh=2.0)
    out = m.generate_proposals(f_cl, (683, 1024), (427, 640), points_per_side=4, points_per_batch=16, **thr)
    want = dict(masks=((0, 427, 640), torch.uint8), boxes=((0, 4), torch.int64), iou_preds=((0,), torch.float32), stability_score=((0,), torch.float32),
                points=((0, 2), torch.float64), areas=((0,), torch.int64))
    assert set(out) == set(want)
    for k, (shape, dtype) in want.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype, (k, out[k].shape, out[k].dtype)
