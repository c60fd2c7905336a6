"""GPU: the training-target kernels (llmseg_rle_decode, llmseg_gt_resample, llmseg_mask_targets, llmseg_resize_aa, llmseg_proposal_targets) and the
validation-metric kernels (llmseg_intersection_union, llmseg_union_resize_iou) through the C ABI on the tables of tests/target_kernel_checks.py, against
the references that tests/test_target_kernels_cpu.py validates.  Integers, and the IoU / IoP divisions of them, exactly; proposal maps bit for bit
wherever the exact value decides the bf16 (elsewhere one of the two neighbours); the fused pass against the three-kernel route with torch.equal.  Every
output lies between canaries: nothing is written beyond it, and a refused call writes nothing at all and launches nothing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import target_kernel_checks as tk

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = [c["name"] for c in tk.CASES]
CANARY, PAD = 0xC5, 256
EINVAL = -1
_SEEN = {}
_LIVE = []                                               # inputs stay allocated until their test is over: the kernels read them after `_p` returned


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    yield
    if _SEEN:
        print("\nproposal maps, per case: pixels, undecided by the reference, kernel pixels outside the bounds, undecided pixels that took the upper value")
        for n in NAMES:
            if n in _SEEN:
                print(f"  {n:22s} " + "  ".join(f"{v:7d}" for v in _SEEN[n]))


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                            # a device fault: nothing more may be started on this GPU
        pytest.exit(f"device fault: {e}", returncode=3)
    del _LIVE[:]


def _lib():
    from llmseg_amd import _lib as L
    return L.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, offset=0):
    """numpy array -> device tensor of the same shape and dtype; offset > 0: at that many bytes into a 256-byte aligned buffer"""
    a = np.ascontiguousarray(a)
    if not offset:
        t = torch.from_numpy(a.copy()).to(DEV)
    else:
        raw = torch.zeros((a.nbytes + 256,), device=DEV, dtype=torch.uint8)
        assert raw.data_ptr() % 256 == 0
        view = raw[offset:offset + a.nbytes]
        view.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        t = view.view(torch.from_numpy(np.empty(0, a.dtype)).dtype).view(a.shape)
    _LIVE.append(t)
    return t


class Out:
    """an output of `shape` between two PAD-byte canaries, itself canary-filled"""

    def __init__(self, shape, dtype, offset=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((PAD + offset + n + PAD,), CANARY, device=DEV, dtype=torch.uint8)
        self.a, self.b = PAD + offset, PAD + offset + n
        self.t = self.raw[self.a:self.b].view(dtype).view(shape)

    def pads_intact(self):
        return bool((self.raw[:self.a] == CANARY).all()) and bool((self.raw[self.b:] == CANARY).all())

    def untouched(self):
        return bool((self.raw == CANARY).all())


def _tables(tabs):
    first, count, w, taps = tabs
    return _dev(first), _dev(count), _dev(w), taps


def _bits(t):
    return t.view(torch.int16).cpu().numpy()


def _nearest(out_n, in_n):
    from llmseg_amd import targets as ht
    return _dev(ht.nearest_index(out_n, in_n))


def _resample_gts(name, offset=0):
    """llmseg_gt_resample of every ground truth of the case -> Out [C, H, W]; each plane equals the reference, nothing written beyond"""
    c, gts = tk.CASE[name], tk.gts_of(name)
    H, W = c["H"], c["W"]
    gtp = Out((max(len(gts), 1), H, W), torch.uint8, offset)
    for i, g in enumerate(gts):
        rc = _lib().llmseg_gt_resample(_p(_dev(g)), _p(_nearest(H, g.shape[0])), _p(_nearest(W, g.shape[1])), _p(gtp.t[i]), H, W, g.shape[0], g.shape[1], _stream())
        assert rc == 0, _lib().llmseg_last_error()
    torch.cuda.synchronize()
    for i in range(len(gts)):
        assert np.array_equal(gtp.t[i].cpu().numpy(), tk.reference(name)["gts"][i][0]), f"{name}: gt_resample of ground truth {i}"
    assert gtp.pads_intact()
    return gtp


@functools.lru_cache(maxsize=None)
def _fused(name):
    """the raw entry point on the case (the first <= 4 ground truths) -> dict of device results; shared by the tests, never modified"""
    c = tk.CASE[name]
    assert tk.fused_takes(c)
    H, W, K, OS = c["H"], c["W"], c["K"], c["out"]
    masks = _dev(tk.masks_of(name), c["misalign"])
    assert masks.data_ptr() % 16 == c["misalign"]
    order = None if c["order"] is None else _dev(np.array(c["order"], np.int64))
    gtp = _resample_gts(name, c["misalign"])
    n = min(len(c["gts"]), tk.LIMITS["n_gt"])
    d_first, d_count, d_w, taps = _tables(tk.tables_of(c))
    out = Out((K, OS, OS), torch.bfloat16)
    cnt, area = Out((max(n, 1), K, 2), torch.int64), Out((max(n, 1),), torch.int64)
    iou, iop = Out((max(n, 1), K), torch.float64), Out((max(n, 1), K), torch.float64)
    lib = _lib()
    n0 = lib.llmseg_launch_count()
    rc = lib.llmseg_proposal_targets(_p(masks), _p(order), _p(gtp.t) if n else None, n, _p(out.t), K, H, W, OS, _p(d_first), _p(d_count), _p(d_w), _p(d_first), _p(d_count),
                                     _p(d_w), taps, _p(cnt.t) if n else None, _p(area.t) if n else None, _p(iou.t) if n else None, _p(iop.t) if n else None, _stream())
    assert rc == 0, lib.llmseg_last_error()
    launches = lib.llmseg_launch_count() - n0
    torch.cuda.synchronize()
    return dict(masks=masks, order=order, gtp=gtp, n=n, out=out, cnt=cnt, area=area, iou=iou, iop=iop, launches=launches, tabs=(d_first, d_count, d_w, taps))


def _check_maps(name, bits):
    ref = tk.reference(name)
    bad = tk.maps_agree(bits, ref["lo"], ref["hi"])
    und = ref["lo"] != ref["hi"]
    _SEEN[name] = (int(bits.size), int(und.sum()), bad, int((und & (bits == ref["hi"])).sum()))
    print(f"\n{name}: {bits.size} pixels, {int(und.sum())} undecided, {bad} outside the bounds")
    assert bad == 0, f"{name}: {bad} of {bits.size} map pixels are not the bf16 the exact value decides"


def _check_targets(name, g, cnt, area, iou, iop):
    _, rc, ra, riou, riop = tk.reference(name)["gts"][g]
    assert np.array_equal(cnt.cpu().numpy(), rc), f"{name}: counts of ground truth {g}: {cnt.cpu().numpy().tolist()[:4]} != {rc.tolist()[:4]}"
    if area is not None:
        assert int(area) == ra, f"{name}: area of ground truth {g}: {int(area)} != {ra}"
    assert np.array_equal(iou.cpu().numpy(), riou, equal_nan=True), f"{name}: iou of ground truth {g}"
    assert np.array_equal(iop.cpu().numpy(), riop, equal_nan=True), f"{name}: iop of ground truth {g}"


FUSED = [n for n in NAMES if tk.fused_takes(tk.CASE[n])]
REFUSED = [n for n in NAMES if not tk.fused_takes(tk.CASE[n])]


# ------------------------------------------------------------ the one-pass kernel ------------------------------------------------------------
@pytest.mark.parametrize("name", FUSED)
def test_fused_pass_equals_the_exact_reference(name):
    r = _fused(name)
    c = tk.CASE[name]
    _check_maps(name, _bits(r["out"].t))
    for g in range(r["n"]):
        _check_targets(name, g, r["cnt"].t[g], r["area"].t[g], r["iou"].t[g], r["iop"].t[g])
    assert r["launches"] == 1 + r["n"]                                     # the pass + one finalize per ground truth
    assert all(r[k].pads_intact() for k in ("out", "cnt", "area", "iou", "iop")), "written beyond an output"
    if r["n"] == 0:                                                        # maps only: the NULL outputs' stand-ins were never passed, and stay canaries
        assert all(r[k].untouched() for k in ("cnt", "area", "iou", "iop")) and c["gts"] == []


@pytest.mark.parametrize("name", FUSED)
def test_fused_pass_equals_the_three_kernel_route(name):
    """llmseg_resize_aa + llmseg_mask_targets on the gathered proposals, with the same tables: torch.equal on the maps ("bit-identical" in the header),
    equal integers and divisions"""
    r = _fused(name)
    c = tk.CASE[name]
    H, W, K, OS = c["H"], c["W"], c["K"], c["out"]
    segs = _dev(tk.selected(name))
    d_first, d_count, d_w, taps = r["tabs"]
    lib = _lib()
    out = Out((K, OS, OS), torch.bfloat16)
    assert lib.llmseg_resize_aa(_p(segs), _p(out.t), K, H, W, OS, _p(d_first), _p(d_count), _p(d_w), _p(d_first), _p(d_count), _p(d_w), taps, _stream()) == 0
    torch.cuda.synchronize()
    assert out.pads_intact()
    assert tk.maps_agree(_bits(out.t), tk.reference(name)["lo"], tk.reference(name)["hi"]) == 0, "llmseg_resize_aa misses the exact reference"
    assert torch.equal(out.t, r["out"].t), f"{name}: {int((out.t.view(torch.int16) != r['out'].t.view(torch.int16)).sum())} pixels differ between the two routes"
    for g, gt in enumerate(tk.gts_of(name)):                               # all of them, also beyond the four of one fused launch
        cnt, area = Out((K, 2), torch.int64), Out((1,), torch.int64)
        iou, iop = Out((K,), torch.float64), Out((K,), torch.float64)
        cnt.t.zero_(); area.t.zero_()
        rc = lib.llmseg_mask_targets(_p(segs), _p(_dev(gt)), _p(_nearest(H, gt.shape[0])), _p(_nearest(W, gt.shape[1])), K, H, W, gt.shape[0], gt.shape[1], _p(cnt.t),
                                     _p(area.t), _p(iou.t), _p(iop.t), _stream())
        assert rc == 0, lib.llmseg_last_error()
        torch.cuda.synchronize()
        _check_targets(name, g, cnt.t, area.t[0], iou.t, iop.t)
        assert all(o.pads_intact() for o in (cnt, area, iou, iop))
        if g < r["n"]:
            assert torch.equal(cnt.t, r["cnt"].t[g]) and int(area.t[0]) == int(r["area"].t[g])
            assert torch.equal(iou.t.view(torch.int64), r["iou"].t[g].view(torch.int64)) and torch.equal(iop.t.view(torch.int64), r["iop"].t[g].view(torch.int64))


@pytest.mark.parametrize("name", [n for n in FUSED if not tk.CASE[n]["gap"]])
def test_python_route_equals_the_reference(name):
    """`proposal_targets_fused` (its own tables, its host split at more than four ground truths) on the case"""
    from llmseg_amd import targets as ht
    c = tk.CASE[name]
    masks = _dev(tk.masks_of(name), c["misalign"])
    order = None if c["order"] is None else _dev(np.array(c["order"], np.int64))
    res = ht.proposal_targets_fused(masks, order, [torch.from_numpy(g.copy()).to(DEV) for g in tk.gts_of(name)], c["out"])
    assert res is not None
    maps, ious, iops, cnts = res
    assert torch.equal(maps, _fused(name)["out"].t)
    assert ious.shape == iops.shape == (len(c["gts"]), c["K"]) and cnts.shape == (len(c["gts"]), c["K"], 2)
    for g in range(len(c["gts"])):
        _check_targets(name, g, cnts[g], None, ious[g], iops[g])


@pytest.mark.parametrize("name", REFUSED)
def test_beyond_the_limits_the_entry_point_refuses_and_python_falls_back(name):
    from llmseg_amd import targets as ht
    c = tk.CASE[name]
    H, W, K, OS = c["H"], c["W"], c["K"], c["out"]
    masks = _dev(tk.masks_of(name))
    gtp = _resample_gts(name)
    d_first, d_count, d_w, taps = _tables(tk.tables_of(c))
    n = len(c["gts"])
    outs = [Out((K, OS, OS), torch.bfloat16), Out((n, K, 2), torch.int64), Out((n,), torch.int64), Out((n, K), torch.float64), Out((n, K), torch.float64)]
    lib = _lib()
    n0 = lib.llmseg_launch_count()
    rc = lib.llmseg_proposal_targets(_p(masks), None, _p(gtp.t), n, _p(outs[0].t), K, H, W, OS, _p(d_first), _p(d_count), _p(d_w), _p(d_first), _p(d_count), _p(d_w), taps,
                                     _p(outs[1].t), _p(outs[2].t), _p(outs[3].t), _p(outs[4].t), _stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and lib.llmseg_launch_count() == n0 and all(o.untouched() for o in outs)
    gts = [torch.from_numpy(g.copy()).to(DEV) for g in tk.gts_of(name)]
    assert ht.proposal_targets_fused(masks, None, gts, OS) is None
    areas = torch.arange(K, 0, -1, device=DEV)                             # descending: the stable sort keeps the order
    res = ht.proposals_and_targets_dense(masks, areas, gts, top=K, out_size=OS)
    assert res["order"].tolist() == list(range(K))
    _check_maps(name, _bits(res["sam_segs"]))
    for g in range(n):
        _, rcnt, _, riou, riop = tk.reference(name)["gts"][g]
        assert np.array_equal(res["sam_ious"][g].cpu().numpy(), riou, equal_nan=True) and np.array_equal(res["sam_iops"][g].cpu().numpy(), riop, equal_nan=True)


# ------------------------------------------------------------ standalone kernels ------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(tk.RESIZE_CASES))
def test_resize_aa(tag):
    K, H, W, OS = tk.RESIZE_CASES[tag]
    segs, tabs = tk.standalone_masks(tag, K, H, W), tk.aa_tables(max(H, W), OS)
    lo, hi = tk.map_bounds(tk.exact_maps(segs, OS, tabs), tabs[3])
    d_first, d_count, d_w, taps = _tables(tabs)
    out = Out((K, OS, OS), torch.bfloat16)
    assert _lib().llmseg_resize_aa(_p(_dev(segs)), _p(out.t), K, H, W, OS, _p(d_first), _p(d_count), _p(d_w), _p(d_first), _p(d_count), _p(d_w), taps, _stream()) == 0
    torch.cuda.synchronize()
    assert tk.maps_agree(_bits(out.t), lo, hi) == 0 and out.pads_intact()


@pytest.mark.parametrize("tag", sorted(tk.MASK_TARGET_CASES))
def test_mask_targets(tag):
    K, H, W, Hg, Wg = tk.MASK_TARGET_CASES[tag]
    segs, gt = tk.standalone_masks(tag, K, H, W), tk.standalone_gt(tag, Hg, Wg)
    rcnt, rarea, riou, riop = tk.ref_counts(segs, tk.ref_gtp(gt, H, W))
    cnt, area, iou, iop = Out((K, 2), torch.int64), Out((1,), torch.int64), Out((K,), torch.float64), Out((K,), torch.float64)
    cnt.t.zero_(); area.t.zero_()
    args = (_p(_dev(segs)), _p(_dev(gt)), _p(_nearest(H, Hg)), _p(_nearest(W, Wg)), K, H, W, Hg, Wg, _p(cnt.t), _p(area.t), _p(iou.t), _p(iop.t), _stream())
    assert _lib().llmseg_mask_targets(*args) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cnt.t.cpu().numpy(), rcnt) and int(area.t[0]) == rarea
    assert np.array_equal(iou.t.cpu().numpy(), riou, equal_nan=True) and np.array_equal(iop.t.cpu().numpy(), riop, equal_nan=True)
    assert _lib().llmseg_mask_targets(*args) == 0                          # counts and area accumulate (the caller zero-fills): a second call doubles them
    torch.cuda.synchronize()
    assert np.array_equal(cnt.t.cpu().numpy(), 2 * rcnt) and int(area.t[0]) == 2 * rarea
    assert all(o.pads_intact() for o in (cnt, area, iou, iop))


@pytest.mark.parametrize("tag", sorted(tk.GT_RESAMPLE_CASES))
def test_gt_resample(tag):
    H, W, Hg, Wg = tk.GT_RESAMPLE_CASES[tag]
    gt = tk.standalone_gt(tag, Hg, Wg)
    out = Out((H, W), torch.uint8)
    assert _lib().llmseg_gt_resample(_p(_dev(gt)), _p(_nearest(H, Hg)), _p(_nearest(W, Wg)), _p(out.t), H, W, Hg, Wg, _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.t.cpu().numpy(), tk.ref_gtp(gt, H, W)) and out.pads_intact()


@pytest.mark.parametrize("name", sorted(tk.rle_cases()))
@pytest.mark.parametrize("hwk", [False, True], ids=["khw", "hwk"])
def test_rle_decode(name, hwk):
    H, W, runs = tk.rle_cases()[name]
    ends, offs = tk.rle_inputs(name)
    ref = tk.rle_reference(name, hwk)
    out = Out(ref.shape, torch.uint8)
    assert _lib().llmseg_rle_decode(_p(_dev(ends.view(np.int32))), _p(_dev(offs)), _p(out.t), len(runs), H, W, 1 if hwk else 0, _stream()) == 0
    torch.cuda.synchronize()
    got = out.t.cpu().numpy()
    assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} of {ref.size} bytes differ"
    assert out.pads_intact()


@pytest.mark.parametrize("name", sorted(tk.IU_CASES))
def test_intersection_union(name):
    pred, tgt = tk.iu_inputs(name)
    ignore = tk.IU_CASES[name][1]
    ref = tk.iu_reference(pred, tgt, ignore)
    out = Out((6,), torch.int64)
    out.t.zero_()
    d_pred, d_tgt = _dev(pred), _dev(tgt)
    lib = _lib()
    assert lib.llmseg_intersection_union(_p(d_pred), _p(d_tgt), len(pred), ignore, _p(out.t), _stream()) == 0
    torch.cuda.synchronize()
    assert out.t.tolist() == ref.tolist()
    assert lib.llmseg_intersection_union(_p(d_pred), _p(d_tgt), len(pred), ignore, _p(out.t), _stream()) == 0      # accumulates
    torch.cuda.synchronize()
    assert out.t.tolist() == (2 * ref).tolist() and out.pads_intact()


@pytest.mark.parametrize("name", sorted(tk.URI_CASES))
def test_union_resize_iou(name):
    """`select` bytes {0, 1, 2, 255}: the header's contract is select[k] != 0"""
    segs, sel, gt, (oh, ow), ignore = tk.uri_inputs(name)
    ref = tk.uri_reference(segs, sel, gt, (oh, ow), ignore)
    H, W, K = segs.shape
    out = Out((6,), torch.int64)
    out.t.zero_()
    rc = _lib().llmseg_union_resize_iou(_p(_dev(segs)), _p(_dev(sel)), _p(_dev(gt)), H, W, K, gt.shape[0], gt.shape[1], oh, ow, ignore, _p(out.t), _stream())
    assert rc == 0, _lib().llmseg_last_error()
    torch.cuda.synchronize()
    assert out.t.tolist() == ref.tolist(), f"{name}: {out.t.tolist()} != {ref.tolist()} (select bytes {sorted(set(sel.tolist()))})"
    assert out.pads_intact()


# ----------------------------------------------------------------- refusals -----------------------------------------------------------------
def _refusals():
    """-> [(label, entry point, argument names, valid arguments, output names, [(what, {argument: value})])].  Buffers have the sizes the LIMIT variants
    claim, so that a check that were missing could not write out of bounds."""
    K, H, W, Hg, Wg, OS, T = 2, 4, 2049, 3, 5, 257, 29
    u8 = lambda *s: torch.ones(s, device=DEV, dtype=torch.uint8)
    i32 = lambda n: torch.zeros((n,), device=DEV, dtype=torch.int32)
    ny, wgt = torch.ones((OS,), device=DEV, dtype=torch.int32), torch.ones((OS, T), device=DEV, dtype=torch.float64)
    res = []
    a = dict(run_ends=torch.tensor([3, H * W], device=DEV, dtype=torch.int32).repeat(K), offsets=torch.tensor([0, 2, 4], device=DEV), out=Out((K, H, W), torch.uint8),
             K=K, H=H, W=W, hwk=0)
    res.append(("rle_decode", "llmseg_rle_decode", list(a), a, ["out"],
                [(f"{k} NULL", {k: None}) for k in ("run_ends", "offsets", "out")] + [(f"{k} = 0", {k: 0}) for k in ("K", "H", "W")] + [("H W = 2^32", {"H": 65536, "W": 65536})]))
    a = dict(gt=u8(Hg, Wg), gy=i32(H), gx=i32(W), out=Out((H, W), torch.uint8), H=H, W=W, Hg=Hg, Wg=Wg)
    res.append(("gt_resample", "llmseg_gt_resample", list(a), a, ["out"],
                [(f"{k} NULL", {k: None}) for k in ("gt", "gy", "gx", "out")] + [(f"{k} = 0", {k: 0}) for k in ("H", "W", "Hg", "Wg")]))
    a = dict(segs=u8(K, H, W), gt=u8(Hg, Wg), gy=i32(H), gx=i32(W), K=K, H=H, W=W, Hg=Hg, Wg=Wg, counts=Out((K, 2), torch.int64), gt_area=Out((1,), torch.int64),
             iou=Out((K,), torch.float64), iop=Out((K,), torch.float64))
    outs = ["counts", "gt_area", "iou", "iop"]
    res.append(("mask_targets", "llmseg_mask_targets", list(a), a, outs,
                [(f"{k} NULL", {k: None}) for k in ["segs", "gt", "gy", "gx"] + outs] + [(f"{k} = 0", {k: 0}) for k in ("K", "H", "W", "Hg", "Wg")]))
    a = dict(segs=u8(K, H, W), out=Out((K, OS, OS), torch.bfloat16), K=K, H=H, W=W, out_size=OS, y0=i32(OS), ny=ny, wy=wgt, x0=i32(OS), nx=ny, wx=wgt, taps=T)
    res.append(("resize_aa", "llmseg_resize_aa", list(a), a, ["out"],
                [(f"{k} NULL", {k: None}) for k in ("segs", "out", "y0", "ny", "wy", "x0", "nx", "wx")] + [(f"{k} = 0", {k: 0}) for k in ("K", "H", "W", "out_size", "taps")]))
    G = 5
    a = dict(masks=u8(K, H, W), order=None, gtp=u8(G, H, W), n_gt=1, out=Out((K, OS, OS), torch.bfloat16), K=K, H=H, W=2048, out_size=256, y0=i32(OS), ny=ny, wy=wgt,
             x0=i32(OS), nx=ny, wx=wgt, taps=28, counts=Out((G, K, 2), torch.int64), gt_area=Out((G,), torch.int64), iou=Out((G, K), torch.float64),
             iop=Out((G, K), torch.float64))
    res.append(("proposal_targets", "llmseg_proposal_targets", list(a), a, ["out"] + outs,
                [(f"{k} NULL", {k: None}) for k in ("masks", "out", "y0", "ny", "wy", "x0", "nx", "wx")]
                + [(f"{k} = 0", {k: 0}) for k in ("K", "H", "W", "out_size", "taps")]
                + [("out_size 257", {"out_size": 257}), ("taps 29", {"taps": 29}), ("W 2049", {"W": 2049}), ("n_gt 5", {"n_gt": 5}), ("n_gt -1", {"n_gt": -1})]
                + [(f"n_gt 1 with {k} NULL", {k: None}) for k in ["gtp"] + outs]))
    n = 5000
    a = dict(pred=u8(n), target=u8(n), n=n, ignore_index=255, out=Out((6,), torch.int64))
    res.append(("intersection_union", "llmseg_intersection_union", list(a), a, ["out"], [(f"{k} NULL", {k: None}) for k in ("pred", "target", "out")] + [("n = 0", {"n": 0}), ("n = -1", {"n": -1})]))
    a = dict(segs=u8(H, W, K), select=u8(K), gt=u8(Hg, Wg), H=H, W=W, K=K, Hg=Hg, Wg=Wg, out_h=7, out_w=9, ignore_index=255, out=Out((6,), torch.int64))
    res.append(("union_resize_iou", "llmseg_union_resize_iou", list(a), a, ["out"],
                [(f"{k} NULL", {k: None}) for k in ("segs", "select", "gt", "out")] + [(f"{k} = 0", {k: 0}) for k in ("H", "W", "K", "Hg", "Wg", "out_h", "out_w")]))
    return res


def test_refused_calls_write_nothing_and_launch_nothing():
    lib = _lib()
    conv = lambda v: _p(v.t) if isinstance(v, Out) else _p(v) if torch.is_tensor(v) else v
    seen = 0
    for label, fn, names, valid, outs, variants in _refusals():
        for what, change in variants:
            args = dict(valid, **change)
            n0 = lib.llmseg_launch_count()
            rc = getattr(lib, fn)(*[conv(args[k]) for k in names], _stream())
            assert rc == EINVAL, f"{label}: {what} was not refused (returned {rc})"
            assert lib.llmseg_launch_count() == n0, f"{label}: {what} launched"
            torch.cuda.synchronize()
            assert all(valid[o].untouched() for o in outs), f"{label}: {what} wrote to an output"
            assert lib.llmseg_last_error(), label
            seen += 1
    assert seen == 80
    # the table's valid arguments are valid: the limits themselves (W 2048, out 256, taps 28) are taken
    label, fn, names, valid, outs, _ = [r for r in _refusals() if r[0] == "proposal_targets"][0]
    valid["y0"][:] = 0
    n0 = lib.llmseg_launch_count()
    assert getattr(lib, fn)(*[conv(valid[k]) for k in names], _stream()) == 0, lib.llmseg_last_error()
    torch.cuda.synchronize()
    assert lib.llmseg_launch_count() == n0 + 2 and all(valid[o].pads_intact() for o in outs)
