"""CPU: the references, emulations and bounds of tests/amg_kernel_checks.py can fail.  The fp64 restatement of the post-processing is pinned against the
oracle (fp32 F.interpolate) at every geometry, the fp32 emulation of the kernel stays at <= EMU_MAX of the bound, every mutant is rejected by the case
the table names for it, and the conditions the GPU test relies on (n_band <= 4, the preprocess table without double-rounding ties, scipy's labelling
equal to a flood fill) are checked on the references alone.  Run with -s for the figures that profiles/amg_parity.md records."""
import numpy as np
import pytest
import torch

from oracle import amg as oamg, sam_decoder as osd
from tests import amg_kernel_checks as ak

GEOMS = list(range(len(ak.GEOMETRIES)))
GIDS = [ak.geometry_id(g) for g in ak.GEOMETRIES]
_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _SEEN:
        print("\npost-processing, per geometry: oracle (fp32 torch) / bound, emulation / bound, smallest c the emulation needs, worst n_band")
        for k in sorted(_SEEN):
            print(f"  {k:34s} " + "  ".join(f"{v:8.3f}" for v in _SEEN[k]))


# ------------------------------------------------------------- post-processing -------------------------------------------------------------
@pytest.mark.parametrize("gi", GEOMS, ids=GIDS)
def test_post_reference_is_the_oracle_and_the_emulation_is_inside_the_bound(gi):
    g = ak.GEOMETRIES[gi]
    low, ref, bound = ak.logits(gi), ak.reference(gi), ak.post_bound(ak.logits(gi))
    tor = osd.postprocess_masks(torch.from_numpy(low.copy()).view(1, ak.N_LOGITS, 256, 256), g[1], g[2], g[0])[0].numpy()
    assert tor.shape == ref.shape == (ak.N_LOGITS,) + tuple(g[2])
    r_or = float(np.abs(tor - ref).max() / bound)
    emu = ak.post_emulation(low, g)
    r_emu = float(np.abs(emu - ref).max() / bound)
    nb = max(int(ak.band(ref, t, o, bound)[0].max()) for t, o in ak.THRESHOLDS)
    _SEEN[f"{gi} {GIDS[gi]}"] = (r_or, r_emu, r_emu * ak.POST_C, nb)
    # torch's fp32 kernel rounds as often as ours (in another order): a coordinate that differed by one fp32 step would show as hundreds of bounds
    assert r_or <= ak.EMU_MAX, f"the fp64 restatement is not torch's upsample_bilinear2d: {r_or:.3f} of the bound"
    assert r_emu <= ak.EMU_MAX, f"the fp32 emulation is at {r_emu:.3f} of the bound"
    # ... and exactly: the weights F.interpolate uses along each axis of each stage are the restated ones, bit for bit
    for n_in, n_out in {(256, g[0]), (g[1][0], g[2][0]), (g[1][1], g[2][1])}:
        got, want = ak.torch_weights(n_in, n_out)
        assert np.array_equal(got, want), f"{n_in} -> {n_out}: torch's coordinates differ at {np.nonzero(got != want)[0][:5].tolist()}"
    # the nested layout only moves addresses: same bits
    assert np.array_equal(ak.post_emulation(ak.to_nested(low), g, nested=True), emu)
    # the statistics of the emulation agree with the reference's in the sense the GPU test asks for
    for t, o in ak.THRESHOLDS:
        assert ak.stats_agree(ak.stats_of(emu, t, o), ref, t, o, bound) == []


@pytest.mark.parametrize("gi", GEOMS, ids=GIDS)
def test_post_band_is_nearly_empty(gi):
    """a condition on the inputs, from the reference alone: at most N_BAND_MAX pixels of a mask lie within the bound of a threshold"""
    ref, bound = ak.reference(gi), ak.post_bound(ak.logits(gi))
    for t, o in ak.THRESHOLDS:
        nb, _ = ak.band(ref, t, o, bound)
        assert nb.max() <= ak.N_BAND_MAX, f"thresholds ({t}, {o}): {nb.tolist()}"


def test_post_fields_are_what_the_table_says():
    for gi in GEOMS:
        low = ak.logits(gi).reshape(ak.N_LOGITS, 256, 256)
        assert abs(float(np.abs(low[0]).max()) - 12.0) < 1e-5
        assert (low[2] == -5).all() and (low[3] == 5).all()
        inner = low[1][1:-1, 1:-1]
        assert (inner < 0).all() and (low[1][0] > 0).all() and (low[1][-1] > 0).all() and (low[1][:, 0] > 0).all() and (low[1][:, -1] > 0).all()
        st = ak.stats_of(ak.reference(gi), 0.0, 1.0)
        oh, ow = ak.GEOMETRIES[gi][2]
        if max(ak.GEOMETRIES[gi][1][0] / oh, ak.GEOMETRIES[gi][1][1] / ow) <= 4:          # (at 73 : 1 no sample falls on the four-pixel frame)
            assert st[1, 3:].tolist() == [0, 0, ow - 1, oh - 1], "the frame's box must reach every border"
        assert st[2].tolist() == ak.STATS_INIT and st[3, :3].tolist() == [oh * ow] * 3
    # the nested permutation is the one of tests/sam_decoder_checks.py, and _low_addr is its inverse
    r = np.arange(65536, dtype=np.float32).reshape(1, 65536)
    t = torch.from_numpy(r.copy()).view(1, 64, 2, 2, 64, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).reshape(1, 65536).numpy()
    assert np.array_equal(ak.to_nested(r), t)
    Y, X = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(t[0][ak._low_addr(Y, X, True)], r.reshape(256, 256))


@pytest.mark.parametrize("mutant", sorted(ak.POST_MUTANTS))
def test_post_mutants_fail_the_case_that_names_them(mutant):
    gi, nested = ak.POST_MUTANTS[mutant]
    ratio, differ = ak.post_mutant_ratio(mutant, gi, nested)
    print(f"\n{mutant}: {ratio:.3g} of the bound at {GIDS[gi]} nested={nested}, statistics differ: {differ}")
    assert ratio >= ak.MUT_MIN or differ, f"{mutant} passes {GIDS[gi]}"
    if mutant in ("ge_at_threshold", "box_max_exclusive", "box_xy_swapped"):
        assert differ
    else:
        assert ratio >= ak.MUT_MIN


# ------------------------------------------------------------------- NMS -------------------------------------------------------------------
def test_nms_table_is_integer_and_the_restatement_is_the_oracle():
    for name, (b, order, thr, scores) in ak.NMS_CASES.items():
        assert (b == np.round(b)).all() and b.min() >= 0 and b.max() < 4096 and len(order) <= ak.NMS_LIMIT, name
        want = ak.nms_oracle(name)
        assert np.array_equal(order[ak.nms_reference(b, order, thr)], want), name
        if scores is not None:                          # the ranking really is the oracle's own stable sort of tied scores
            assert len(np.unique(scores)) < len(scores)
            assert np.array_equal(oamg.nms(torch.from_numpy(b), torch.from_numpy(scores), thr).numpy(), want), name
    keep = {n: ak.nms_reference(*ak.NMS_CASES[n][:3]).tolist() for n in ak.NMS_CASES if n.startswith("iou_") or "zero_area" in n}
    assert keep["iou_equals_thr_0.5"] == keep["iou_equals_thr_0.25"] == [True, True]
    assert keep["iou_one_step_above_thr_0.5"] == keep["iou_one_step_above_thr_0.25"] == [True, False]
    assert keep["two_identical_zero_area"] == [True, True] and keep["zero_area_boxes"] == [True, True, True, False, True, True]
    assert len(ak.NMS_CASES["n8192_limit"][1]) == ak.NMS_LIMIT
    b, order, _, _ = ak.NMS_CASES["order_is_a_subset"]
    assert len(order) < len(b) and len(set(order.tolist())) == len(order) and order.tolist() != sorted(order.tolist())


def test_nms_oracle_is_torchvision():
    tv = pytest.importorskip("torchvision")
    for name, (b, order, thr, _) in ak.NMS_CASES.items():
        bb = torch.from_numpy(b[order.astype(np.int64)])
        got = tv.ops.nms(bb, -torch.arange(len(order), dtype=torch.float32), thr)
        assert np.array_equal(order[got.numpy()], ak.nms_oracle(name)), name


@pytest.mark.parametrize("mutant", sorted(ak.NMS_MUTANTS))
def test_nms_mutants_fail_the_case_that_names_them(mutant):
    b, order, thr, _ = ak.NMS_CASES[ak.NMS_MUTANTS[mutant]]
    assert not np.array_equal(ak.nms_reference(b, order, thr, mutant), ak.nms_reference(b, order, thr))


# ------------------------------------------------------------- small regions -------------------------------------------------------------
@pytest.mark.parametrize("shape", ak.SHAPES, ids=[f"{h}x{w}" for h, w in ak.SHAPES])
def test_region_restatement_is_the_oracle(shape):
    names, ms = ak.region_masks(shape)
    assert set(np.unique(ms[names.index("blobs_as_0_255")]).tolist()) <= {0, 255}
    for a in ak.MIN_AREAS:
        a = ak.min_area_of(a, shape)
        ref, ch, boxes, areas = ak.region_reference(shape, a)
        for k in range(len(names)):
            f, c = ak.clean_reference(ms[k], a)
            assert np.array_equal(f, ref[k]) and c == ch[k], (names[k], a)
    # min_area above the image: the empty mask is one small hole and comes back full
    ref, ch, _, _ = ak.region_reference(shape, shape[0] * shape[1] + 1)
    assert ref[names.index("empty")].all() and ch[names.index("empty")]


def test_region_patterns_are_what_the_table_says():
    from scipy import ndimage
    for shape in ak.SHAPES:
        names, ms = ak.region_masks(shape)
        H, W = shape
        if H > 1 and W > 1:
            for n in ("checkerboard", "serpentine", "spiral", "zigzag"):
                m = ms[names.index(n)] != 0
                assert ndimage.label(m, structure=ak._FULL8)[1] == 1, (shape, n)
            assert ndimage.label(ms[names.index("checkerboard")] == 0, structure=ak._FULL8)[1] == 1
            assert ms[names.index("serpentine")].sum() >= (H // 2) * W
            z = ms[names.index("zigzag")] != 0
            assert ndimage.label(z, structure=ak._CROSS4)[1] == H
            if W > 256:
                assert z[0, 255] and z[1, 256]
        if "exact_sizes" in names:
            m = ms[names.index("exact_sizes")] != 0
            for fg in (m, ~m):
                lab, n = ndimage.label(fg, structure=ak._FULL8)
                sizes = set(np.bincount(lab.ravel())[1:].tolist())
                assert set(ak.RUNS) <= sizes, (shape, sorted(sizes))
        for n, want in (("small_strict_largest", [1, 3, 2]), ("small_tie_of_two", [3, 3, 1]), ("small_tie_of_three", [2, 3, 3, 3])):
            if n in names:
                lab, k = ndimage.label(ms[names.index(n)] != 0, structure=ak._FULL8)
                assert np.bincount(lab.ravel())[1:].tolist() == want                  # (labels are numbered by first pixel in raster order)
                if H > 1 and W > 1:
                    firsts = [np.argwhere(lab == i + 1)[0] for i in range(k)]
                    assert all(firsts[i][1] > firsts[i + 1][1] for i in range(k - 1)), "raster order must differ from order by column"


def test_scipy_labelling_is_a_flood_fill():
    """the oracle's connected components (scipy, 8-connectivity, labels by first pixel in raster order) against a plain flood fill, three smallest cases"""
    from scipy import ndimage
    for shape in [(1, 1), (1, 300), (300, 1)]:
        _, ms = ak.region_masks(shape)
        for m in ms:
            for fg in (m != 0, m == 0):
                lab, n = ndimage.label(fg, structure=ak._FULL8)
                flab, sizes = ak.flood_fill_labels(fg)
                assert np.array_equal(lab, flab) and np.bincount(lab.ravel(), minlength=n + 1)[1:].tolist() == sizes
    # and once in two dimensions, diagonal contacts included
    m = ak.region_masks((64, 257))[1][ak.region_masks((64, 257))[0].index("blobs")][:24, 230:257] != 0
    assert np.array_equal(ndimage.label(m, structure=ak._FULL8)[0], ak.flood_fill_labels(m)[0])


@pytest.mark.parametrize("mutant", sorted(ak.REGION_MUTANTS))
def test_region_mutants_fail_the_case_that_names_them(mutant):
    shape, pattern, a = ak.REGION_MUTANTS[mutant]
    a = ak.min_area_of(a, shape)
    names, ms = ak.region_masks(shape)
    m = ms[names.index(pattern)]
    f0, c0 = ak.clean_reference(m, a)
    f1, c1 = ak.clean_reference(m, a, mutant)
    assert not np.array_equal(f0, f1) or c0 != c1


# -------------------------------------------------------------- sam_preprocess --------------------------------------------------------------
def test_preprocess_fp32_route_rounds_like_fp64_on_all_768_pairs():
    t64, t32 = ak.pre_table()
    assert t64.shape == (256, 3)
    differ = {(int(v), int(c)): (int(t64[v, c]), int(t32[v, c])) for v, c in np.argwhere(t64 != t32)}
    assert differ == ak.PRE_TIES, f"(value, channel) -> (fp64 bits, fp32 bits): {differ}"
    # the one-rounding conversion is torch's on values that need no second rounding
    x = torch.randn(4096, dtype=torch.float32)
    assert np.array_equal(ak.bf16_bits(x.double().numpy()), x.to(torch.bfloat16).view(torch.int16).numpy())
    for (h, w), S in ak.PRE_SIZES:
        img = ak.pre_image(h, w)
        if h * w >= 256:
            assert all(len(np.unique(img[:, :, c])) == 256 for c in range(3))
        ref = ak.pre_reference(h, w, S)
        assert (ref[:, h:, :] == 0).all() and (ref[:, :, w:] == 0).all()


def test_every_mutant_table_names_a_case():
    """walks the three mutant tables: each entry names an existing case, and that case rejects it"""
    for mutant, (gi, nested) in ak.POST_MUTANTS.items():
        ratio, differ = ak.post_mutant_ratio(mutant, gi, nested)
        assert ratio >= ak.MUT_MIN or differ, mutant
    for mutant, case in ak.NMS_MUTANTS.items():
        b, order, thr, _ = ak.NMS_CASES[case]
        assert not np.array_equal(ak.nms_reference(b, order, thr, mutant), ak.nms_reference(b, order, thr)), mutant
    for mutant, (shape, pattern, a) in ak.REGION_MUTANTS.items():
        names, ms = ak.region_masks(shape)
        m, a = ms[names.index(pattern)], ak.min_area_of(a, shape)
        assert ak.clean_reference(m, a)[0].tolist() != ak.clean_reference(m, a, mutant)[0].tolist(), mutant
