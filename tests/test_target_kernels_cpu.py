"""CPU: the tables, references, emulations and mutants of tests/target_kernel_checks.py can fail.  The exact map reference is pinned to the oracle
(torch's antialiased float64 interpolate) inside a stated float64 rounding bound, the integer references are the oracle's, the structural emulation of
the fused kernel (and of its fallback and host split) equals the reference at every case, every mutant is rejected by the case the table names for it,
and the conditions the GPU test relies on (every case reaches the branch it is there for, set pixels on every slice boundary, at most 0.01 % undecided
pixels) hold on the references alone.  Run with -s for the figures that profiles/target_parity.md records."""
import numpy as np
import pytest
import torch

from oracle import metric as ometric, targets as ot
from tests import target_kernel_checks as tk

NAMES = [c["name"] for c in tk.CASES]
_PIN = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _PIN:
        print("\ncase                    HxW -> out      K  taps ring ns staging   weights   fused  undecided  |torch - exact| max, / bound")
        for n in NAMES:
            if n in _PIN:
                print("  " + _PIN[n])


def _staging(c):
    return "vector" if c["W"] % 16 == 0 and not c["misalign"] else "scalar"


# ------------------------------------------------------------------ the table ------------------------------------------------------------------
def test_every_case_reaches_the_branch_it_is_there_for():
    taps = {n: tk.tables_of(tk.CASE[n])[3] for n in NAMES}
    ns = {n: tk.n_slices(tk.CASE[n]["K"], tk.CASE[n]["out"]) for n in NAMES}
    assert taps["w40_scalar_staging"] == 7 and _staging(tk.CASE["w40_scalar_staging"]) == "scalar" and _staging(tk.CASE["w48_vector"]) == "vector"
    assert _staging(tk.CASE["w48_base_plus_8"]) == "scalar" and np.array_equal(tk.masks_of("w48_base_plus_8"), tk.masks_of("w48_vector"))
    assert (taps["side80_11taps"], taps["side81_13taps"], taps["side112_15taps"], taps["side208_27taps"], taps["side209_29taps"]) == (11, 13, 15, 27, 29)
    assert tk.ring_of(11) == 16 and tk.ring_of(12) == 16 and tk.ring_of(13) == 32 and tk.ring_of(27) == 32
    assert tk.fused_takes(tk.CASE["side208_27taps"]) and not tk.fused_takes(tk.CASE["side209_29taps"])
    assert (ns["out48_k2"], ns["out40_k3"], ns["out100_k1"], ns["out48_k400"], ns["w40_scalar_staging"]) == (3, 2, 6, 2, 1)
    assert sorted({b - a for a, b, _, _ in tk.slice_rows(tk.CASE["out100_k1"])}) == [16, 17]
    assert tk.slice_rows(tk.CASE["pad_below_8x64"])[1][2] >= tk.slice_rows(tk.CASE["pad_below_8x64"])[1][3] == 8                          # owns no rows
    assert taps["up_10x12"] == 3 and ns["up_10x12"] == 2 and len(set(tk.tables_of(tk.CASE["up_10x12"])[0].tolist())) < 32                # repeated y0
    assert taps["w2048"] == 17 and int(tk.tables_of(tk.CASE["w2048"])[0].max()) == 2036 and tk.fused_takes(tk.CASE["w2048"]) and not tk.fused_takes(tk.CASE["w2049"])
    assert [len(tk.CASE[n]["gts"]) for n in ("gt0", "gt4", "gt5", "gt9")] == [0, 4, 5, 9]
    # the tail: rows 76 .. 79 of slice 0 are owned, and no window of the slice reaches them (the last one ends at 76, staged in fours from 0)
    (a, b, ca, cb) = tk.slice_rows(tk.CASE["gap5_tail"])[0]
    y0, ny = tk.tables_of(tk.CASE["gap5_tail"])[:2]
    assert (ca, cb) == (0, 80) and int(y0[b - 1] + ny[b - 1]) == 76
    # with antialiasing tables the tail is unreachable: the last window of a slice reaches the first row of the next slice
    for n in NAMES:
        c = tk.CASE[n]
        if c["gap"]:
            continue
        y0, ny = tk.tables_of(c)[:2]
        for (a, b, ca, cb) in tk.slice_rows(c):
            assert min(c["H"], int(y0[b - 1] + ny[b - 1])) >= cb, n
    # byte values, orders
    assert set(np.unique(tk.masks_of("bytes_odd"))) == {0, 2, 0x10, 0x7f, 0x80} and set(np.unique(tk.masks_of("bytes_0_255"))) == {0, 255}
    assert sorted(tk.CASE["order_perm"]["order"]) == list(range(5)) and len(set(tk.CASE["order_dup"]["order"])) < 5 and len(tk.CASE["order_drop"]["order"]) < 6
    for n in ("gt4", "gt5", "gt9"):
        assert set(np.unique(np.concatenate([g.reshape(-1) for g in tk.gts_of(n)]))) == {0, 1, 2, 255}
        assert not tk.gts_of(n)[-1].any()                                  # an empty ground truth
        sh = [g.shape for g in tk.gts_of(n)]
        H, W = tk.CASE[n]["H"], tk.CASE[n]["W"]
        assert any(h > H and w > W for h, w in sh) and any(h < H for h, w in sh) and any(w < W for h, w in sh)
    assert tk.gts_of("gt5")[3].shape == (1, 1)
    assert not tk.masks_of("gt4")[1].any()                                 # an empty proposal: 0 / 0


@pytest.mark.parametrize("name", NAMES)
def test_slice_boundaries_carry_set_pixels(name):
    """a row counted twice or dropped at a slice boundary must change |seg| and |seg & gt'|: both boundary rows hold set pixels of proposal 0 and
    (with a ground truth) of gt' on them"""
    c = tk.CASE[name]
    segs = tk.selected(name)
    for (_, _, ca, _) in tk.slice_rows(c)[1:]:
        for y in (ca - 1, ca):
            if 0 <= y < c["H"]:
                assert (segs[0, y] != 0).any(), (name, y)
                if name in ("out48_k2", "out100_k1", "out40_k3"):
                    gtp = tk.reference(name)["gts"][0][0]
                    assert ((segs[0, y] != 0) & (gtp[y] != 0)).any(), (name, y)


# ---------------------------------------------------------------- references ----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reference_is_the_oracle_and_nearly_every_pixel_is_decided(name):
    c, ref = tk.CASE[name], tk.reference(name)
    tabs = tk.tables_of(c)
    taps = tabs[3]
    assert ref["undecided"] <= tk.UNDECIDED_MAX, f"{ref['undecided']:.2e} of the pixels are undecided: choose other masks"
    line = (f"{name:22s} {c['H']:4d}x{c['W']:<4d} -> {c['out']:3d} {c['K']:4d} {taps:4d} {tk.ring_of(taps):4d} {tk.n_slices(c['K'], c['out']):3d} {_staging(c):8s} "
            f"{'register' if taps <= tk.TG_WREG else 'scalar':9s} {str(tk.fused_takes(c)):6s} {ref['undecided']:.1e}")
    if not c["gap"]:
        # the exact value against torch's own float64 kernel, before any bf16 rounding, per pixel inside the float64 bound
        tor = tk.torch_maps(name)
        v = ref["v"]
        d = np.abs(tor.astype(tk.LD) - v)
        bound = tk.LD(tk.torch_pin_terms(taps) * tk.U53) * v
        assert (d <= bound).all(), f"torch's float64 resize is {float((d / np.where(v > 0, bound, 1)).max()):.3f} of the bound away (or non-zero where v = 0)"
        worst = float(np.where(v > 0, d / np.where(v > 0, bound, 1), 0).max())
        line += f"   {float(d.max()):.2e}  {worst:.3f}"
        # and the oracle's bf16 maps lie between the two bounds
        segs = (tk.selected(name) != 0).astype(np.float64)
        side = max(c["H"], c["W"])
        sq = np.pad(segs, ((0, 0), (0, side - c["H"]), (0, side - c["W"]))).transpose(1, 2, 0)
        bits = ot.proposal_maps(np.ascontiguousarray(sq), out=c["out"]).view(torch.int16).numpy()
        assert tk.maps_agree(bits, ref["lo"], ref["hi"]) == 0
    else:
        line += "   (caller tables: no torch counterpart)"
    _PIN[name] = line
    # integer references: the oracle's compute_all_iou_iop on the same masks
    segs = tk.selected(name)
    for g, (gtp, cnt, area, iou, iop) in zip(tk.gts_of(name), ref["gts"]):
        o_iou, o_iop = ot.compute_all_iou_iop(np.ascontiguousarray((segs != 0).transpose(1, 2, 0)), (g != 0).astype(np.uint8))
        assert np.array_equal(iou, o_iou, equal_nan=True) and np.array_equal(iop, o_iop, equal_nan=True)
        assert area == int(gtp.sum()) and gtp.shape == (c["H"], c["W"])
    if name == "gt4":
        iou, iop = ref["gts"][-1][3], ref["gts"][-1][4]
        assert np.isnan(iou[1]) and np.isnan(iop[1]) and not np.isnan(iop[0]) and iou[0] == 0      # empty proposal and empty ground truth: 0 / 0


def test_nearest_rule_is_scipy_zoom():
    """the restated skimage order-0 rule against scipy.ndimage.zoom(order=0, grid_mode=True), at the shapes of the table"""
    from scipy.ndimage import zoom
    for (H, W, Hg, Wg) in list(tk.GT_RESAMPLE_CASES.values()) + [(24, 40, 48, 80), (24, 40, 12, 20), (24, 40, 36, 28)]:
        g = np.arange(Hg * Wg, dtype=np.float64).reshape(Hg, Wg)
        want = zoom(g, (H / Hg, W / Wg), order=0, mode="grid-constant", grid_mode=True)
        assert want.shape == (H, W) and np.array_equal(ot.resize_nearest(g, H, W), want), (H, W, Hg, Wg)
        assert np.array_equal(tk.emulate_nearest_index(H, Hg), np.clip(want[:, 0] // Wg, 0, Hg - 1).astype(np.int32))


# ---------------------------------------------------------- emulation and mutants ----------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_emulation_equals_the_reference(name):
    bad = tk.route_differs(name, tk.emulate_route(name))
    assert bad == [], bad
    c = tk.CASE[name]                                                      # the three-kernel route on the same case
    bits = tk.to_bf16_bits(tk.emulate_resize_aa(tk.selected(name), c["out"], tk.tables_of(c)))
    assert tk.maps_agree(bits, tk.reference(name)["lo"], tk.reference(name)["hi"]) == 0


@pytest.mark.parametrize("mutant", sorted(tk.ROUTE_MUTANTS))
def test_route_mutants_fail_the_case_that_names_them(mutant):
    name = tk.ROUTE_MUTANTS[mutant]
    bad = tk.route_differs(name, tk.emulate_route(name, mut=mutant))
    print(f"\n{mutant:30s} {name:22s} {'; '.join(bad)}")
    assert bad, f"{mutant} passes {name}"


def test_ring_of_16_rows_is_enough_up_to_13_taps():
    """RING 16 at 13 taps is not a defect one can observe: windows of ny rows plus the three rows staged ahead occupy ny + 3 ring rows, and at 13 taps
    ny <= 11 (side 81 -> 16).  The forced-RING-16 mutant therefore passes the 13-tap case; it fails at 15 taps (ny = 14) and at 27."""
    assert int(tk.tables_of(tk.CASE["side81_13taps"])[1].max()) <= 13 and int(tk.tables_of(tk.CASE["side112_15taps"])[1].max()) == 14
    assert tk.route_differs("side81_13taps", tk.emulate_route("side81_13taps", mut="ring16_always")) == []
    assert tk.route_differs("side112_15taps", tk.emulate_route("side112_15taps", mut="ring16_always"))


def test_lds_junk_matters():
    """the emulation's LDS starts full of junk: a kernel that read a byte or a ring row nobody wrote would not equal the reference.  Shown by the two
    mutants that do read them: their maps turn wrong (junk bytes weigh) or NaN (ring rows)."""
    bits = tk.emulate_route("pad_right_64x8", mut="tap_beyond_w_weighs")[0]
    assert tk.maps_agree(bits, tk.reference("pad_right_64x8")["lo"], tk.reference("pad_right_64x8")["hi"]) > 0
    val = tk.emulate_fused(tk.masks_of("side208_27taps"), None, None, 208, 160, 16, tk.tables_of(tk.CASE["side208_27taps"]), mut="ring16_always")[0]
    good = tk.emulate_fused(tk.masks_of("side208_27taps"), None, None, 208, 160, 16, tk.tables_of(tk.CASE["side208_27taps"]))[0]
    assert not np.isnan(good).any() and not np.array_equal(val, good)


# ------------------------------------------------------------ standalone kernels ------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(tk.RESIZE_CASES))
def test_resize_cases(tag):
    K, H, W, out = tk.RESIZE_CASES[tag]
    segs, tabs = tk.standalone_masks(tag, K, H, W), tk.aa_tables(max(H, W), out)
    v = tk.exact_maps(segs, out, tabs)
    lo, hi = tk.map_bounds(v, tabs[3])
    assert float((lo != hi).mean()) <= tk.UNDECIDED_MAX
    assert tk.maps_agree(tk.to_bf16_bits(tk.emulate_resize_aa(segs, out, tabs)), lo, hi) == 0
    assert (out > 256) != (tabs[3] > tk.LIMITS["taps"])                    # each is beyond exactly one limit of the fused kernel


@pytest.mark.parametrize("tag", sorted(tk.MASK_TARGET_CASES))
def test_mask_target_cases(tag):
    K, H, W, Hg, Wg = tk.MASK_TARGET_CASES[tag]
    segs, gt = tk.standalone_masks(tag, K, H, W), tk.standalone_gt(tag, Hg, Wg)
    gtp = tk.ref_gtp(gt, H, W)
    cnt, area, iou, iop = tk.ref_counts(segs, gtp)
    o_iou, o_iop = ot.compute_all_iou_iop(np.ascontiguousarray((segs != 0).transpose(1, 2, 0)), (gt != 0).astype(np.uint8))
    assert np.array_equal(iou, o_iou, equal_nan=True) and np.array_equal(iop, o_iop, equal_nan=True)
    e_cnt, e_area = tk.emulate_mask_targets(segs, tk.emulate_gt_resample(gt, H, W))
    assert np.array_equal(e_cnt, cnt) and e_area == area
    m_cnt, m_area = tk.emulate_mask_targets(segs, tk.emulate_gt_resample(gt, H, W, mut="nearest_floor_c"))
    if tag == "hw4097":
        assert not np.array_equal(m_cnt, cnt) or m_area != area


@pytest.mark.parametrize("name", sorted(tk.rle_cases()))
@pytest.mark.parametrize("hwk", [False, True], ids=["khw", "hwk"])
def test_rle_decode_cases(name, hwk):
    ref = tk.rle_reference(name, hwk)
    assert np.array_equal(tk.emulate_rle_decode(name, hwk), ref)
    H, W, runs = tk.rle_cases()[name]
    if name.startswith("short"):
        assert all(sum(r) < H * W for r in runs)
        assert {len(r) & 1 for r in runs} == ({1} if "odd" in name else {0})
    elif name == "37x53_mixed_run_counts":
        assert all(sum(r) == H * W for r in runs) and runs[2][0] == 0 and len(runs[1]) == 1 and len(runs[0]) > 100 * len(runs[4])
    for mut, killer in tk.RLE_MUTANTS.items():
        if killer == name:
            got = tk.emulate_rle_decode(name, hwk, fixed=False) if mut == "parity_beyond_the_last_run" else tk.emulate_rle_decode(name, hwk, mut=mut)
            assert got.shape == ref.shape and not np.array_equal(got, ref), f"{mut} passes {name}"


@pytest.mark.parametrize("name", sorted(n for n in tk.IU_CASES if tk.IU_CASES[n][0] < 10 ** 6))
def test_intersection_union_cases(name):
    pred, tgt = tk.iu_inputs(name)
    ignore = tk.IU_CASES[name][1]
    ref = tk.iu_reference(pred, tgt, ignore)
    assert np.array_equal(tk.emulate_iu(pred, tgt, ignore), ref)
    for mut, killer in tk.IU_MUTANTS.items():
        if killer == name:
            assert not np.array_equal(tk.emulate_iu(pred, tgt, ignore, mut), ref), f"{mut} passes {name}"
    if ignore == 255:                                                      # the restatement is the oracle's; values 2 and 255 appear on both sides
        assert set(np.unique(pred)) <= {0, 1, 2, 7, 255}
        if len(pred) > 1000:
            assert {0, 1, 2, 255} <= set(np.unique(pred)) and {0, 1, 2, 255} <= set(np.unique(tgt))


@pytest.mark.parametrize("name", sorted(tk.URI_CASES))
def test_union_resize_iou_cases(name):
    segs, sel, gt, out_hw, ignore = tk.uri_inputs(name)
    ref = tk.uri_reference(segs, sel, gt, out_hw, ignore)
    assert np.array_equal(tk.emulate_uri(segs, sel, gt, out_hw, ignore), ref)
    for mut, killer in tk.URI_MUTANTS.items():
        if killer == name:
            assert not np.array_equal(tk.emulate_uri(segs, sel, gt, out_hw, ignore, mut), ref), f"{mut} passes {name}"
    kind = tk.URI_CASES[name][8]
    if kind == "bytes":
        assert sel[0] == 2 and (segs[:, :, 0] != 0).any()                  # an even select byte on a proposal that has pixels
    if name == "k300_select_bytes":
        assert sel[256] == 2 and sel[299] == 255 and set(np.unique(sel)) == {0, 1, 2, 255}
    if name == "argmax_form":
        assert out_hw == gt.shape and int((sel != 0).sum()) == 1
        # the oracle's own arg-max body on the same inputs (ignore 255): segs as 0 / 1, similarity = the one-hot row
        i, u, t, _ = ometric.argmax_iou(torch.from_numpy((segs != 0).astype(np.uint8)), torch.from_numpy(sel.astype(np.float32)), torch.from_numpy(gt))
        assert np.array_equal(torch.cat([i, u, t]).long().numpy(), ref)
    assert {0, 1, 2, 255} <= set(np.unique(gt)) or gt.size < 60
