"""CPU: the tables of tests/image_kernel_checks.py.  The restatements against Pillow on every swept pair and every case shape; the mutant switchboard without
a mutant against the pinned references; every mutant changes something on every case it is declared for and every case is hit by a mutant; why the GPU file reads
the tap tables (an LSB on one table row changes no byte of the older image comparisons)."""
import collections

import numpy as np
import pytest

from tests import image_frontend_checks as fc
from tests import image_kernel_checks as kc

_TAB = {}


def _ref_tab(filt, i, o):
    if (filt, i, o) not in _TAB:
        _TAB[(filt, i, o)] = kc.ref_coeffs(filt, i, o)
    return _TAB[(filt, i, o)]


def _all_pairs(filt):
    return sorted(set(kc.sweep_pairs(filt) + kc.vertical_pairs(filt)))


def _report(title, smallest):
    print(f"\n{title}")
    for k in sorted(smallest):
        print(f"  {k:12s} smallest effect {smallest[k][0]:6d}  at {smallest[k][1]}  ({smallest[k][2]} cases)")


def test_the_limits_are_where_the_kernels_put_them():
    assert kc.ksize(kc.BILINEAR, 31, 1) == 63 and kc.ksize(kc.BILINEAR, 32, 1) == 65 and kc.ksize(kc.BILINEAR, 64, 2) == 65
    assert kc.ksize(kc.BICUBIC, 127, 2) == 255 and kc.ksize(kc.BICUBIC, 63, 1) == 253 and kc.ksize(kc.BICUBIC, 128, 2) == 257 and kc.ksize(kc.BICUBIC, 64, 1) == 257
    for filt in kc.FILTERS:
        assert all(kc.ksize(filt, i, o) <= kc.MAX_KSIZE[filt] for i, o in _all_pairs(filt))
        assert all(kc.ksize(filt, i, o) > kc.MAX_KSIZE[filt] for i, o in kc.BOUNDARY_REFUSED[filt])
        for i, o in _all_pairs(filt):
            assert _ref_tab(filt, i, o)[2].shape[1] == kc.ksize(filt, i, o)
    refused = sorted(c.name for c in kc.resample_cases() if kc.case_refused(c))
    # the kernels take at most 64 (bilinear) and 256 (bicubic) table columns: these shapes of the list are refusals, and the GPU file checks them as such
    assert refused == ["bicubic-255x2-4x2-c1", "bilinear-127x3-2x3-c3", "bilinear-1x63-1x1-c3", "bilinear-255x2-4x2-c1", "bilinear-37x1-1x1-c3",
                       "bilinear-37x53-1x1-c3", "bilinear-3x127-3x2-c1", "bilinear-9x300-9x7-c3"]


@pytest.mark.parametrize("filt", kc.FILTERS, ids=[kc.FNAME[f] for f in kc.FILTERS])
def test_restatement_equals_pillow_on_every_swept_pair(filt):
    Image = pytest.importorskip("PIL.Image")
    res = Image.BILINEAR if filt == kc.BILINEAR else Image.BICUBIC
    rows = 0
    for n, (i, o) in enumerate(_all_pairs(filt)):
        a = np.random.default_rng(n).integers(0, 256, (1, i, 3), dtype=np.uint8)
        assert np.array_equal(kc.ref_resize(filt, a, 1, o), np.array(Image.fromarray(a).resize((o, 1), res))), (i, o)
        t = np.ascontiguousarray(a.transpose(1, 0, 2))
        assert np.array_equal(kc.ref_resize(filt, t, o, 1), np.array(Image.fromarray(t).resize((1, o), res))), (i, o)
        rows += o
    print(f"\n{kc.FNAME[filt]}: {len(_all_pairs(filt))} pairs, {rows} output indices, as a row and as a column")


def test_restatement_equals_pillow_on_every_case_shape():
    """2 and 4 channels channel by channel as `L` images: Pillow premultiplies LA / RGBA, the kernel resamples every channel on its own"""
    Image = pytest.importorskip("PIL.Image")
    for c in kc.resample_cases():
        img = kc.make_input(c)[3]
        res = Image.BILINEAR if c.filt == kc.BILINEAR else Image.BICUBIC
        ref = np.stack([np.array(Image.fromarray(np.ascontiguousarray(img[..., k])).resize((c.ow, c.oh), res)) for k in range(c.ch)], -1)
        assert np.array_equal(kc.ref_resize(c.filt, img, c.oh, c.ow), ref), c.name


@pytest.mark.parametrize("filt", kc.FILTERS, ids=[kc.FNAME[f] for f in kc.FILTERS])
def test_table_mutants(filt):
    smallest, hit = {}, collections.Counter()
    pairs = [(i, o) for i, o in _all_pairs(filt) if i != o]
    for (i, o) in pairs:
        ref = _ref_tab(filt, i, o)
        assert kc.table_diff(kc.taps_m(filt, i, o), ref) == 0, (i, o)
        for mut in kc.TABLE_MUTANTS:
            if not kc.table_mutant_applies(mut, filt, i, o):
                continue
            d = kc.table_diff(kc.taps_m(filt, i, o, mut), ref)
            assert d >= 1, f"{kc.TABLE_MUTANTS[mut]} leaves the {kc.FNAME[filt]} table of {i} -> {o} unchanged"
            hit[(i, o)] += 1
            s = smallest.get(mut, (1 << 60, None, 0))
            smallest[mut] = (min(s[0], d), (i, o) if d < s[0] else s[1], s[2] + 1)
    assert all(hit[p] >= 1 for p in pairs), [p for p in pairs if not hit[p]]
    assert set(smallest) == {m for m in kc.TABLE_MUTANTS if filt == kc.BICUBIC or m not in ("support", "a075", "neground")}
    _report(f"{kc.FNAME[filt]} table mutants over {len(pairs)} pairs (table entries that differ)", smallest)


def _bicubic_with_tables(img, oh, ow, edit):
    h, w = img.shape[:2]
    x = img.astype(np.int64)
    if ow != w:
        x = kc._pass_m(x, edit(fc.coeffs(w, ow)), True, "")
    if oh != h:
        x = kc._pass_m(x, edit(fc.coeffs(h, oh)), False, "")
    return x.astype(np.uint8)


def test_an_lsb_in_the_tables_is_invisible_to_the_image_comparisons():
    """tests/image_frontend_checks.py::RESIZE_CASES (up to 427 x 640 -> 224 x 335, 225 k output bytes): +1 LSB on one tap of one row of each table changes no byte of
    any case; +1 LSB on the first tap of EVERY row, or +0.5 rounding on every negative tap, moves fewer than one byte in a thousand.  Hence the GPU file compares the
    tables themselves."""
    def one_row(t):
        k = t[2].copy(); k[len(k) // 2, 0] += 1
        return t[0], t[1], k

    def every_row(t):
        k = t[2].copy(); k[:, 0] += 1
        return t[0], t[1], k

    print()
    for n, (h, w, oh, ow) in enumerate(fc.RESIZE_CASES):
        a = fc.random_image(h, w, 100 + n)
        ref = fc.resize_bicubic_u8(a, oh, ow)
        assert np.array_equal(_bicubic_with_tables(a, oh, ow, lambda t: t), ref)
        d1 = int((_bicubic_with_tables(a, oh, ow, one_row) != ref).sum())
        d2 = int((_bicubic_with_tables(a, oh, ow, every_row) != ref).sum())
        x = a.astype(np.int64)
        if ow != w:
            x = kc._pass_m(x, kc.taps_m(kc.BICUBIC, w, ow, "neground"), True, "")
        if oh != h:
            x = kc._pass_m(x, kc.taps_m(kc.BICUBIC, h, oh, "neground"), False, "")
        d3 = int((x.astype(np.uint8) != ref).sum())
        print(f"  {h}x{w} -> {oh}x{ow}: {ref.size} bytes; one row +1 LSB {d1}, every row +1 LSB {d2}, +0.5 on negative taps {d3}")
        assert d1 == 0
        if n < 6:                                                              # the six cases that resample more than a few bytes
            assert 1 <= d2 and d2 * 1000 < ref.size and 1 <= d3 and d3 * 1000 < ref.size


def test_resample_cases_and_image_mutants():
    smallest, unhit = {}, []
    cases = [c for c in kc.resample_cases() if not kc.case_refused(c)]
    names = [c.name for c in kc.resample_cases()]
    assert len(set(names)) == len(names)
    for c in cases:
        buf, off, stride, img = kc.make_input(c)
        assert np.array_equal(kc.window(buf, off, stride, c.h, c.w, c.ch), img)
        ref = kc.ref_resize(c.filt, img, c.oh, c.ow)
        assert ref.shape == (c.oh, c.ow, c.ch)
        assert np.array_equal(kc.resample_m(c.filt, buf, off, stride, c.h, c.w, c.ch, c.oh, c.ow), ref), c.name
        hits = 0
        for mut in kc.IMAGE_MUTANTS:
            if not kc.image_mutant_applies(mut, c):
                continue
            d = int((kc.resample_m(c.filt, buf, off, stride, c.h, c.w, c.ch, c.oh, c.ow, mut) != ref).sum())
            assert d >= 1, f"{kc.IMAGE_MUTANTS[mut]} leaves {c.name} unchanged"
            hits += 1
            s = smallest.get(mut, (1 << 60, None, 0))
            smallest[mut] = (min(s[0], d), c.name if d < s[0] else s[1], s[2] + 1)
        if not hits:
            unhit.append(c.name)
    assert not unhit, unhit
    assert set(smallest) == set(kc.IMAGE_MUTANTS)
    _report(f"image mutants over {len(cases)} accepted cases (output bytes that differ)", smallest)


def test_the_case_table_covers_what_it_claims():
    cases = [c for c in kc.resample_cases() if not kc.case_refused(c)]
    for filt in kc.FILTERS:
        mine = [c for c in cases if c.filt == filt]
        for ch in (1, 2, 3, 4):
            odd = [c for c in mine if c.ch == ch and c.extra > 0 and kc.make_input(c)[1] % 2 == 1]
            assert odd, (filt, ch)                                             # a window that starts at an odd byte of an even-aligned buffer
            for want in ("up", "down", "horizontal", "vertical", "copy"):
                assert any(c.ch == ch and want in c.name for c in mine), (filt, ch, want)
        for kind in kc.CONTENTS:
            assert sum(c.content == kind for c in mine) == len(kc.CLASS_SHAPES)
    both = [c for c in cases if c.content.startswith("block") and c.filt == kc.BICUBIC]
    assert any(kc.ref_resize(c.filt, kc.make_input(c)[3], c.oh, c.ow).min() == 0 and kc.ref_resize(c.filt, kc.make_input(c)[3], c.oh, c.ow).max() == 255 for c in both)


def test_clip_cases_and_mutants():
    smallest, unhit, seen = {}, [], collections.Counter()
    for n, (h, w, S) in enumerate(kc.CLIP_CASES):
        img = kc.clip_image(h, w, 300 + n)
        ref = kc.clip_ref_bits(img, S)
        assert ref.shape == (3, S, S) and ref.dtype == np.int16
        assert np.array_equal(kc.clip_m(img, S), ref), (h, w, S)
        nh, nw, top, left = kc.clip_geometry(h, w, S)
        assert (nh, nw) == fc.clip_resized_size(h, w, S)
        seen[("top", top % 2, nh != S)] += 1; seen[("left", left % 2, nw != S)] += 1
        q = S * max(h, w) / min(h, w)
        seen["exact"] += q == int(q) and max(h, w) != min(h, w)
        if nh != h and nh != S:                                                # the window's vertical taps stay clear of both borders
            xmin, cnt, _ = (t[top:top + S] for t in fc.coeffs(h, nh))
            seen["inner"] += int(xmin.min()) > 0 and int((xmin + cnt).max()) < h
        hits = 0
        for mut in kc.CLIP_MUTANTS:
            if not kc.clip_mutant_applies(mut, h, w, S):
                continue
            d = int((kc.clip_m(img, S, mut=mut) != ref).sum())
            assert d >= 1, f"{kc.CLIP_MUTANTS[mut]} leaves clip {h}x{w} -> {S} unchanged"
            hits += 1
            s = smallest.get(mut, (1 << 60, None, 0))
            smallest[mut] = (min(s[0], d), (h, w, S) if d < s[0] else s[1], s[2] + 1)
        if not hits:
            unhit.append((h, w, S))
    assert not unhit, unhit
    for key in (("top", 0, True), ("top", 1, True), ("left", 0, True), ("left", 1, True), "exact", "inner"):
        assert seen[key] >= 1, key
    assert kc.clip_geometry(113, 97, 7)[:2] == (8, 7) and kc.clip_geometry(113, 99, 7)[:2] == (7, 7)
    # u / 255: the IEEE fp32 division is the stated arithmetic on every byte; the product with the fp32 reciprocal shows on U255 alone, at three elements
    u = np.arange(256)
    assert np.array_equal((u.astype(np.float64) * (1.0 / 255.0)).astype(np.float32), u.astype(np.float32) / np.float32(255.0))
    img = kc.u255_image()
    assert all(np.array_equal(np.sort(img[..., c].reshape(-1)), u) for c in range(3))
    ref = kc.clip_ref_bits(img, kc.U255_SIZE, kc.U255_MEAN, kc.U255_STD)
    assert np.array_equal(kc.clip_m(img, kc.U255_SIZE, kc.U255_MEAN, kc.U255_STD), ref)
    d = int((kc.clip_m(img, kc.U255_SIZE, kc.U255_MEAN, kc.U255_STD, mut="u255f32") != ref).sum())
    assert d == 3, d
    assert int((kc.clip_m(img, kc.U255_SIZE, mut="u255f32") != kc.clip_ref_bits(img, kc.U255_SIZE)).sum()) == 0      # invisible under the CLIP statistics
    assert all(float(np.float32(v)) == v for v in kc.U255_MEAN + kc.U255_STD)
    smallest["u255f32"] = (d, "U255", 1)
    assert set(smallest) == set(kc.CLIP_MUTANTS)
    _report(f"CLIP mutants over {len(kc.CLIP_CASES)} cases + U255 (bf16 elements that differ)", smallest)


def test_union_cases_and_mutants():
    import torch
    smallest = {}
    for n in kc.UNION_N:
        for K in kc.UNION_K:
            masks, sel, sel_all = kc.union_case(n, K)
            assert masks.shape[1] * masks.shape[2] == n and set(np.unique(masks)) <= set(kc.MASK_VALUES.tolist())
            assert not sel[0].any() and (sel[1] != 0).sum() == 1 and set(np.unique(sel[3])) - {0, 1} and (sel[1:] != 0).any(1).all()
            hits = 0
            for s, m in ((sel, kc.with_sentinel(masks, sel)), (sel_all, masks)):
                ref = kc.union_m(m, s)
                tm, ts = torch.from_numpy(masks), torch.from_numpy(s)             # the unguarded masks: a sentinel mask shows as a difference here
                exp = torch.stack([tm[ts[c].bool()].any(0) if bool(ts[c].any()) else torch.zeros(tm.shape[1:], dtype=torch.bool) for c in range(s.shape[0])])
                assert np.array_equal(ref, exp.to(torch.uint8).numpy())
                assert set(np.unique(ref)) <= {0, 1}
                for mut in kc.UNION_MUTANTS:
                    if not kc.union_mutant_applies(mut, n, K) or (mut == "neighbour" and s.shape[0] == 1):
                        continue
                    d = int((kc.union_m(m, s, mut) != ref).sum())
                    assert d >= 1, f"{kc.UNION_MUTANTS[mut]} leaves mask_union n={n} K={K} C={s.shape[0]} unchanged"
                    hits += 1
                    k0 = smallest.get(mut, (1 << 60, None, 0))
                    smallest[mut] = (min(k0[0], d), (n, K, s.shape[0]) if d < k0[0] else k0[1], k0[2] + 1)
            assert hits >= 1
            if K == 33:                                                        # some mask is marked by no row, and reading it would show
                m = kc.with_sentinel(masks, sel)
                idle = ~(sel != 0).any(0)
                assert idle.any() and (m[idle] == kc.UNION_SENTINEL).all()
                leak = np.stack([(m[(sel[c] != 0) | idle] != 0).any(0) for c in range(4)]).astype(np.uint8)
                assert (leak != kc.union_m(m, sel)).any()
    assert set(smallest) == set(kc.UNION_MUTANTS)
    _report("mask-union mutants (pixels that differ)", smallest)
