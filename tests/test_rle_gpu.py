"""GPU: the COCO RLE codec on the device (llmseg_rle_encode / llmseg_rle_parse through the C ABI and through llmseg_amd.targets) against the
oracle's restated pycocotools codec (oracle.targets.rle_encode / rle_decode) and the host parse (targets.rle_counts).  Integer work: bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rand(h, w, seed, p=0.5):
    return (np.random.default_rng(seed).random((h, w)) > p).astype(np.uint8)


def _case(name):
    """-> uint8 [K, H, W] (numpy).  Seeds are chosen so that the run counts the tests name hold (checked in the tests)."""
    if name == "37x53":                      # the six masks of tests/test_targets_cpu.py::test_rle_encode_masks_matches_the_restated_pycocotools_codec
        g = torch.Generator().manual_seed(3)
        H, W = 37, 53
        m = (torch.rand(6, H, W, generator=g) > 0.6).to(torch.uint8)
        m[1] = 0
        m[2] = 1
        m[3, 0, 0] = 1
        m[4, :, :20] = 1; m[4, :, 20:] = 0
        m[5] = (torch.rand(H, W, generator=g) > 0.97).to(torch.uint8)
        return m.numpy()
    if name in ("1x1", "1x37", "41x1"):      # degenerate widths / heights: ones, zeros, random
        h, w = (int(v) for v in name.split("x"))
        return np.stack([np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8), _rand(h, w, 5), _rand(h, w, 6, 0.8)])
    if name == "97x130":                     # 6416 counts > the 4096 first-try capacity: the retry; W % 4 != 0; one copy as 0 / 255
        m = _rand(97, 130, 1004)
        return np.stack([m, m * 255])
    if name == "3x2100":                     # 3203 counts: crosses every per-workgroup column chunk
        return _rand(3, 2100, 1)[None]
    if name == "2100x3":                     # 3112 counts: crosses the row segments of a column
        return _rand(2100, 3, 6)[None]
    if name == "1024x1024":                  # empty, full, ones at column-major positions {5, 900000, 900010}
        m = np.zeros((3, 1024, 1024), np.uint8)
        m[1] = 1
        for p in (5, 900000, 900010):
            m[2, p % 1024, p // 1024] = 1
        return m
    if name == "checkerboard":               # 4033 single-pixel runs (63 column boundaries join two equal pixels)
        y, x = np.mgrid[0:64, 0:64]
        return ((x + y) & 1).astype(np.uint8)[None]
    raise KeyError(name)


CASES = ("37x53", "1x1", "1x37", "41x1", "97x130", "3x2100", "2100x3", "1024x1024", "checkerboard")
_REF = {}


def _ref(name):
    """(masks, the oracle's encodings), computed once per case and shared by the tests (never modified)."""
    if name not in _REF:
        from oracle import targets as ot
        m = _case(name)
        _REF[name] = (m, [ot.rle_encode((mk != 0).astype(np.uint8)) for mk in m])
    return _REF[name]


def _host_parse(recs):
    """What `decode_rles` builds on the host: (run_ends uint32, run_offsets int64)."""
    from llmseg_amd import targets as ht
    runs = [ht.rle_counts(r) for r in recs]
    ends = np.concatenate([np.cumsum(r, dtype=np.uint64).astype(np.uint32) for r in runs])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
    return ends, offs


@pytest.mark.parametrize("name", CASES)
def test_encode_equals_the_restated_pycocotools_codec(name):
    from llmseg_amd import targets as ht
    from oracle import targets as ot
    m, ref = _ref(name)
    got = ht.rle_encode_masks(torch.from_numpy(m).to(DEV))
    assert len(got) == len(ref)
    for k in range(len(ref)):
        assert got[k] == ref[k], (name, k, got[k]["counts"][:80], ref[k]["counts"][:80])
        assert type(got[k]["counts"]) is str and type(got[k]["size"][0]) is int
        assert np.array_equal(ot.rle_decode(got[k]), (m[k] != 0).astype(np.uint8))


def test_the_cases_hold_the_runs_they_are_there_for():
    from llmseg_amd import targets as ht
    n = lambda name, k=0: ht.rle_counts(_ref(name)[1][k])
    assert len(n("97x130")) == 6416 and len(n("97x130")) > ht.RLE_CAP_COUNTS          # the retry path runs
    assert len(n("3x2100")) == 3203 and len(n("2100x3")) == 3112 and len(n("checkerboard")) == 4033
    assert n("37x53", 4).tolist() == [0, 740, 1221]                                    # a run across 19 column boundaries
    assert n("1024x1024", 0).tolist() == [1048576] and len(_ref("1024x1024")[1][0]["counts"]) == 5
    assert n("1024x1024", 2).tolist() == [5, 1, 899994, 1, 9, 1, 148565] and len(_ref("1024x1024")[1][2]["counts"]) == 18


def test_encode_of_a_non_contiguous_view_encodes_the_view():
    from llmseg_amd import targets as ht
    from oracle import targets as ot
    big = np.stack([_rand(74, 53, s, 0.6) for s in (21, 22, 23)])
    view = torch.from_numpy(big).to(DEV)[:, ::2]
    assert not view.is_contiguous() and view.shape == (3, 37, 53)
    got = ht.rle_encode_masks(view)
    assert got == [ot.rle_encode(big[k, ::2]) for k in range(3)]
    assert ht.rle_encode_masks(torch.zeros((0, 37, 53), device=DEV, dtype=torch.uint8)) == []
    b = torch.from_numpy(big).to(DEV) != 0                                             # bool masks
    assert ht.rle_encode_masks(b) == [ot.rle_encode(big[k]) for k in range(3)]


def test_raw_encode_truncates_at_the_caps_and_reports_the_true_sizes():
    from llmseg_amd import _lib, targets as ht
    m, ref = _ref("97x130")
    K, H, W = m.shape
    lib = _lib.load()
    d = torch.from_numpy(m).to(DEV)
    cap_c, cap_h, pad = 16, 12, 8
    counts = torch.full((K, cap_c + pad), 0x5a5a5a5a, device=DEV, dtype=torch.int32)      # rows of cap + pad: the pad must stay as it is
    chars = torch.full((K, cap_h + pad), 0xa5, device=DEV, dtype=torch.uint8)
    # the entry point sees rows of stride cap only when they are dense: encode one mask per call into its padded row
    n_counts = torch.zeros((K,), device=DEV, dtype=torch.int32)
    n_chars = torch.zeros((K,), device=DEV, dtype=torch.int32)
    nb = int(lib.llmseg_rle_encode_ws_bytes(1, H, W))
    ws = torch.empty((nb,), device=DEV, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    for k in range(K):
        rc = lib.llmseg_rle_encode(p(d[k]), 1, H, W, p(counts[k]), p(n_counts[k:]), cap_c, p(chars[k]), p(n_chars[k:]), cap_h, p(ws), nb, ht._stream())
        assert rc == 0, lib.llmseg_last_error()
    torch.cuda.synchronize()
    for k in range(K):
        want = ht.rle_counts(ref[k])
        assert int(n_counts[k]) == 6416 == len(want) and int(n_chars[k]) == len(ref[k]["counts"])
        assert counts[k, :cap_c].cpu().numpy().view(np.uint32).tolist() == want[:cap_c].tolist()
        assert (counts[k, cap_c:] == 0x5a5a5a5a).all() and (chars[k, cap_h:] == 0xa5).all()
        # the characters of the stored counts (16 counts take at least 16 characters), cut at cap_chars
        assert bytes(chars[k, :cap_h].cpu().numpy().tobytes()) == ref[k]["counts"].encode()[:cap_h]
    # bad arguments and a short workspace are refused before any launch
    assert lib.llmseg_rle_encode(p(d), 1, H, W, p(counts), p(n_counts), cap_c, p(chars), p(n_chars), cap_h, p(ws), nb - 1, ht._stream()) == -1
    assert b"workspace" in lib.llmseg_last_error()
    assert lib.llmseg_rle_encode(p(d), 1, H, W, p(counts), p(n_counts), 0, p(chars), p(n_chars), cap_h, p(ws), nb, ht._stream()) == -1
    assert lib.llmseg_rle_encode(None, 1, H, W, p(counts), p(n_counts), cap_c, p(chars), p(n_chars), cap_h, p(ws), nb, ht._stream()) == -1
    assert lib.llmseg_rle_parse(None, None, 1, None, None, None, 0, ht._stream()) == -1


@pytest.mark.parametrize("name", CASES)
def test_parse_equals_the_host_parse_and_feeds_decode(name):
    from llmseg_amd import targets as ht
    from oracle import targets as ot
    m, ref = _ref(name)
    ends, offs = _host_parse(ref)
    for as_bytes in (False, True):
        strings = [r["counts"].encode("ascii") if as_bytes else r["counts"] for r in ref]
        d_ends, d_offs = ht._parse_rles_device(strings, DEV)
        assert torch.equal(d_offs.cpu(), torch.from_numpy(offs))
        assert torch.equal(d_ends[:len(ends)].cpu(), torch.from_numpy(ends.view(np.int32)))
        recs = [{"size": r["size"], "counts": s} for r, s in zip(ref, strings)]
        for hwk in (False, True):
            a = ht.decode_rles(recs, DEV, hwk=hwk)
            b = ht.decode_rles(recs, DEV, hwk=hwk, host_parse=True)
            assert torch.equal(a, b)
            want = np.stack([ot.rle_decode(r) for r in ref], -1 if hwk else 0)
            assert torch.equal(a.cpu(), torch.from_numpy(want))


def test_parse_of_strings_of_very_different_length_in_one_batch():
    """A 5-character string next to 6416 counts (and an 18-character one after it): a carry across chunks and masks that end inside a chunk."""
    from llmseg_amd import targets as ht
    big, small = _ref("97x130")[1], _ref("1024x1024")[1]
    recs = [small[0], big[0], small[2], big[1], small[1]]
    ends, offs = _host_parse(recs)
    d_ends, d_offs = ht._parse_rles_device([r["counts"] for r in recs], DEV)
    assert torch.equal(d_offs.cpu(), torch.from_numpy(offs))
    assert torch.equal(d_ends[:len(ends)].cpu(), torch.from_numpy(ends.view(np.int32)))


def _blobs(k, h, w, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((k, h, w), np.uint8)
    for i in range(k):
        y0, x0 = rng.integers(0, h - 8), rng.integers(0, w - 8)
        m[i, y0:y0 + rng.integers(4, h - y0), x0:x0 + rng.integers(4, w - x0)] = 1
        m[i] &= (rng.random((h, w)) > 0.02).astype(np.uint8)
    return m


def test_round_trip_and_records_equal_the_host_route():
    from llmseg_amd import amg, targets as ht
    h, w, k = 240, 320, 70
    masks = torch.from_numpy(_blobs(k, h, w, 4)).to(DEV)
    enc = ht.rle_encode_masks(masks)
    assert enc == ht.rle_encode_masks(masks.cpu())
    assert torch.equal(ht.decode_rles(enc, DEV), (masks != 0).to(torch.uint8))
    g = torch.Generator().manual_seed(1)
    out = dict(masks=masks, boxes=torch.randint(0, 200, (k, 4), generator=g).to(DEV), iou_preds=torch.rand(k, generator=g).to(DEV),
               stability_score=torch.rand(k, generator=g).to(DEV), points=torch.rand((k, 2), generator=g, dtype=torch.float64),
               areas=masks.flatten(1).sum(1), crop_boxes=torch.tensor([3, 5, 300, 200]).repeat(k, 1))
    dev_recs = amg.to_records(out, (h, w))
    host_recs = amg.to_records({n: v.cpu() for n, v in out.items()}, (h, w))
    assert dev_recs == host_recs and len(dev_recs) == k
    assert all(type(r["area"]) is int and type(r["predicted_iou"]) is float and type(r["segmentation"]["counts"]) is str for r in dev_recs)
    del out["crop_boxes"]
    assert amg.to_records(out, (h, w)) == amg.to_records({n: v.cpu() for n, v in out.items()}, (h, w))
