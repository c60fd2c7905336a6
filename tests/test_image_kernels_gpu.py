"""GPU: the raw-pixel kernels of csrc/image.hip held to the tables of tests/image_kernel_checks.py through the C ABI.  Tap tables integer for integer out of the
caller's workspace; the resampler case table in both filters, byte for byte; `llmseg_clip_preprocess` bf16 bit for bit with its two tables; `llmseg_mask_union`
exactly.  Every output and every workspace sits inside a guard that must be unchanged, every workspace is exactly as long as its formula says and is filled with
0xFF (then 0) first, every refusal is made before a launch.  tests/test_image_kernels_cpu.py proves what these cases would notice."""
import collections
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import image_frontend_checks as fc
from tests import image_kernel_checks as kc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_BYTE = 0x5A
_COUNT = collections.Counter()
RESAMPLE_CASES = kc.resample_cases()


@pytest.fixture(scope="module", autouse=True)
def _module():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    t0 = time.time()
    yield
    print(f"\nimage kernels: wall time of this file {time.time() - t0:.1f} s")
    for k in sorted(_COUNT):
        print(f"  {k}: {_COUNT[k]}")


def _fault_guard(name, e):
    if "HIP error" in str(e) or "illegal memory access" in str(e):          # a device fault: nothing more may be started on this GPU
        pytest.exit(f"{name}: {e}", returncode=3)


@contextlib.contextmanager
def _guarded(name):
    try:
        yield
    except RuntimeError as e:
        _fault_guard(name, e)
        raise


class Buf:
    """`nbytes` device bytes the call may write, GUARD (+ lead) bytes of GUARD_BYTE in front and GUARD behind; the body is pre-filled with `fill`"""

    def __init__(self, nbytes, fill, lead=0):
        self.n, self.start = nbytes, kc.GUARD + lead
        self.buf = torch.full((self.start + nbytes + kc.GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.body.fill_(fill)

    @property
    def body(self):
        return self.buf[self.start:self.start + self.n]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    def intact(self):
        return bool((self.buf[:self.start] == GUARD_BYTE).all()) and bool((self.buf[self.start + self.n:] == GUARD_BYTE).all())

    def numpy(self):
        return self.body.cpu().numpy()


def _lib_ops():
    from llmseg_amd import _lib, ops
    return _lib.load(), _lib, ops


def _resize(entry, filt, d_in, off, stride, h, w, oh, ow, ch, ws_fill, ws_short=0):
    """one call of the C ABI on a window of the device buffer d_in -> (rc, launches, out Buf, ws Buf)"""
    lib, _, ops = _lib_ops()
    nb = lib.llmseg_image_resize_filter_workspace(h, w, oh, ow, ch, filt)
    assert nb == kc.resize_workspace(filt, h, w, oh, ow, ch)
    if filt == kc.BILINEAR:
        assert nb == lib.llmseg_image_resize_workspace(h, w, oh, ow, ch)
    out, ws = Buf(oh * ow * ch, 0x33), Buf(nb - ws_short, ws_fill)
    n0 = lib.llmseg_launch_count()
    if entry == "plain":
        rc = lib.llmseg_image_resize_u8(d_in.data_ptr() + off, stride, out.ptr, h, w, oh, ow, ch, ws.ptr, ws.n, ops._stream())
    else:
        rc = lib.llmseg_image_resize_u8_filter(d_in.data_ptr() + off, stride, out.ptr, h, w, oh, ow, ch, filt, ws.ptr, ws.n, ops._stream())
    launches = lib.llmseg_launch_count() - n0
    torch.cuda.synchronize()
    return rc, launches, out, ws


# ------------------------------------------------------------------------------------------------------------------------ A. tap tables
def _table_sweep(filt, pairs, vertical):
    """one-row (one-column) images: only the horizontal (vertical) pass runs; the table out of the workspace and the bytes in the same call"""
    bad_entries = bad_bytes = rows = taps = 0
    other = kc.align256((kc.ksize(filt, 1, 1) + 2) * 4)                        # the table of the axis of size 1: one row, never written
    for n, (i, o) in enumerate(pairs):
        a = np.random.default_rng(7000 + n).integers(0, 256, (i, 1, 3) if vertical else (1, i, 3), dtype=np.uint8)
        d_in = torch.from_numpy(a.reshape(-1)).to(DEV)
        h, w, oh, ow = (i, 1, o, 1) if vertical else (1, i, 1, o)
        with _guarded(f"{kc.FNAME[filt]} {i} -> {o}"):
            rc, launches, out, ws = _resize("filter" if n % 2 or filt == kc.BICUBIC else "plain", filt, d_in, 0, w * 3, h, w, oh, ow, 3, 0xFF)
        assert rc == 0 and out.intact() and ws.intact(), (i, o)
        got, wsb = out.numpy(), ws.numpy()
        bad_bytes += int((got != kc.ref_resize(filt, a, oh, ow).reshape(-1)).sum())
        ks = kc.ksize(filt, i, o)
        tab_bytes = o * (ks + 2) * 4
        lo = other if vertical else 0
        if i == o:                                                             # the copy route: no launch, no table
            assert launches == 0 and bool((wsb == 0xFF).all()), (i, o)
            continue
        assert launches == 2, (i, o)
        d = kc.table_diff(kc.decode_table(wsb, lo, o, ks), kc.ref_coeffs(filt, i, o))
        assert d == 0, f"{kc.FNAME[filt]} {'vertical' if vertical else 'horizontal'} table of {i} -> {o}: {d} entries differ"
        bad_entries += d
        rows += o
        taps += o * ks
        # nothing of the workspace but the table is written: the other axis' table and the intermediate are not used by a one-pass call
        assert bool((wsb[:lo] == 0xFF).all()) and bool((wsb[lo + tab_bytes:] == 0xFF).all()), (i, o)
    which = f"{kc.FNAME[filt]} {'vertical' if vertical else 'horizontal'}"
    _COUNT[f"{which} tables: pairs"] += len(pairs)
    _COUNT[f"{which} tables: rows compared"] += rows
    _COUNT[f"{which} tables: tap slots compared (zero fill included)"] += taps
    assert bad_entries == 0 and bad_bytes == 0, (bad_entries, bad_bytes)


@pytest.mark.parametrize("filt", kc.FILTERS, ids=[kc.FNAME[f] for f in kc.FILTERS])
def test_horizontal_tap_tables_integer_for_integer(filt):
    _table_sweep(filt, kc.sweep_pairs(filt), vertical=False)


@pytest.mark.parametrize("filt", kc.FILTERS, ids=[kc.FNAME[f] for f in kc.FILTERS])
def test_vertical_tap_tables_integer_for_integer(filt):
    _table_sweep(filt, kc.vertical_pairs(filt), vertical=True)


# ------------------------------------------------------------------------------------------------------------------- B. the resampler case table
@pytest.mark.parametrize("case", RESAMPLE_CASES, ids=[c.name for c in RESAMPLE_CASES])
def test_resampler_case(case):
    c = case
    buf, off, stride, img = kc.make_input(c)
    d_in = torch.from_numpy(buf).to(DEV)
    args = (c.filt, d_in, off, stride, c.h, c.w, c.oh, c.ow, c.ch)
    if kc.case_refused(c):                                                     # more table columns than the kernel takes: refused before a launch
        with _guarded(c.name):
            rc, launches, out, ws = _resize("filter", *args, 0xFF)
        assert rc == -1 and launches == 0 and out.intact() and ws.intact()
        assert bool((out.body == 0x33).all()) and bool((ws.body == 0xFF).all())
        _COUNT["resampler: cases refused for their tap count"] += 1
        return
    ref = kc.ref_resize(c.filt, img, c.oh, c.ow).reshape(-1)
    with _guarded(c.name):
        rc1, l1, out1, ws1 = _resize("plain" if c.filt == kc.BILINEAR else "filter", *args, 0xFF)
        rc2, l2, out2, ws2 = _resize("filter", *args, 0x00)
    assert rc1 == 0 and rc2 == 0
    assert l1 == l2 == 2 * ((c.ow != c.w) + (c.oh != c.h))
    assert out1.intact() and ws1.intact() and out2.intact() and ws2.intact(), f"{c.name}: a store outside the output or the workspace"
    got1, got2 = out1.numpy(), out2.numpy()
    d1, d2 = int((got1 != ref).sum()), int((got2 != ref).sum())
    assert d1 == 0 and d2 == 0, f"{c.name}: {d1} / {d2} of {ref.size} bytes differ (0xFF / zero workspace)"
    assert np.array_equal(d_in.cpu().numpy(), buf), f"{c.name}: the input buffer was written"
    _COUNT[f"resampler: {kc.FNAME[c.filt]} cases compared byte for byte"] += 1
    _COUNT[f"resampler: {kc.FNAME[c.filt]} bytes compared"] += ref.size


@pytest.mark.parametrize("filt", kc.FILTERS, ids=[kc.FNAME[f] for f in kc.FILTERS])
def test_resampler_refusals_are_made_before_a_launch(filt):
    calls = []                                                                 # (name, entry, filter, h, w, oh, ow, ch, stride, bytes the workspace is short)
    for (i, o) in kc.BOUNDARY_REFUSED[filt]:
        calls.append((f"{i} -> {o} columns", "filter", filt, 2, i, 2, o, 3, i * 3, 0))
        calls.append((f"{i} -> {o} rows", "filter", filt, i, 2, o, 2, 3, 6, 0))
    calls.append(("five channels", "filter", filt, 4, 6, 5, 7, 5, 30, 0))
    calls.append(("row stride below a row", "filter", filt, 4, 6, 5, 7, 3, 17, 0))
    calls.append(("workspace one byte short", "filter", filt, 4, 6, 5, 7, 3, 18, 1))
    calls.append(("workspace one byte short, copy route", "filter", filt, 4, 6, 4, 6, 3, 18, 1))
    if filt == kc.BILINEAR:
        calls += [(n + " (llmseg_image_resize_u8)", "plain") + tuple(r) for n, _, *r in calls]
    lib, _, ops = _lib_ops()
    d_in = torch.full((1 << 16,), kc.SENTINEL, dtype=torch.uint8, device=DEV)
    for name, entry, f, h, w, oh, ow, ch, stride, short in calls:
        assert h * max(stride, w * ch) <= d_in.numel()
        with _guarded(name):
            rc, launches, out, ws = _resize(entry, f, d_in, 0, stride, h, w, oh, ow, ch, 0xFF, ws_short=short)
        assert rc == -1 and launches == 0, name
        assert out.intact() and ws.intact() and bool((out.body == 0x33).all()) and bool((ws.body == 0xFF).all()), name
        _COUNT["resampler: refused calls"] += 1
    if filt == kc.BICUBIC:                                                     # a filter the library does not know: no workspace size either
        assert lib.llmseg_image_resize_filter_workspace(4, 6, 5, 7, 3, 2) == -1
        out, ws = Buf(5 * 7 * 3, 0x33), Buf(1 << 16, 0xFF)
        n0 = lib.llmseg_launch_count()
        rc = lib.llmseg_image_resize_u8_filter(d_in.data_ptr(), 18, out.ptr, 4, 6, 5, 7, 3, 2, ws.ptr, ws.n, ops._stream())
        torch.cuda.synchronize()
        assert rc == -1 and lib.llmseg_launch_count() == n0 and bool((out.body == 0x33).all()) and bool((ws.body == 0xFF).all())
        _COUNT["resampler: refused calls"] += 1


@pytest.mark.parametrize("resample", ("bilinear", "bicubic"))
def test_crop_box_of_the_python_entry_equals_the_c_abi(resample):
    _, _, ops = _lib_ops()
    filt = kc.BICUBIC if resample == "bicubic" else kc.BILINEAR
    for ch, (x0, y0, x1, y1), (oh, ow) in ((3, (5, 3, 28, 20), (9, 31)), (1, (1, 0, 14, 21), (30, 13)), (4, (3, 2, 12, 8), (6, 9)), (2, (0, 1, 33, 2), (1, 40))):
        img = np.random.default_rng(40 + ch).integers(0, 256, (21, 33, ch), dtype=np.uint8)
        d = torch.from_numpy(img).to(DEV)
        h, w = y1 - y0, x1 - x0
        with _guarded(f"crop_box {resample} c{ch}"):
            got = ops.image_resize_u8(d, oh, ow, crop_box=(x0, y0, x1, y1), resample=resample).cpu().numpy()
            rc, _, out, ws = _resize("filter", filt, d, (y0 * 33 + x0) * ch, 33 * ch, h, w, oh, ow, ch, 0xFF)
        assert rc == 0 and out.intact() and ws.intact()
        ref = kc.ref_resize(filt, np.ascontiguousarray(img[y0:y1, x0:x1]), oh, ow)
        assert np.array_equal(got, ref) and np.array_equal(out.numpy(), ref.reshape(-1)), (resample, ch)
        _COUNT["resampler: crop_box rows"] += 1


# ------------------------------------------------------------------------------------------------------------------------ C. CLIP preprocess
def _clip(d_in, off, stride, h, w, S, mean, std, ws_fill, ws_short=0):
    lib, _, ops = _lib_ops()
    nb = lib.llmseg_clip_preprocess_workspace(h, w, max(S, 1))
    assert nb == kc.clip_workspace(h, w, max(S, 1))
    out, ws = Buf(3 * max(S, 1) * max(S, 1) * 2, 0x33), Buf(nb - ws_short, ws_fill)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    n0 = lib.llmseg_launch_count()
    rc = lib.llmseg_clip_preprocess(d_in.data_ptr() + off, stride, out.ptr, h, w, S, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), ws.ptr, ws.n, ops._stream())
    launches = lib.llmseg_launch_count() - n0
    torch.cuda.synchronize()
    return rc, launches, out, ws


_CLIP_ALL = [(h, w, S, 300 + n) for n, (h, w, S) in enumerate(kc.CLIP_CASES)] + [(kc.U255_SIZE, kc.U255_SIZE, kc.U255_SIZE, None)]
_CLIP_REF = {}


def _clip_case(h, w, S, seed):
    """(img, mean, std, expected bits), computed once for the dense and the strided run"""
    if (h, w, S) not in _CLIP_REF:
        if seed is None:
            img, mean, std = kc.u255_image(), kc.U255_MEAN, kc.U255_STD
        else:
            img, mean, std = kc.clip_image(h, w, seed), fc.CLIP_MEAN, fc.CLIP_STD
        _CLIP_REF[(h, w, S)] = (img, mean, std, kc.clip_ref_bits(img, S, mean, std))
    return _CLIP_REF[(h, w, S)]


@pytest.mark.parametrize("strided", (False, True), ids=("dense", "strided-odd-start"))
@pytest.mark.parametrize("case", _CLIP_ALL, ids=[f"{h}x{w}-{S}" + ("" if seed is not None else "-every-byte") for h, w, S, seed in _CLIP_ALL])
def test_clip_preprocess_bit_for_bit_with_its_tables(case, strided):
    h, w, S, seed = case
    img, mean, std, ref = _clip_case(h, w, S, seed)
    lead, extra = (3, 7) if strided else (0, 0)                                # a window of a larger sentinel image that starts at an odd byte
    stride = w * 3 + extra
    buf = np.full(((h + 3) * stride + lead + 16,), kc.SENTINEL, np.uint8)
    off = 2 * stride + lead
    assert off % 2 == (1 if strided else 0)
    for y in range(h):
        buf[off + y * stride: off + y * stride + w * 3] = img[y].reshape(-1)
    d_in = torch.from_numpy(buf).to(DEV)
    name = f"clip {h}x{w} -> {S}"
    with _guarded(name):
        rc1, l1, out1, ws1 = _clip(d_in, off, stride, h, w, S, mean, std, 0xFF)
        rc2, l2, out2, ws2 = _clip(d_in, off, stride, h, w, S, mean, std, 0x00)
    nh, nw, top, left = kc.clip_geometry(h, w, S)
    do_h, do_v = nw != w, nh != h
    assert rc1 == 0 and rc2 == 0 and l1 == l2 == 2 * do_h + 1 + do_v
    assert out1.intact() and ws1.intact() and out2.intact() and ws2.intact(), f"{name}: a store outside the output or the workspace"
    got1, got2 = (o.numpy().view(np.int16).reshape(3, S, S) for o in (out1, out2))
    d1, d2 = int((got1 != ref).sum()), int((got2 != ref).sum())
    assert d1 == 0 and d2 == 0, f"{name}: {d1} / {d2} of {ref.size} bf16 elements differ (0xFF / zero workspace)"
    assert np.array_equal(d_in.cpu().numpy(), buf)
    wsb = ws1.numpy()
    kw, kh = kc.ksize(kc.BICUBIC, w, nw), kc.ksize(kc.BICUBIC, h, nh)
    voff = kc.align256(S * (kw + 2) * 4)
    if do_h:                                                                   # S rows: the columns left .. left + S of the w -> nw resampling
        exp = tuple(t[left:left + S] for t in fc.coeffs(w, nw))
        d = kc.table_diff(kc.decode_table(wsb, 0, S, kw), exp)
        assert d == 0, f"{name}: {d} entries of the horizontal table differ"
        _COUNT["clip: table rows compared"] += S
    else:
        assert bool((wsb[:voff] == 0xFF).all())
    if do_v:                                                                   # S rows top .. top + S; first indices relative to the first input row the call reads
        xmin, cnt, kk = (t[top:top + S] for t in fc.coeffs(h, nh))
        g0, gc, gk = kc.decode_table(wsb, voff, S, kh)
        r0 = int(xmin[0]) - int(g0[0])
        assert 0 <= r0 <= int(xmin.min()), (r0, int(xmin.min()))
        d = kc.table_diff((g0 + r0, gc, gk), (xmin, cnt, kk))
        assert d == 0, f"{name}: {d} entries of the vertical table differ"
        _COUNT["clip: table rows compared"] += S
    else:
        assert bool((wsb[voff:voff + kc.align256(S * (kh + 2) * 4)] == 0xFF).all())
    _COUNT["clip: cases compared bit for bit"] += 1
    _COUNT["clip: bf16 elements compared"] += ref.size


def test_clip_preprocess_refusals_are_made_before_a_launch():
    d_in = torch.full((1 << 14,), kc.SENTINEL, dtype=torch.uint8, device=DEV)
    for name, h, w, S, stride, short in (("row stride below a row", 20, 30, 7, 89, 0), ("workspace one byte short", 20, 30, 7, 90, 1), ("size 0", 20, 30, 0, 90, 0)):
        with _guarded(name):
            rc, launches, out, ws = _clip(d_in, 0, stride, h, w, S, fc.CLIP_MEAN, fc.CLIP_STD, 0xFF, ws_short=short)
        assert rc == -1 and launches == 0, name
        assert out.intact() and ws.intact() and bool((out.body == 0x33).all()) and bool((ws.body == 0xFF).all()), name
        _COUNT["clip: refused calls"] += 1
    lib = _lib_ops()[0]
    assert lib.llmseg_clip_preprocess_workspace(20, 30, 0) == -1 and lib.llmseg_clip_preprocess_workspace(0, 30, 7) == -1


# ----------------------------------------------------------------------------------------------------------------------------- D. mask union
@pytest.mark.parametrize("K", kc.UNION_K)
@pytest.mark.parametrize("n", list(kc.UNION_N))
def test_mask_union_exact(n, K):
    lib, _lib, ops = _lib_ops()
    H, W = kc.UNION_N[n]
    masks, sel, sel_all = kc.union_case(n, K)
    for s, m in ((sel, kc.with_sentinel(masks, sel)), (sel_all, masks)):
        ref = kc.union_m(m, s).reshape(-1)
        dm, ds = torch.from_numpy(m).to(DEV), torch.from_numpy(s).to(DEV)
        Cn = s.shape[0]
        for lead in (0, 5):                                                    # a 16-byte aligned output, and one at an odd address
            out = Buf(Cn * n, 0x33, lead=lead)
            assert out.ptr % 16 == (0 if lead == 0 else 5)
            with _guarded(f"mask_union n={n} K={K}"):
                n0 = lib.llmseg_launch_count()
                rc = lib.llmseg_mask_union(dm.data_ptr(), ds.data_ptr(), out.ptr, K, Cn, H, W, ops._stream())
                launches = lib.llmseg_launch_count() - n0
                torch.cuda.synchronize()
            assert rc == 0 and launches == 1 and out.intact(), f"n={n} K={K} C={Cn} lead={lead}"
            d = int((out.numpy() != ref).sum())
            assert d == 0, f"mask_union n={n} K={K} C={Cn} lead={lead}: {d} pixels differ"
            _COUNT["mask_union: calls compared exactly"] += 1
            _COUNT["mask_union: pixels compared"] += ref.size
        with _guarded(f"ops.mask_union n={n} K={K}"):
            got = ops.mask_union(dm, ds).cpu().numpy()
        assert np.array_equal(got.reshape(-1), ref)
        assert np.array_equal(dm.cpu().numpy(), m) and np.array_equal(ds.cpu().numpy(), s)
