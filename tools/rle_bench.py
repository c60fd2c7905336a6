"""COCO RLE codec timing on one MI355X: the device routes (`llmseg_rle_encode`, `llmseg_rle_parse`) against the host routes they replace, on
the same box in the same run.  K = 64 and K = 100 synthetic blob masks (ellipses with a ragged edge, a few hundred to ~2000 runs each, like
everything-mode proposals) at 1024 x 1024 and 683 x 1024, masks on the device.
  (a) encode, host route:   rle_encode_masks(masks.cpu())   -- the copy included, as `amg.to_records` ran it before the device codec
  (b) encode, device route: rle_encode_masks(masks)
  (c) decode, host parse:   decode_rles(recs, "cuda", host_parse=True)
  (d) decode, device parse: decode_rles(recs, "cuda")
Wall clock around the whole call (synchronised before and after; median of `reps`), HIP events around the device part of (b) and (d):
`_rle_encode_device` (the library call and the copy of the K sizes it reports) and `_parse_rles_device` + `llmseg_rle_decode` (the upload of the
joined strings and the library calls).  Prints one markdown table.
usage: python tools/rle_bench.py [reps=10]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from llmseg_amd import targets as ht  # noqa: E402

DEV = "cuda"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def blobs(k, h, w, seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.zeros((k, h, w), np.uint8)
    for i in range(k):
        cy, cx = rng.uniform(0.1, 0.9) * h, rng.uniform(0.1, 0.9) * w
        ry, rx = rng.uniform(0.03, 0.3) * h, rng.uniform(0.03, 0.3) * w
        r = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2
        m[i] = r < 1.0 + 0.15 * np.sin(xs * 0.21 + i) * np.cos(ys * 0.17)
    return m


def wall(fn):
    ts = []
    for _ in range(reps + 1):                      # the first run is the warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return f"{statistics.median(ts[1:]) * 1e3:.2f} [{min(ts[1:]) * 1e3:.2f} - {max(ts[1:]) * 1e3:.2f}]", out


def events(fn):
    ts = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); a.record()
        fn()
        b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts[1:])


print(f"device: {torch.cuda.get_device_name(0)}; median [min - max] of {reps} after one warm-up; ms")
print("| masks | runs / mask | (a) encode host + copy | (b) encode device | (b) device part | (c) decode host parse | (d) decode device parse | (d) device part |")
print("|---|---:|---:|---:|---:|---:|---:|---:|")
for h, w in ((1024, 1024), (683, 1024)):
    for k in (64, 100):
        masks = torch.from_numpy(blobs(k, h, w, k + h)).to(DEV)
        t_a, recs_host = wall(lambda: ht.rle_encode_masks(masks.cpu()))
        t_b, recs = wall(lambda: ht.rle_encode_masks(masks))
        assert recs == recs_host
        t_bd = events(lambda: ht._rle_encode_device(masks))
        t_c, dense_host = wall(lambda: ht.decode_rles(recs, DEV, host_parse=True))
        t_d, dense = wall(lambda: ht.decode_rles(recs, DEV))
        assert torch.equal(dense, dense_host) and torch.equal(dense, masks)
        strings = [r["counts"] for r in recs]

        def device_part():
            ends, offs = ht._parse_rles_device(strings, DEV)
            out = torch.empty((k, h, w), device=DEV, dtype=torch.uint8)
            ht._lib.check(ht._lib.load().llmseg_rle_decode(ht._p(ends), ht._p(offs), ht._p(out), k, h, w, 0, ht._stream()), "rle_decode")
        t_dd = events(device_part)
        runs = sum(len(ht.rle_counts(r)) for r in recs) / k
        print(f"| {k} x {h} x {w} | {runs:.0f} | {t_a} | {t_b} | {t_bd:.2f} | {t_c} | {t_d} | {t_dd:.2f} |", flush=True)
