#!/usr/bin/env python
"""Frame -> blob kernels on the same frames: the single-size entries
(vd_image_to_blob / vd_image_resize_to_blob, sizes as launch arguments) against
vd_image_resize_to_blob_ragged (a geometry row per frame read from device
memory).  HIP events around each launch, the two alternated launch by launch
after a warm-up, so both see the same machine state; medians and the
10th..90th percentile spread per case, one JSON line each.  Outputs are
compared bit for bit before anything is timed.

  python tools/bench_ragged_blob.py [--frames 8] [--launches 40] [--nhwc 1]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vosdetectron_amd import ops  # noqa: E402

# (name, H, W, TEST.SCALE, TEST.MAX_SIZE)
CASES = [("800x1333 identity", 800, 1333, 800, 1333),
         ("480x854 x1.561 (800/1333)", 480, 854, 800, 1333),
         ("480x854 x1.667 (800/1500)", 480, 854, 800, 1500)]


def timed(fn, ev):
    ev[0].record()
    fn()
    ev[1].record()


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_us": round(float(np.median(a)) * 1e3, 2),
            "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e3, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e3, 2),
            "min_us": round(float(a[0]) * 1e3, 2), "max_us": round(float(a[-1]) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nhwc", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_blob needs a GPU")
    dev = torch.device("cuda")
    lut = torch.from_numpy(ops.pixel_lut()).to(dev)
    F, nhwc = a.frames, bool(a.nhwc)
    for name, H, W, target, max_size in CASES:
        geo = ops.frame_geometry([(H, W)] * F, target, max_size, 32)
        (Hp, Wp), s = geo.padded[0], geo.scale[0]
        fr = np.random.RandomState(H).randint(0, 256, (F, H, W, 3), np.uint8)
        frames = torch.from_numpy(fr).to(dev)
        packed = frames.view(-1)
        rows = torch.from_numpy(geo.rows().view(np.uint8)).to(dev)
        shape = (F, Hp, Wp, 3) if nhwc else (F, 3, Hp, Wp)
        out_a = torch.empty(shape, dtype=torch.float32, device=dev)
        out_b = torch.empty(shape, dtype=torch.float32, device=dev)
        if s == 1.0:
            def single():
                ops.image_to_blob(frames, lut, Hp, Wp, nhwc=nhwc, out=out_a)
        else:
            def single():
                ops.image_resize_to_blob(frames, lut, s, Hp, Wp, nhwc=nhwc, out=out_a)

        def ragged():
            ops.image_resize_to_blob_ragged(packed, rows, lut, Hp, Wp, nhwc=nhwc, out=out_b)

        single()
        ragged()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b))
        for _ in range(a.warmup):
            single()
            ragged()
        torch.cuda.synchronize()
        evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                for _ in range(a.launches)] for _ in range(2)]
        for i in range(a.launches):  # alternate; swap who goes first every launch
            order = ((0, single), (1, ragged)) if i % 2 == 0 else ((1, ragged), (0, single))
            for k, fn in order:
                timed(fn, evs[k][i])
        torch.cuda.synchronize()
        t = [[e0.elapsed_time(e1) for e0, e1 in evs[k]] for k in range(2)]
        in_b, out_bytes = F * H * W * 3, F * Hp * Wp * 3 * 4
        line = {"case": name, "frames": F, "scale": s, "blob": [Hp, Wp], "nhwc": nhwc,
                "launches": a.launches, "bit_identical": same,
                "bytes_in": in_b, "bytes_out": out_bytes,
                "single_size": stats(t[0]), "ragged": stats(t[1])}
        line["ragged_over_single_median"] = round(
            line["ragged"]["median_us"] / line["single_size"]["median_us"], 4)
        line["ragged_gbps"] = round((in_b + out_bytes) / (line["ragged"]["median_us"] * 1e-6) / 1e9,
                                    1)
        print(json.dumps(line), flush=True)
        if not same:
            raise SystemExit("outputs differ: %s" % name)


if __name__ == "__main__":
    main()
