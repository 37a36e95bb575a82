#!/usr/bin/env python
"""The objects of label maps (vd_label_objects): what the device call costs against the
reference's route, which copies the maps to the host and loops over np.unique there.

Shapes: 16 maps of 480 x 854 and 64 maps of 800 x 1333, each with about 5 and about 100
elliptic objects (seeded; later objects cover earlier ones, so fewer may be visible).

  (a)  ops.label_objects into given buffers (no host read), entry form (expand 0.05),
       obj_cap 255, rle_cap 4 W + 2: with the RLE pass and without it (want_rle=False: the
       init, statistics and finish launches alone).  Timed over `--reps` alternating windows
       of `--calls` calls between two HIP events after a warm-up, as replayed hipGraphs
       (device time: the headline) and eagerly.
  (b)  the reference's route: the maps copied to the host (timed by itself, wall clock around
       a synchronised copy), then tests/label_objects_ref.objects per frame: np.unique, a
       mask, min / max, the float64 box and a column-major RLE per value.  One thread, wall
       clock, on the first --host-frames frames, scaled to F.  Its results are compared
       with (a)'s.

The statistics pass reads every map byte once: F H W bytes over the time of (a) without
RLE, given as a share of the device copy bandwidth measured in the same run
(bench.measure_hbm_copy: read + write bytes of a torch copy_) and of the 8 TB/s peak.

One JSON line per shape and object count, appended to --out when given.

  python tools/bench_label_objects.py [--calls 5] [--reps 9] [--host-frames 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_oks_nms import captured, windows  # noqa: E402
from vosdetectron_amd import ops  # noqa: E402

HBM_PEAK = 8e12
OBJ_CAP = 255


def make_maps(F, h, w, n, seed):
    """F maps with n ellipses each, values 1..n, painted inside their own windows."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((F, h, w), np.uint8)
    k = 0.5 / np.sqrt(n)  # mean semi-axis as a share of the frame side
    for f in range(F):
        for i in range(n):
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            sx, sy = rng.uniform(0.4, 1.6, 2) * k * np.array([w, h]) + 1
            x0, x1 = max(int(cx - sx), 0), min(int(cx + sx) + 1, w)
            y0, y1 = max(int(cy - sy), 0), min(int(cy + sy) + 1, h)
            if x1 <= x0 or y1 <= y0:
                continue
            yy, xx = np.mgrid[y0:y1, x0:x1]
            inside = ((xx - cx) / sx) ** 2 + ((yy - cy) / sy) ** 2 <= 1.0
            lab[f, y0:y1, x0:x1][inside] = i + 1
    return lab


def outputs(F, w, dev, rle):
    out = {"ids": torch.empty((F, OBJ_CAP), dtype=torch.uint8, device=dev),
           "rects": torch.empty((F, OBJ_CAP, 4), dtype=torch.int32, device=dev),
           "areas": torch.empty((F, OBJ_CAP), dtype=torch.int32, device=dev),
           "boxes": torch.empty((F, OBJ_CAP, 4), dtype=torch.float32, device=dev),
           "counts": torch.empty((F,), dtype=torch.int32, device=dev)}
    if rle:
        out["rle_counts"] = torch.empty((F, OBJ_CAP, 4 * w + 2), dtype=torch.int32, device=dev)
        out["rle_n"] = torch.empty((F, OBJ_CAP), dtype=torch.int32, device=dev)
    return out


def host_route(lab_dev, frames):
    """(d2h_us of all maps, numpy_us of `frames` frames, their objects)."""
    from tests import label_objects_ref as R
    torch.set_num_threads(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = lab_dev.cpu().numpy()
    t1 = time.perf_counter()
    objs = [R.objects(host[f], 0.05) for f in range(frames)]
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, objs


def equal_to_host(res, objs):
    counts = res["counts"].cpu().numpy()
    for f, o in enumerate(objs):
        k = len(o["ids"])
        if counts[f] != k:
            return False
        for name in ("ids", "rects", "areas"):
            if not np.array_equal(res[name][f, :k].cpu().numpy(), o[name]):
                return False
        if not np.array_equal(res["boxes"][f, :k].cpu().numpy().view(np.int32),
                              o["boxes"].view(np.int32)):
            return False
        n = res["rle_n"][f, :k].cpu().numpy()
        for i in range(k):
            if n[i] != len(o["rle"][i]) or not np.array_equal(
                    res["rle_counts"][f, i, :n[i]].cpu().numpy().view(np.uint32), o["rle"][i]):
                return False
    return True


def shape_line(F, h, w, n, a, dev, copy_bw):
    lab = torch.from_numpy(make_maps(F, h, w, n, 11 * F + n)).to(dev)
    out_rle, out_no = outputs(F, w, dev, True), outputs(F, w, dev, False)

    def with_rle():
        return ops.label_objects(lab, rle_cap=4 * w + 2, out=out_rle)

    def without():
        return ops.label_objects(lab, want_rle=False, out=out_no)

    for _ in range(2):
        res, _ = with_rle(), without()
    torch.cuda.synchronize()
    runs = {"rle_eager": lambda: [with_rle() for _ in range(a.calls)],
            "stats_eager": lambda: [without() for _ in range(a.calls)]}
    runs["rle_graph"] = captured(runs["rle_eager"])
    runs["stats_graph"] = captured(runs["stats_eager"])
    tm = windows(runs, a.reps, a.calls)
    hf = min(a.host_frames, F)
    d2h_us, numpy_us, objs = host_route(lab, hf)
    numpy_us *= F / hf
    counts = res["counts"].cpu().numpy()
    live = torch.arange(OBJ_CAP, device=dev)[None, :] < res["counts"][:, None]
    over = int((torch.where(live, res["rle_n"], 1) < 0).sum())
    a_us, s_us = tm["rle_graph"]["median_us"], tm["stats_graph"]["median_us"]
    nbytes = F * h * w
    rate = nbytes / (s_us * 1e-6)
    back = sum(int(c) for c in counts) * (1 + 16 + 4 + 16 + 4) + 4 * F + \
        4 * int(torch.where(live, res["rle_n"], 0).clamp(min=0).sum())
    return {"what": "vd_label_objects", "frames": F, "frame_hw": [h, w], "objects_painted": n,
            "objects_per_frame_mean": round(float(counts.mean()), 1),
            "nonzero_share": round(float((lab != 0).float().mean()), 3),
            "obj_cap": OBJ_CAP, "rle_cap": 4 * w + 2, "objects_over_rle_cap": over,
            "calls_per_window": a.calls, "windows": a.reps,
            "a_with_rle_graph": tm["rle_graph"], "a_with_rle_eager": tm["rle_eager"],
            "a_without_rle_graph": tm["stats_graph"], "a_without_rle_eager": tm["stats_eager"],
            "map_bytes": nbytes, "stats_read_GBs": round(rate / 1e9, 1),
            "stats_read_share_of_measured_copy": round(rate / (copy_bw * 1e9), 4),
            "stats_read_share_of_hbm_peak": round(rate / HBM_PEAK, 4),
            "measured_copy_GBs": copy_bw,
            "b_host_route": {"d2h_maps_us": round(d2h_us, 1), "frames_timed": hf,
                             "numpy_loop_us_scaled": round(numpy_us, 1),
                             "total_us": round(d2h_us + numpy_us, 1),
                             "equal_a": bool(equal_to_host(res, objs))},
            "result_bytes_to_host": back,
            "b_over_a_with_rle": round((d2h_us + numpy_us) / a_us, 1),
            "d2h_alone_over_a_with_rle": round(d2h_us / a_us, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--shapes", default="16x480x854,64x800x1333")
    ap.add_argument("--objects", default="5,100")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_objects needs a GPU")
    import bench
    dev = torch.device("cuda")
    copy_bw = bench.measure_hbm_copy(dev)["GBs"]
    for spec in a.shapes.split(","):
        F, h, w = (int(v) for v in spec.split("x"))
        for n in (int(v) for v in a.objects.split(",")):
            s = json.dumps(shape_line(F, h, w, n, a, dev, copy_bw))
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(s + "\n")


if __name__ == "__main__":
    main()
