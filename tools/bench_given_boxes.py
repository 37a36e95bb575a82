#!/usr/bin/env python
"""Detection from given boxes: what vd_rois_from_boxes, and it plus vd_gather_rows, cost
against the host route the reference takes for the same step.

Shapes: F = 16 and F = 64 frames with 1000 boxes per frame (cap 1000), a third of them
duplicates, frames of 800 x 1333 at im_scale 1, DEDUP_BOXES 1/16, K = 81 classes.

  (a)  ops.rois_from_boxes: one launch for all frames.
  (b)  (a) + ops.gather_rows on [F,cap,81] scores and [F,cap,324] deltas.
  (c)  the host route (lib/core/test.py:130-139): the boxes copied to the host, per frame
       _get_rois_blob, the hash and np.unique in numpy, then rois, index and inv_index
       copied back to the device.  One thread, wall clock, median of --host-reps runs; its
       maps are compared with (a)'s.

(a) and (b) are timed over `--reps` alternating windows of `--calls` calls between two HIP
events after a warm-up, as replayed hipGraphs (device time: the headline) and eagerly.

One JSON line per shape, appended to --out when given.

  python tools/bench_given_boxes.py [--calls 20] [--reps 9] [--host-reps 9] [--out FILE]
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
from bench_oks_nms import captured, stats, windows  # noqa: E402
from vosdetectron_amd import ops  # noqa: E402

N, K, DEDUP, HW = 1000, 81, 0.0625, (800, 1333)


def make_boxes(F, seed):
    from tests.given_boxes_ref import _random_boxes
    rng = np.random.default_rng(seed)
    return np.stack([_random_boxes(rng, N, HW, 1. / 3) for _ in range(F)])


def host_route(boxes_d, counts_d, dev):
    """(c) once: (d2h_us, numpy_us, h2d_us) and the maps."""
    from tests.given_boxes_ref import dedup, rois_blob
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    boxes, counts = boxes_d.cpu().numpy(), counts_d.cpu().numpy()
    t1 = time.perf_counter()
    F, cap = boxes.shape[:2]
    rois = np.zeros((F, cap, 5), np.float32)
    index = np.zeros((F, cap), np.int32)
    inv = np.zeros((F, cap), np.int32)
    ucounts = np.zeros((F,), np.int32)
    for f in range(F):
        n = int(counts[f])
        r, i, v = dedup(rois_blob(boxes[f, :n], 1.0, f), DEDUP)
        ucounts[f] = len(i)
        rois[f, :len(i)], index[f, :len(i)], inv[f, :n] = r, i, v
    t2 = time.perf_counter()
    out = [torch.from_numpy(a).to(dev) for a in (rois, ucounts, index, inv)]
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return ((t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6), out


def shape_line(F, a, dev):
    boxes = torch.from_numpy(make_boxes(F, 11 * F)).to(dev)
    counts = torch.full((F,), N, dtype=torch.int32, device=dev)
    scale = torch.ones((F,), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(F)
    scores = torch.rand((F, N, K), device=dev, generator=g)
    deltas = torch.randn((F, N, 4 * K), device=dev, generator=g)

    def front():
        return ops.rois_from_boxes(boxes, counts, scale, DEDUP)

    def both():
        rois, ucounts, index, inv = front()
        return ops.gather_rows(boxes, scores, deltas, index, inv, counts, ucounts)

    for _ in range(3):
        got = front()
        both()
    torch.cuda.synchronize()
    runs = {"a_eager": lambda: [front() for _ in range(a.calls)],
            "b_eager": lambda: [both() for _ in range(a.calls)]}
    runs["a_graph"] = captured(runs["a_eager"])
    runs["b_graph"] = captured(runs["b_eager"])
    tm = windows(runs, a.reps, a.calls)
    torch.set_num_threads(1)
    parts, ref = [], None
    for _ in range(a.host_reps):
        p, ref = host_route(boxes, counts, dev)
        parts.append(p)
    same = all(bool(torch.equal(x, y)) for x, y in zip(got, ref))
    parts = np.asarray(parts)
    total = stats(list(parts.sum(1)))
    a_us, b_us = tm["a_graph"]["median_us"], tm["b_graph"]["median_us"]
    return {"what": "vd_rois_from_boxes", "frames": F, "boxes_per_frame": N, "cap": N,
            "distinct_per_frame_mean": round(float(got[1].float().mean()), 1),
            "dedup_boxes": DEDUP, "classes": K, "calls_per_window": a.calls, "windows": a.reps,
            "a_rois_from_boxes_graph": tm["a_graph"], "a_rois_from_boxes_eager": tm["a_eager"],
            "b_with_gather_graph": tm["b_graph"], "b_with_gather_eager": tm["b_eager"],
            "c_host_route": {"runs": a.host_reps, "total": total,
                             "d2h_median_us": round(float(np.median(parts[:, 0])), 1),
                             "numpy_median_us": round(float(np.median(parts[:, 1])), 1),
                             "h2d_median_us": round(float(np.median(parts[:, 2])), 1),
                             "equal_a": same},
            "c_over_a_graph": round(total["median_us"] / a_us, 1),
            "c_over_b_graph": round(total["median_us"] / b_us, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=9)
    ap.add_argument("--frames", default="16,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_given_boxes needs a GPU")
    dev = torch.device("cuda")
    for F in (int(v) for v in a.frames.split(",")):
        s = json.dumps(shape_line(F, a, dev))
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
