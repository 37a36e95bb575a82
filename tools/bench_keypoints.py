#!/usr/bin/env python
"""Keypoint R-CNN stage times at the bench's step size (64 frames x 100 detections):

  * vd_heatmaps_to_keypoints alone (one launch over all rows),
  * the keypoint head (Keypoint_Head's convs + Keypoint_Outs) on the same number of
    14 x 14 RoI maps, the convs alone, and the convs on the Winograd F(4x4) route the
    head declines for its accuracy bound,
  * the numpy restatement of the decode (tests/keypoint_ref.py, one thread) on an
    evenly spaced sample of the same rows, scaled to all rows.

The boxes are the detections the e2e_keypoint_rcnn_R-50-FPN_1x pipeline makes on
two seeded 320 x 480 frames (the GPU test's), scaled to 800 x 1333 and repeated to
the row count; the heatmaps are seeded normal logits x 3.  HIP events around each
call after a warm-up; median and 10th..90th percentile, one JSON line.

  python tools/bench_keypoints.py [--rows 6400] [--iters 10] [--cpu-rows 16]
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
from vosdetectron_amd import config as vcfg, modeling, ops  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 3),
            "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 3),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 3)}


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return stats([e0.elapsed_time(e1) for e0, e1 in evs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6400)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-rows", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keypoints needs a GPU")
    import bench
    from tests import keypoint_ref as kref
    from vosdetectron_amd.engine import KeypointFramePipeline
    from vosdetectron_amd.weights import build_model
    dev = torch.device("cuda")
    cfg = vcfg.get("e2e_keypoint_rcnn_R-50-FPN_1x")
    model, _ = build_model(cfg, seed=0, device=dev, channels_last=True)
    pipe = KeypointFramePipeline(model, cfg, frame_hw=(320, 480), batch=2, channels_last=True,
                                 device=dev)
    out = pipe.run(torch.from_numpy(bench.synthetic_frames(2, 21, 320, 480)).to(dev))
    ks = out["counts_host"]
    src = torch.cat([out["dets"][f, :k, :4] for f, k in enumerate(ks)]).cpu().numpy()
    if not len(src):
        raise SystemExit("the seeded frames gave no detections")
    sc = np.asarray([1333 / 480., 800 / 320., 1333 / 480., 800 / 320.], np.float32)
    boxes_np = np.resize(src * sc, (a.rows, 4)).astype(np.float32)
    K, S = cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.HEATMAP_SIZE
    g = torch.Generator(device="cuda").manual_seed(3)
    maps = torch.randn((a.rows, K, S, S), device=dev, generator=g) * 3
    boxes = torch.from_numpy(boxes_np).to(dev)
    w = np.maximum(boxes_np[:, 2] - boxes_np[:, 0], 1)
    h = np.maximum(boxes_np[:, 3] - boxes_np[:, 1], 1)
    px = float(np.sum(np.ceil(w) * np.ceil(h))) * K  # resized-map values the decode visits

    dec = timed(lambda: ops.heatmaps_to_keypoints(maps, boxes, cfg.KRCNN.INFERENCE_MIN_SIZE),
                a.iters)
    P = cfg.KRCNN.ROI_XFORM_RESOLUTION
    feat = torch.randn((a.rows, P, P, 256), device=dev, generator=g)
    kh = model.Keypoint_Head
    modeling.ROUTE_COUNTS.clear()
    with torch.no_grad():
        head = timed(lambda: model.Keypoint_Outs(kh.head_nhwc(feat)), a.iters)
        convs = timed(lambda: kh.head_nhwc(feat), a.iters)
        routes = dict(modeling.ROUTE_COUNTS)
        # the F(4x4) route the head declines for its accuracy bound, for the record
        kh.wino4 = True
        modeling.ROUTE_COUNTS.clear()
        convs4 = timed(lambda: kh.head_nhwc(feat), a.iters)
        routes4 = dict(modeling.ROUTE_COUNTS)
        kh.wino4 = False

    torch.set_num_threads(1)
    idx = np.linspace(0, a.rows - 1, a.cpu_rows).astype(int)
    m_np, b_np = maps[idx].cpu().numpy(), boxes_np[idx]
    t0 = time.perf_counter()
    ref = kref.heatmaps_to_keypoints(m_np, b_np, cfg.KRCNN.INFERENCE_MIN_SIZE)
    cpu_s = time.perf_counter() - t0
    got = ops.heatmaps_to_keypoints(maps[idx], boxes[idx]).cpu().numpy()
    same = bool(np.array_equal(got[:, :3], ref[:, :3]))
    w_s, h_s = w[idx], h[idx]
    px_s = float(np.sum(np.ceil(w_s) * np.ceil(h_s))) * K
    print(json.dumps({
        "rows": a.rows, "keypoints": K, "heatmap": S, "source_detections": int(len(src)),
        "mean_box_wh": [round(float(w.mean()), 1), round(float(h.mean()), 1)],
        "resized_values": px, "decode": dec,
        "decode_gvalues_per_s": round(px / (dec["median_ms"] * 1e-3) / 1e9, 2),
        "head_convs_and_outputs": head, "head_convs_only": convs, "conv_routes": routes,
        "head_convs_only_wino4": convs4, "conv_routes_wino4": routes4,
        "numpy_one_thread": {"rows_timed": int(len(idx)), "seconds": round(cpu_s, 3),
                             "scaled_to_all_rows_s": round(cpu_s * px / px_s, 1),
                             "xy_logit_equal_device": same}}), flush=True)


if __name__ == "__main__":
    main()
