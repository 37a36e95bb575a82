#!/usr/bin/env python
"""What combining the TEST.KPS_AUG views costs at the bench's step size (64 frames x 100
detections, K = 17, 56 x 56 heatmaps, V = 6 views of which every other one is flipped and
the last four are tagged ds, ds, us, us):

  (a) torch   the torch composition on the device: per flipped view index_select of the
              channels + flip of the last axis, stack, mean / amax over the views, then
              vd_heatmaps_to_keypoints on the result,
  (b) fused   vd_heatmaps_to_keypoints_aug: one launch, the combination made while each
              workgroup loads its map,
  (c) plain   vd_heatmaps_to_keypoints on one view: the floor (b) cannot beat,
  host        once: the views copied to the host, and the numpy restatement of the
              combination (tests/kps_aug_ref.py) on an evenly spaced sample of the rows,
              scaled to all rows.

(a), (b) and (c) alternate inside every round of one process, HIP events around each call
after a warm-up; median and 10th..90th percentile per path.  The verdict for shipping (b)
as the pipeline's route: its median may exceed (a)'s by at most (a)'s own p10..p90 spread.
The boxes are the detections the e2e_keypoint_rcnn_R-50-FPN_1x pipeline makes on two
seeded 320 x 480 frames, scaled to 800 x 1333 and repeated to the row count (as
tools/bench_keypoints.py draws them); the heatmaps are seeded normal logits x 3.

--step adds one whole-step comparison: KeypointFramePipeline against
KeypointAugFramePipeline with six keypoint views (H_FLIP, scales 600 and 1000,
SCALE_H_FLIP) on one 800 x 1333 frame, wall clock around synchronised steps.

  python tools/bench_kps_aug.py [--rows 6400] [--rounds 12] [--cpu-rows 320] [--step]

One JSON line per heuristic (HM_AVG, HM_AVG with AREA_TH, HM_MAX), then the step line.
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
from vosdetectron_amd import config as vcfg, keypoints, ops  # noqa: E402

HFLIP = [False, True, False, True, False, True]
DS = [False, False, True, True, False, False]
US = [False, False, False, False, True, True]


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 3),
            "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 3),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 3)}


def interleaved(fns, rounds, warmup=2):
    """{name: [ms per round]}: every round runs each path once, in the same order."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}


def torch_route(views, perm_t, heur, boxes, min_size):
    ts = [v.index_select(1, perm_t).flip(3) if hf else v for v, hf in zip(views, HFLIP)]
    st = torch.stack(ts)
    comb = st.mean(0) if heur == "HM_AVG" else st.amax(0)
    return ops.heatmaps_to_keypoints(comb, boxes, min_size), comb


def bench_boxes(dev, rows):
    import bench
    from vosdetectron_amd.engine import KeypointFramePipeline
    from vosdetectron_amd.weights import build_model
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
    return cfg, model, np.resize(src * sc, (rows, 4)).astype(np.float32)


def whole_step(dev, model, iters=5):
    """Seconds per synchronised step, plain and with six keypoint views, one frame."""
    import bench
    from vosdetectron_amd.engine import KeypointAugFramePipeline, KeypointFramePipeline
    frames = torch.from_numpy(bench.synthetic_frames(1, 5, 800, 1333)).to(dev)
    cfg = vcfg.get("e2e_keypoint_rcnn_R-50-FPN_1x")
    aug = vcfg.get("e2e_keypoint_rcnn_R-50-FPN_1x")
    aug.TEST.KPS_AUG.update(ENABLED=True, H_FLIP=True, SCALES=(600, 1000), MAX_SIZE=2000,
                            SCALE_H_FLIP=True)
    kw = dict(frame_hw=(800, 1333), batch=1, channels_last=True, device=dev)
    pipes = {"plain": KeypointFramePipeline(model, cfg, **kw),
             "kps_aug_6_views": KeypointAugFramePipeline(model, aug, **kw)}
    res = {}
    for _ in range(2):  # warm-up: the views' convolution shapes search on their first run
        for p in pipes.values():
            p.run(frames)
    torch.cuda.synchronize()
    times = {k: [] for k in pipes}
    for _ in range(iters):
        for k, p in pipes.items():
            t0 = time.perf_counter()
            out = p.run(frames)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
            res[k + "_detections"] = int(sum(out["counts_host"]))
    for k, v in times.items():
        res[k] = stats(v)
    res["views"] = [list(v) for v in pipes["kps_aug_6_views"].kps_views]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6400)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--cpu-rows", type=int, default=320)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kps_aug needs a GPU")
    from tests import kps_aug_ref as kar
    dev = torch.device("cuda")
    cfg, model, boxes_np = bench_boxes(dev, a.rows)
    K, S, V = cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.HEATMAP_SIZE, len(HFLIP)
    min_size = cfg.KRCNN.INFERENCE_MIN_SIZE
    g = torch.Generator(device="cuda").manual_seed(3)
    views = [torch.randn((a.rows, K, S, S), device=dev, generator=g) * 3 for _ in range(V)]
    boxes = torch.from_numpy(boxes_np).to(dev)
    perm_t = torch.tensor(keypoints.flip_permutation(), device=dev)
    area = kar.boxes_area(boxes_np)
    th = float(np.sort(area)[len(area) // 2])  # the median area: a float32, so exact
    view_bytes = a.rows * K * S * S * 4

    # the host route, once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [v.cpu() for v in views]
    d2h_s = time.perf_counter() - t0
    idx = np.linspace(0, a.rows - 1, a.cpu_rows).astype(int)
    sample = [h.numpy()[idx] for h in host]
    del host
    t0 = time.perf_counter()
    ref, _ = kar.combine(sample, HFLIP, "HM_AVG", DS, US, boxes_np[idx], th)
    np_s = time.perf_counter() - t0
    host_line = {"d2h_all_views_s": round(d2h_s, 3), "d2h_bytes": V * view_bytes,
                 "numpy_combine_rows_timed": int(len(idx)), "numpy_combine_s": round(np_s, 3),
                 "numpy_combine_scaled_to_all_rows_s": round(np_s * a.rows / len(idx), 2)}
    _, got = ops.heatmaps_to_keypoints_aug([v[idx] for v in views], HFLIP, DS, US, boxes[idx],
                                           min_size, "HM_AVG", th, want_combined=True)
    host_line["numpy_equals_device"] = bool(np.array_equal(got.cpu().numpy(), ref))

    for heur, area_th in (("HM_AVG", None), ("HM_AVG", th), ("HM_MAX", None)):
        fns = {"torch": lambda: torch_route(views, perm_t, heur, boxes, min_size),
               "fused": lambda: ops.heatmaps_to_keypoints_aug(views, HFLIP, DS, US, boxes,
                                                              min_size, heur, area_th),
               "plain": lambda: ops.heatmaps_to_keypoints(views[0], boxes, min_size)}
        if area_th is not None:  # torch has no per-row view choice to compare with
            del fns["torch"]
        ms = interleaved(fns, a.rounds)
        line = {"heur": heur, "area_th": area_th, "rows": a.rows, "views": V, "keypoints": K,
                "heatmap": S, "rounds": a.rounds, "view_bytes": view_bytes}
        line.update({k: stats(v) for k, v in ms.items()})
        b, c = line["fused"]["median_ms"], line["plain"]["median_ms"]
        line["fused_over_plain"] = round(b / c, 2)
        line["fused_read_gb_per_s"] = round(
            (V if area_th is None else V - 2) * view_bytes / (b * 1e-3) / 1e9, 1)
        if "torch" in ms:
            ta = line["torch"]
            spread = round(ta["p90_ms"] - ta["p10_ms"], 3)
            line.update(torch_spread_ms=spread, fused_minus_torch_ms=round(b - ta["median_ms"], 3),
                        ship_fused=bool(b - ta["median_ms"] <= spread))
            kt, ct = torch_route(views, perm_t, heur, boxes, min_size)
            kf, cf = ops.heatmaps_to_keypoints_aug(views, HFLIP, DS, US, boxes, min_size, heur,
                                                   want_combined=True)
            line["combined_max_abs_diff_vs_torch"] = float((ct - cf).abs().max())
            # torch's mean is not np.mean bit for bit, so the logits may differ in the last
            # place and an argmax between near-equal values may move
            line["keypoints_xy_equal_torch"] = round(float(
                (kt[:, :2] == kf[:, :2]).all(dim=1).float().mean()), 6)
            line["logit_max_abs_diff_vs_torch"] = float((kt[:, 2] - kf[:, 2]).abs().max())
            del kt, ct, kf, cf
        print(json.dumps(line), flush=True)
    print(json.dumps({"host_route": host_line}), flush=True)
    if a.step:
        del views
        torch.cuda.empty_cache()
        print(json.dumps({"whole_step_800x1333_ms": whole_step(dev, model)}), flush=True)


if __name__ == "__main__":
    main()
