#!/usr/bin/env python
"""The VOS tail's mask-IoU NMS: what one vd_mask_iou_nms_frames call over all rows of a
step costs against the per-row planes loop it replaces.

Shapes: 16 rows of 480 x 854 with 100 and with 10 detections each, 64 rows of 800 x 1333
with 100 each (skipped, with the size it asked for, when its workspace exceeds the
default budget); det_cap 256, 28 x 28 masks, NMS_WITH_MASK_IOU 0.5,
NUM_DET_PER_CLASS_POST 1.  Inputs: tests/mask_nms_frames_ref.gen_frame (clustered
boxes, logistic-disc masks, scores in sixteenths).

  (a)  ops.mask_iou_nms_frames with the previous-frame record: one call, no host read.
  (b)  the device work of the loop frame_results ran before: per row ops.paste_masks
       into n x H x W planes, then ops.mask_iou_nms with its .item().  Its keep lists
       are compared with (a)'s.
  (c)  VOSPipeline.frame_results on a completed step as wall time (host clock, ends in
       a synchronise): the per-row loop as it was before finalize(), restated here, and
       the current one.  Both include the per-row RLE encoding, which did not change.

(a) and (b) alternate, one call per window between two HIP events, `--reps` windows each
after a warm-up; median and spread (max - min, and the 10th..90th percentile range).
The speed-up is stated only when (a)'s median is below (b)'s by more than the sum of
the two 10..90 spreads.

--step also times finalize() against the stages of a 16-row VOS step of the test
configuration (enable_timers), for the tail's share of a step.

One JSON line per shape, appended to --out when given.

  python tools/bench_mask_nms_frames.py [--reps 25] [--step] [--out FILE]
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
from vosdetectron_amd import ops, segm  # noqa: E402

CAP, R = 256, 28
IOU_TH, PER_CLASS, BIN = 0.5, 1, 0.5
BUDGET = 1 << 30
K = 81


def make_inputs(F, n, h, w, seed):
    from tests.mask_nms_frames_ref import gen_frame
    rng = np.random.default_rng(seed)
    dets = np.zeros((F, CAP, 5), np.float32)
    classes = np.zeros((F, CAP), np.int32)
    masks = []
    for f in range(F):
        m, d, c = gen_frame(rng, n, h, w, R)
        dets[f, :n], classes[f, :n] = d, c
        masks.append(m)
    return np.concatenate(masks), dets, classes, np.full((F,), n, np.int32)


def stats(us):
    us = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(us[0]), 1),
            "max_us": round(float(us[-1]), 1),
            "spread_p10_p90_us": round(float(np.percentile(us, 90) - np.percentile(us, 10)), 1),
            "windows": len(us)}


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def wall_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


class TailOnly:
    """The attributes VOSPipeline.frame_results / finalize read, without a model: the
    tail of a step whose detections and masks are given."""

    def __new__(cls, F, h, w, dev):
        from vosdetectron_amd import config as vcfg
        from vosdetectron_amd.engine import VOSPipeline
        p = object.__new__(VOSPipeline)
        cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_davis")
        cfg.TEST.NMS_WITH_MASK_IOU, cfg.TEST.NUM_DET_PER_CLASS_POST = IOU_TH, PER_CLASS
        cfg.MODEL.NUM_CLASSES = K
        p.cfg, p.H, p.W, p.device, p.det_cap = cfg, h, w, dev, CAP
        p.prev_dets = torch.zeros((F, CAP, 5), device=dev)
        p.prev_classes = torch.zeros((F, CAP), dtype=torch.int32, device=dev)
        p.prev_counts = torch.zeros((F,), dtype=torch.int32, device=dev)
        p._unfinalized = False
        return p


def frame_results_before(pipe, out):
    """VOSPipeline.frame_results as it was before finalize(): per row paste_masks,
    mask_iou_nms, three device-to-host copies and the previous-frame writes."""
    ks = [int(k) for k in out["counts_host"]]
    res, start = [], 0
    for f, k in enumerate(ks):
        dets, classes = out["dets"][f, :k], out["classes"][f, :k]
        masks = out["masks"][start:start + k]
        start += k
        rles = segm.encode_masks(masks, dets, pipe.H, pipe.W, BIN)
        keep = torch.arange(k, device=pipe.device)
        if k:
            planes = ops.paste_masks(masks, dets, pipe.H, pipe.W, BIN)
            keep = ops.mask_iou_nms(planes, dets, classes, IOU_TH, PER_CLASS)
        kd, kc = dets[keep], classes[keep]
        n = kd.shape[0]
        pipe.prev_dets[f, :n] = kd
        pipe.prev_classes[f, :n] = kc
        pipe.prev_counts[f] = n
        kd_h, kc_h = kd.cpu().numpy(), kc.cpu().tolist()
        kept = keep.cpu().tolist()
        cls_boxes = [np.zeros((0, 5), np.float32) for _ in range(K)]
        cls_segms = [[] for _ in range(K)]
        for j in sorted(set(kc_h)):
            rows = [i for i, c in enumerate(kc_h) if c == j]
            cls_boxes[j] = kd_h[rows]
            cls_segms[j] = [rles[kept[i]] for i in rows]
        res.append((cls_boxes, cls_segms))
    return res


def shape_line(F, n, h, w, a, dev):
    line = {"what": "vd_mask_iou_nms_frames", "rows": F, "frame_hw": [h, w],
            "dets_per_row": n, "det_cap": CAP, "mask_size": R, "iou_th": IOU_TH,
            "max_per_class": PER_CLASS}
    size = ops.mask_iou_nms_frames_workspace(F, CAP, F * n, h, w)
    line["workspace_bytes"] = size
    line["planes_bytes_per_row"] = n * h * w
    if size > BUDGET:
        line["skipped"] = "workspace above the default budget of %d bytes" % BUDGET
        return line
    host = make_inputs(F, n, h, w, 7 * F + h + n)
    m, d, c, cnt = (torch.from_numpy(x).to(dev) for x in host)
    prev = (torch.zeros((F, CAP, 5), device=dev),
            torch.zeros((F, CAP), dtype=torch.int32, device=dev),
            torch.zeros((F,), dtype=torch.int32, device=dev))

    def new():
        return ops.mask_iou_nms_frames(m, d, c, cnt, h, w, IOU_TH, PER_CLASS, BIN, prev=prev)

    def before():
        keeps = []
        for f in range(F):
            planes = ops.paste_masks(m[f * n:(f + 1) * n], d[f, :n], h, w, BIN)
            keeps.append(ops.mask_iou_nms(planes, d[f, :n], c[f, :n], IOU_TH, PER_CLASS))
        return keeps

    for _ in range(3):
        got, ref = new(), before()
    torch.cuda.synchronize()
    kc = got[1].cpu().tolist()
    line["b_equal_a"] = all(got[0][f, :kc[f]].cpu().tolist() == ref[f].cpu().tolist()
                            for f in range(F))
    line["kept_per_row_mean"] = round(float(np.mean(kc)), 1)
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(event_time(new))
        tb.append(event_time(before))
    sa, sb = stats(ta), stats(tb)
    line["a_frames_call"], line["b_per_row_planes_loop"] = sa, sb
    clear = sa["median_us"] + sa["spread_p10_p90_us"] + sb["spread_p10_p90_us"] < sb["median_us"]
    line["a_below_b_by_more_than_the_spreads"] = bool(clear)
    if clear:
        line["b_over_a"] = round(sb["median_us"] / sa["median_us"], 1)

    pipe = TailOnly(F, h, w, dev)

    def completed():
        return {"masks": m, "dets": d, "classes": c, "counts": cnt,
                "counts_host": [n] * F}

    r0 = frame_results_before(pipe, completed())
    r1 = pipe.frame_results(completed())
    line["c_results_equal"] = all(
        all(np.array_equal(x, y) for x, y in zip(b0, b1)) and s0 == s1
        for (b0, s0), (b1, s1) in zip(r0, r1))
    wb, wn = [], []
    for _ in range(max(5, a.reps // 4)):
        wb.append(wall_time(lambda: frame_results_before(pipe, completed())))
        wn.append(wall_time(lambda: pipe.frame_results(completed())))
    line["c_frame_results_before_wall"], line["c_frame_results_now_wall"] = stats(wb), stats(wn)
    return line


def step_line(a, dev):
    """finalize() next to the stages of a 16-row VOS step of the test configuration."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import VOSPipeline
    from vosdetectron_amd.weights import build_model
    F, h, w = 16, 480, 854
    cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_davis")
    cfg.TEST.NMS_SMALL_BOX_IOU = 0.3
    cfg.TEST.NMS_SMALL_BOX_SCORE_THRESHOLD = 0.0
    cfg.TEST.NMS_WITH_MASK_IOU = 0.5
    cfg.TEST.NUM_DET_PER_CLASS_POST = 1
    frames = [np.stack([np.random.RandomState(600 + 10 * i + r).randint(0, 256, (h, w, 3),
                                                                      np.uint8)
                        for r in range(F)]) for i in range(3)]
    model, _ = build_model(cfg, device=dev, channels_last=True, calibrate_frame=frames[0][0])
    pipe = VOSPipeline(model, cfg, frame_hw=(h, w), batch=F, device=dev, channels_last=True)
    dev_frames = [torch.from_numpy(f).to(dev) for f in frames]
    for fr in dev_frames:  # warm-up
        pipe.finalize(pipe.run(fr, sync=False))
    pipe.reset()
    pipe.enable_timers()
    tail, dets = [], []
    for _ in range(max(2, a.reps // 3)):
        for fr in dev_frames:
            out = pipe.run(fr, sync=False)
            tail.append(event_time(lambda: pipe.finalize(out)))
            dets.append(float(out["counts"].float().mean()))
        pipe.reset()
    stages = {k: round(v * 1e6, 1) for k, v in pipe.timer_summary().items()}
    step_us = sum(stages.values())
    st = stats(tail)
    return {"what": "VOSPipeline.finalize in a step", "rows": F, "frame_hw": [h, w],
            "config": "vos_R-101-FPN_3x_gn_dynamic_davis, both heuristics on, random weights",
            "dets_per_row_mean": round(float(np.mean(dets)), 1), "stage_mean_us": stages,
            "step_us": round(step_us, 1), "finalize": st,
            "finalize_share_of_step_plus_tail": round(st["median_us"] /
                                                      (step_us + st["median_us"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--shapes", default="16x100x480x854,16x10x480x854,64x100x800x1333")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_nms_frames needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda")
    lines = [lambda s=spec: shape_line(*(int(v) for v in s.split("x")), a, dev)
             for spec in a.shapes.split(",") if spec]
    if a.step:
        lines.append(lambda: step_line(a, dev))
    for make in lines:
        s = json.dumps(make())
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
