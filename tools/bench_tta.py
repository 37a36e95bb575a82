#!/usr/bin/env python
"""Test-time augmentation: what an AugFramePipeline step costs, by stage, and the union
stage against the only route the code before it offered for the same result.

  step     R-50-FPN (synthetic weights, channels_last) on seeded 800 x 1333 frames with
           the 18 box + 18 mask views of e2e_mask_rcnn_X-152-32x8d-FPN-IN5k_1.44x.yaml
           (H_FLIP, SCALES 400..1200 at MAX_SIZE 2000, SCALE_H_FLIP; UNION, SOFT_AVG, box
           voting AVG at 0.9), F = 1 and F = 4 frames per step.  Stage times are HIP-event
           intervals on the launch stream (engine.FramePipeline.enable_timers), summed
           over a step's views; median and 10th..90th percentile over --steps steps after
           --warmup steps:
             views      blob + body + RPN + proposals + box RoIAlign + box head of the
                        18 views (marks conv_body, proposals, box_head)
             add_view   vd_box_union_add_view x 18
             union      vd_box_union_detections (+ post-filter): mark misc_bbox
             masks      the 18 mask views + vd_mask_aug_accumulate / _finish
  host     the union stage the way it had to be done before: the per-view rois, scores
           and deltas copied to the host (.cpu(), which waits for the device), then the
           numpy decode + flip + vstack + box_results_with_nms_and_limit of the oracle,
           per frame; wall clock, once (--host 0 skips it), WITHOUT box voting (the
           oracle's voting is a Python loop of minutes at these sizes), next to the
           device's union stage without voting.  Its detections are compared with the
           device's.

One JSON line per measurement, appended to --out when given.

  python tools/bench_tta.py [--steps 5] [--warmup 2] [--frames 1,4] [--out FILE]
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

HW = (800, 1333)
SCALES = (400, 500, 600, 700, 900, 1000, 1100, 1200)
GROUPS = {"views": ("conv_body", "proposals", "box_head"), "add_view": ("union_add_view",),
          "union": ("misc_bbox",), "masks": ("im_detect_mask",)}


def config(vote=True):
    from vosdetectron_amd import config as vcfg
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    for aug in (cfg.TEST.BBOX_AUG, cfg.TEST.MASK_AUG):
        aug.update(ENABLED=True, H_FLIP=True, SCALES=SCALES, MAX_SIZE=2000, SCALE_H_FLIP=True)
    cfg.TEST.BBOX_VOTE.update(ENABLED=vote, VOTE_TH=0.9, SCORING_METHOD="AVG")
    vcfg.check_supported(cfg, test_aug=True)
    return cfg


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 3),
            "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 3),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 3)}


def step_line(pipe, frames, steps, warmup):
    for _ in range(warmup):
        pipe.run(frames)
    per = {k: [] for k in GROUPS}
    per["step"] = []
    for _ in range(steps):
        pipe.enable_timers()
        out = pipe.run(frames)
        t = pipe.timers
        for k, names in GROUPS.items():
            per[k].append(1e3 * sum(t[n].total_time for n in names if n in t))
        per["step"].append(1e3 * sum(v.total_time for v in t.values()))
    pipe.enable_timers(False)
    return {k: stats(v) for k, v in per.items()}, out


def host_union(cfg, pipe, frames):
    """The per-view outputs to the host + the oracle's union, per frame."""
    from oracle import oracle as orc
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import aug_ref
    out = pipe.run(frames, keep_intermediates=True)
    torch.cuda.synchronize()
    tst, K = cfg.TEST, cfg.MODEL.NUM_CLASSES
    t0 = time.perf_counter()
    host = {v: {k: out["views"][v][k].cpu() for k in ("rois", "roi_counts", "cls_prob",
                                                      "bbox_pred")} for v in pipe.box_views}
    t1 = time.perf_counter()
    same = True
    for f in range(frames.shape[0]):
        scores_ts, boxes_ts = [], []
        for v in pipe.box_views:
            o = host[v]
            n, post = int(o["roi_counts"][f]), o["rois"].shape[1]
            scores_ts.append(o["cls_prob"].view(-1, post, K)[f, :n].numpy())
            boxes_ts.append(aug_ref.decode_view(
                o["rois"][f, :n].numpy(), o["bbox_pred"].view(-1, post, 4 * K)[f, :n].numpy(),
                np.float32(pipe.geom[v].scale), HW + (3,), v[2],
                tuple(cfg.MODEL.BBOX_REG_WEIGHTS)))
        sc, bx = aug_ref.union(scores_ts, boxes_ts)
        s, b, _ = orc.box_results_with_nms_and_limit(
            sc, bx, K, tst.SCORE_THRESH, tst.NMS, tst.DETECTIONS_PER_IM)
        k = out["counts_host"][f]
        d = out["dets"][f, :k].cpu().numpy()
        same = same and k == len(s) and np.array_equal(d[:, :4], b) and np.array_equal(d[:, 4], s)
    t2 = time.perf_counter()
    return {"d2h_ms": round(1e3 * (t1 - t0), 2), "numpy_union_ms": round(1e3 * (t2 - t1), 1),
            "rows_per_frame": int(sc.shape[0]), "equal_to_device": bool(same),
            "largest_list": int(out["cand_counts"].max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", default="1,4")
    ap.add_argument("--host", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    from vosdetectron_amd.engine import AugFramePipeline
    from vosdetectron_amd.weights import build_model
    dev = torch.device("cuda")
    cfg = config()
    model, _ = build_model(cfg, device=dev, channels_last=True)
    lines = []
    for F in [int(x) for x in a.frames.split(",")]:
        frames = torch.from_numpy(np.stack([
            np.random.RandomState(1000 + i).randint(0, 256, HW + (3,), np.uint8)
            for i in range(F)])).to(dev)
        pipe = AugFramePipeline(model, cfg, frame_hw=HW, batch=F, device=dev, channels_last=True)
        st, out = step_line(pipe, frames, a.steps, a.warmup)
        line = {"what": "tta_step", "frames": F, "box_views": len(pipe.box_views),
                "mask_views": len(pipe.mask_views), "cand_cap": pipe.cand_cap,
                "detections": out["counts_host"], "largest_list": int(out["cand_counts"].max()),
                "steps": a.steps, "warmup": a.warmup, **st}
        lines.append(line)
        print(json.dumps(line), flush=True)
        if a.host and F == 1:
            plain = config(vote=False)
            p2 = AugFramePipeline(model, plain, frame_hw=HW, batch=F, device=dev,
                                  channels_last=True)
            st2, _ = step_line(p2, frames, a.steps, 1)
            line = {"what": "tta_union_host_route", "frames": F, "box_vote": False,
                    "device_union": st2["union"], "device_add_view": st2["add_view"],
                    **host_union(plain, p2, frames)}
            del p2
            lines.append(line)
            print(json.dumps(line), flush=True)
        del pipe
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
