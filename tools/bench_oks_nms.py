#!/usr/bin/env python
"""keypoint_results' OKS NMS: what the vd_nms_oks_frames launch sequence costs, against
the reference's route and inside the keypoint step.

  kernel   ops.nms_oks_frames (the per-frame NMS launch + the gather launch) on F frames
           of n clustered poses (the fixture generator's, tools/gen_goldens.py), D = 256,
           threshold 0.3.  A window is `--calls` back-to-back calls between two HIP
           events, timed as a replayed hipGraph (device time: the headline) and eagerly
           (host enqueue included); per-call median and 10th..90th percentile over
           `--reps` windows after a warm-up.  Shapes: F = 64 and F = 2, n = 100.
  (a)      the reference's route on the same data: keyps / dets / counts copied to the
           host (.cpu(), which waits for the device) and the numpy loop of
           tests/oks_ref.py per frame, one thread; wall clock, median over --cpu-reps.
           Its keep lists are compared with the device's.
  (b)      the keypoint step of tools/bench_keypoints.py's pipeline (R-50-FPN keypoint
           config with person as the only class, two 320 x 480 seeded frames, run
           (sync=False)) with nms_oks off -- the step as it was -- and on, alternating,
           as replayed hipGraphs and eagerly.  The on - off difference stands next to
           the kernel's own time at the step's F and counts.

One JSON line per measurement, appended to --out when given.

  python tools/bench_oks_nms.py [--calls 20] [--reps 15] [--cpu-reps 3] [--out FILE]
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
from vosdetectron_amd import ops  # noqa: E402

D = 256


def stats(us):
    a = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(a)), 2),
            "p10_us": round(float(a[int(0.1 * (len(a) - 1))]), 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]), 2)}


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    return e0, e1


def captured(run):
    """run() as a replayable hipGraph, captured on a stream of its own after a warm-up."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        keep = run()
    torch.cuda.synchronize()
    return lambda: (g.replay(), keep)[0]  # keep: the captured calls' tensors stay alive


def windows(runs, reps, per_window):
    """Alternate the runs over `reps` windows: {name: per-call stats}."""
    ev = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            ev[k].append(timed(run))
    torch.cuda.synchronize()
    return {k: stats([a.elapsed_time(b) * 1e3 / per_window for a, b in v])
            for k, v in ev.items()}


def pose_frames(F, n, seed):
    from gen_goldens import _clustered_poses
    keyps, dets = [], np.zeros((F, D, 5), np.float32)
    for f in range(F):
        kp, rois, _ = _clustered_poses(np.random.default_rng(seed + f), n)
        keyps.append(kp)
        dets[f, :n, :4] = rois
        dets[f, :n, 4] = np.linspace(0.99, 0.05, n, dtype=np.float32)
    return (np.concatenate(keyps), dets, np.ones((F, D), np.int32),
            np.full((F,), n, np.int32))


def kernel_line(F, n, calls, reps, cpu_reps, dev):
    from tests import oks_ref
    host = pose_frames(F, n, 1000)
    t = [torch.from_numpy(a).to(dev) for a in host]

    def call():
        return ops.nms_oks_frames(*t, thresh=0.3)
    for _ in range(3):
        res = call()
    torch.cuda.synchronize()
    runs = {"eager": lambda: [call() for _ in range(calls)]}
    runs["graph"] = captured(runs["eager"])
    tm = windows(runs, reps, calls)
    # (a) the reference's route: D2H of what the loop reads, then the loop per frame
    torch.set_num_threads(1)
    cpu, keeps = [], None
    for _ in range(cpu_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kp, de, cn = t[0].cpu().numpy(), t[1].cpu().numpy(), t[3].cpu().numpy()
        t1 = time.perf_counter()
        keeps, o = [], 0
        for f in range(F):
            keeps.append(oks_ref.nms_oks(kp[o:o + cn[f]], de[f, :cn[f], :4], 0.3))
            o += cn[f]
        cpu.append((t1 - t0, time.perf_counter() - t1))
    got_keep, got_cnt = res.keep.cpu().numpy(), res.counts.cpu().numpy()
    same = all(got_keep[f, :got_cnt[f]].tolist() == keeps[f] for f in range(F))
    copy_us = float(np.median([c[0] for c in cpu])) * 1e6
    loop_us = float(np.median([c[1] for c in cpu])) * 1e6
    pairs = F * n * (n - 1) // 2
    return {"what": "vd_nms_oks_frames", "frames": F, "rows_per_frame": n, "det_cap": D,
            "thresh": 0.3, "kept_per_frame_mean": round(float(got_cnt.mean()), 1),
            "calls_per_window": calls, "windows": reps,
            "device_graph": tm["graph"], "device_eager": tm["eager"],
            "pair_tests_upper_bound": pairs,
            "reference_route_host": {"d2h_copy_us": round(copy_us, 1),
                                     "numpy_loop_us": round(loop_us, 1),
                                     "total_us": round(copy_us + loop_us, 1),
                                     "reps": cpu_reps, "keep_equal_device": bool(same)},
            "host_route_over_device_graph": round((copy_us + loop_us)
                                                  / tm["graph"]["median_us"], 1)}


def step_line(reps, dev):
    import bench
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import KeypointFramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("e2e_keypoint_rcnn_R-50-FPN_1x")
    cfg.MODEL.NUM_CLASSES = 2
    model, _ = build_model(cfg, seed=0, device=dev, channels_last=True)
    kw = dict(frame_hw=(320, 480), batch=2, channels_last=True, device=dev)
    frames = torch.from_numpy(bench.synthetic_frames(2, 21, 320, 480)).to(dev)
    pipes = {"off": KeypointFramePipeline(model, cfg, **kw),
             "on": KeypointFramePipeline(model, cfg, nms_oks=True, **kw)}
    outs = {}
    for k, p in pipes.items():
        for _ in range(3):
            outs[k] = p.run(frames)
    torch.cuda.synchronize()
    runs = {k: (lambda p=p: p.run(frames, sync=False)) for k, p in pipes.items()}
    runs.update({k + "_graph": captured(v) for k, v in list(runs.items())})
    tm = windows(runs, reps, 1)
    # the kernel alone on the step's own pre-NMS tensors
    pre = pipes["on"].run(frames, keep_intermediates=True)
    args = [pre[k + "_pre_oks"] for k in ("keyps", "dets", "classes", "counts")]
    calls = 20
    alone = {"eager": lambda: [ops.nms_oks_frames(*args, thresh=0.3) for _ in range(calls)]}
    alone["graph"] = captured(alone["eager"])
    ta = windows(alone, reps, calls)
    return {"what": "keypoint step, nms_oks off / on", "frames": 2, "frame_hw": [320, 480],
            "counts_pre_nms": pre["counts_pre_oks_host"], "counts_post_nms": pre["counts_host"],
            "off_counts": outs["off"]["counts_host"], "windows": reps,
            "step_off_graph": tm["off_graph"], "step_on_graph": tm["on_graph"],
            "step_off_eager": tm["off"], "step_on_eager": tm["on"],
            "on_minus_off_graph_us": round(tm["on_graph"]["median_us"]
                                           - tm["off_graph"]["median_us"], 2),
            "on_minus_off_eager_us": round(tm["on"]["median_us"] - tm["off"]["median_us"], 2),
            "kernel_alone_graph": ta["graph"], "kernel_alone_eager": ta["eager"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_oks_nms needs a GPU")
    dev = torch.device("cuda")
    lines = [kernel_line(64, 100, a.calls, a.reps, a.cpu_reps, dev),
             kernel_line(2, 100, a.calls, a.reps, a.cpu_reps, dev)]
    with torch.no_grad():
        lines.append(step_line(a.reps, dev))
    for ln in lines:
        s = json.dumps(ln)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
