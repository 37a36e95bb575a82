#!/usr/bin/env python
"""Flow preparation of the dynamic VOS step: what the five FlowAlign
conv_flow_downsample convolutions cost, and what the one vd_flow_to_levels launch
that replaces them (and the host-side flo_to_blob) costs.

  (a) parent path: the blob-resolution flow F x 2 x Hp x Wp is already on the
      device; the five frozen 2 -> 2 convs (kernel = stride = 64, 32, 16, 8, 4)
      run exactly as the FlowAlign modules run them (MIOpen, fp32);
  (b) ops.flow_to_levels on the raw F x H x W x 2 flow: resize, scale, pad and
      the five block sums in one launch.

Shapes: the VOS bench step (16 frames of 480 x 854, scale 1, blob 512 x 896) and a
scaled one (16 frames of 720 x 1280 at 480/720, blob 512 x 896).  Both paths read
a different input buffer every call, out of a ring larger than the 256 MiB
Infinity Cache, so the reads come from HBM.  A window is `--calls` back-to-back
calls between two HIP events; it is timed both as a replayed hipGraph (device time,
no host work between the kernels: the headline figures) and eagerly (what a caller
sees, host enqueue included).  The paths alternate over `--reps` windows after a
warm-up; per-call median and 10th..90th percentile over the windows.

Algorithmic bytes of (b): the raw flow read once + the five levels written;
hbm_fraction = bytes / time / 8 TB/s (the HBM3E peak; a float4 copy reaches 0.79).
(a)'s bytes are the blob flow read once per conv + the levels.  One JSON line per
shape, appended to --out when given.

  python tools/bench_flow_prep.py [--calls 20] [--reps 15] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vosdetectron_amd import ops  # noqa: E402
from vosdetectron_amd.vos import FlowAlign  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
RING_BYTES = 640 << 20
STRIDES = ops.FLOW_STRIDES


def stats(us):
    a = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(a)), 2),
            "p10_us": round(float(a[int(0.1 * (len(a) - 1))]), 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]), 2)}


def timed(run):
    """One timed window: run() between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    return e0, e1


def captured(run):
    """run() as a replayable hipGraph (captured on a stream of its own after a
    warm-up there): the window then holds the kernels with no host work between."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        run()
    torch.cuda.synchronize()
    return g.replay


def shape_line(F, H, W, im_scale, calls, reps, dev):
    Hr, Wr = ops.resized_hw(H, W, im_scale)
    Hp, Wp = -(-Hr // 64) * 64, -(-Wr // 64) * 64
    g = torch.Generator(device="cuda").manual_seed(7)
    raw_bytes, blob_bytes = F * H * W * 2 * 4, F * 2 * Hp * Wp * 4
    n_raw = max(2, -(-RING_BYTES // raw_bytes))
    n_blob = max(2, -(-RING_BYTES // blob_bytes))
    raws = [(torch.rand((F, H, W, 2), device=dev, generator=g) - 0.5) * 12 for _ in range(n_raw)]
    blobs = [ops.flow_to_levels(raws[i % n_raw], im_scale, Hp, Wp, want_blob=True)[1]
             for i in range(n_blob)]
    mods = [FlowAlign(1.0 / k).to(dev) for k in STRIDES[::-1]]  # the model's order: 1/64 .. 1/4

    def parent(blob):
        return [m.conv_flow_downsample(blob) for m in mods]

    def new(raw):
        return ops.flow_to_levels(raw, im_scale, Hp, Wp)

    with torch.no_grad():
        for _ in range(3):  # warm-up: code objects, MIOpen's algorithm choice
            for b in blobs[:2]:
                parent(b)
            for r in raws[:2]:
                new(r)
        torch.cuda.synchronize()
        runs = {"parent": lambda: [parent(blobs[i % n_blob]) for i in range(calls)],
                "new": lambda: [new(raws[i % n_raw]) for i in range(calls)]}
        runs.update({k + "_graph": captured(v) for k, v in list(runs.items())})
        ev = {k: [] for k in runs}
        for _ in range(reps):  # alternate the paths
            for k, run in runs.items():
                ev[k].append(timed(run))
        torch.cuda.synchronize()
        # same numbers: the new levels against the parent's convs on the same flow
        lv, blob = ops.flow_to_levels(raws[0], im_scale, Hp, Wp, want_blob=True)
        diff = {k: float((a - b).abs().max()) for k, a, b in zip(STRIDES, lv, parent(blob)[::-1])}
    t = {k: stats([a.elapsed_time(b) * 1e3 / calls for a, b in v]) for k, v in ev.items()}
    level_bytes = sum(F * 2 * (Hp // k) * (Wp // k) * 4 for k in STRIDES)
    new_bytes = raw_bytes + level_bytes
    parent_bytes = 5 * blob_bytes + level_bytes
    dt_new = t["new_graph"]["median_us"]
    return {
        "frames": F, "frame_hw": [H, W], "im_scale": round(im_scale, 6), "resized_hw": [Hr, Wr],
        "blob_hw": [Hp, Wp], "calls_per_window": calls, "windows": reps,
        "ring_buffers": {"raw": n_raw, "blob": n_blob},
        "parent_five_convs": t["parent_graph"], "new_one_launch": t["new_graph"],
        "parent_five_convs_eager": t["parent"], "new_one_launch_eager": t["new"],
        "speedup_median": round(t["parent_graph"]["median_us"] / dt_new, 2),
        "new_algorithmic_bytes": new_bytes,
        "new_hbm_fraction_of_8TBps": round(new_bytes / (dt_new * 1e-6) / HBM_PEAK, 3),
        "parent_algorithmic_bytes": parent_bytes,
        "parent_hbm_fraction_of_8TBps": round(
            parent_bytes / (t["parent_graph"]["median_us"] * 1e-6) / HBM_PEAK, 3),
        "max_abs_diff_new_vs_parent": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_prep needs a GPU")
    dev = torch.device("cuda")
    for F, H, W, s in ((16, 480, 854, 1.0), (16, 720, 1280, 480.0 / 720.0)):
        line = json.dumps(shape_line(F, H, W, s, a.calls, a.reps, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
