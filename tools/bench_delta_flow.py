#!/usr/bin/env python
"""The delta-flow head (MODEL.USE_DELTA_FLOW) of the dynamic VOS step: the torch
composition against the two HIP launches, by the method of tools/bench_flow_prep.py.

  (a) composition: per level conv3x3 (C -> 2, MIOpen) + tanh, the difference with
      the previous feature, bilinear upsample to the blob, division by the scale
      and the sum (data_flow), then the five FlowAlign conv_flow_downsample convs;
  (b) ops.delta_flow_features + ops.delta_flow_to_levels (two launches);
  (c) each of the two launches alone.

Shape: 16 frames, C = 256, blob 512 x 896 (the VOS bench step), channels_last
pyramids.  One pyramid set is 626 MB, more than the 256 MiB Infinity Cache; the
calls of a window cycle through `--sets` of them, so the features come from HBM.
A window is `--calls` back-to-back calls replayed as a hipGraph between two HIP
events; the paths alternate over `--reps` windows after a warm-up; per-call median
and 10th..90th percentile over the windows.

Algorithmic bytes: the features read once, the state read and written, the deltas
written (launch 1); the deltas read and the levels written (launch 2); both for
(b).  hbm_fraction = bytes / time / 8 TB/s.  One JSON line per path.

  python tools/bench_delta_flow.py [--calls 6] [--reps 11] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vosdetectron_amd import ops  # noqa: E402
from vosdetectron_amd.vos import FlowAlign  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
STRIDES = ops.FLOW_STRIDES[::-1]  # 64 .. 4: [P6 .. P2]


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
    """run() as a replayable hipGraph, captured on a stream of its own after a
    warm-up there."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--blob", type=int, nargs=2, default=(512, 896))
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_delta_flow needs a GPU")
    dev = torch.device("cuda")
    B, C, (Hp, Wp) = a.frames, a.channels, a.blob
    g = torch.Generator(device="cuda").manual_seed(3)
    hw = [(Hp // k, Wp // k) for k in STRIDES]
    sets = [[torch.randn((B, C, h, w), device=dev, generator=g).contiguous(
        memory_format=torch.channels_last) for h, w in hw] for _ in range(a.sets)]
    convs = [torch.nn.Conv2d(C, 2, 3, 1, 1, bias=False).to(dev).to(
        memory_format=torch.channels_last) for _ in STRIDES]
    for c in convs:
        c.weight.data.normal_(0, 0.02, generator=g)
    weights = [c.weight.detach() for c in convs]
    mods = [FlowAlign(1.0 / k).to(dev) for k in STRIDES]
    state = [torch.zeros((B, 2, h, w), device=dev) for h, w in hw]
    valid = torch.ones((B,), dtype=torch.int32, device=dev)
    prev = [torch.zeros((B, 2, h, w), device=dev) for h, w in hw]
    deltas = [torch.rand((B, 2, h, w), device=dev, generator=g) * 2 - 1 for h, w in hw]

    def composition(feats):
        flow = torch.zeros((B, 2, Hp, Wp), device=dev)
        for i, k in enumerate(STRIDES):
            feat = torch.tanh(convs[i](feats[i]))
            d = feat - prev[i]
            prev[i].copy_(feat)
            flow = flow + F.interpolate(d, scale_factor=float(k), mode="bilinear",
                                        align_corners=False) * float(k)
        return [m.conv_flow_downsample(flow) for m in mods]

    def features(feats):
        return ops.delta_flow_features(feats, weights, state, valid)

    def to_levels(d):
        return ops.delta_flow_to_levels(d, Hp, Wp)[0]

    def fused(feats):
        return to_levels(features(feats))

    with torch.no_grad():
        for _ in range(2):  # warm-up: code objects, MIOpen's algorithm choice
            for s in sets:
                composition(s)
                fused(s)
        torch.cuda.synchronize()
        n = a.calls
        runs = {"composition": lambda: [composition(sets[i % a.sets]) for i in range(n)],
                "two_launches": lambda: [fused(sets[i % a.sets]) for i in range(n)],
                "features_only": lambda: [features(sets[i % a.sets]) for i in range(n)],
                "to_levels_only": lambda: [to_levels(deltas) for i in range(n)]}
        runs = {k: captured(v) for k, v in runs.items()}
        ev = {k: [] for k in runs}
        for _ in range(a.reps):  # alternate the paths
            for k, run in runs.items():
                ev[k].append(timed(run))
        torch.cuda.synchronize()
        # same numbers: both paths from the same previous feature on the same pyramid
        for p, s in zip(prev, state):
            s.copy_(p)
        diff = [float((x - y).abs().max()) for x, y in zip(fused(sets[0]), composition(sets[0]))]
    t = {k: stats([x.elapsed_time(y) * 1e3 / n for x, y in v]) for k, v in ev.items()}
    feat_bytes = sum(B * C * h * w * 4 for h, w in hw)
    small = sum(B * 2 * h * w * 4 for h, w in hw)
    bytes_ = {"features_only": feat_bytes + 3 * small, "to_levels_only": 2 * small}
    bytes_["two_launches"] = bytes_["features_only"] + bytes_["to_levels_only"]
    lines = []
    for k in ("composition", "two_launches", "features_only", "to_levels_only"):
        rec = {"path": k, "frames": B, "channels": C, "blob_hw": [Hp, Wp],
               "calls_per_window": n, "windows": a.reps, "pyramid_sets": a.sets}
        rec.update(t[k])
        if k in bytes_:
            rec["algorithmic_bytes"] = bytes_[k]
            rec["hbm_fraction_of_8TBps"] = round(
                bytes_[k] / (t[k]["median_us"] * 1e-6) / HBM_PEAK, 3)
        if k == "two_launches":
            rec["speedup_median"] = round(t["composition"]["median_us"] / t[k]["median_us"], 2)
            rec["ranges_overlap"] = bool(t[k]["p90_us"] >= t["composition"]["p10_us"])
            rec["max_abs_diff_vs_composition_P6_to_P2"] = diff
        lines.append(json.dumps(rec))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
