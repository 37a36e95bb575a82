#!/usr/bin/env python
"""Aspect-ratio views: what the one-launch blob (vd_image_aspect_resize_to_blob) costs
against the two routes that give a blob of the same size, and what two such views add
to a step.

  blob   F = 64 seeded frames of 800 x 1333, ar 0.5 and 2.0, plain and flipped, NHWC,
         at (TEST.SCALE, TEST.MAX_SIZE) = (800, 1333).  Three variants, alternated inside
         every round of one process:
           aspect    ops.image_aspect_resize_to_blob on the frames (im_ar never written)
           resize    ops.image_resize_to_blob on seeded frames that already are H x War:
                     the existing launch producing a blob of the same output size
           two_step  a torch composition that materialises the u8 im_ar on the device
                     (gathers of the two tap columns, int32 multiply-add with the
                     2048-scale coefficients, the shifts, a flip for a flipped view),
                     then ops.image_resize_to_blob on it; checked equal to `aspect`
         Times are HIP-event intervals around --iters back-to-back calls, per call;
         median and min..max over --rounds rounds after a warm-up round.  Bytes are the
         algorithm's: `aspect` reads the frames once and writes the blob; `resize` reads
         its H x War frames and writes the blob; `two_step` reads the frames, writes and
         reads im_ar, and writes the blob (its int32 intermediates are not counted).
         hbm_peak_fraction = bytes / time / 8.0 TB/s (the MI355X's specified peak; a
         float4 copy reaches 0.79 of it).
  step   one R-50-FPN AugFramePipeline step (synthetic weights, channels_last, F = 1,
         800 x 1333) with the identity view alone and with the views of ASPECT_RATIOS
         (0.5, 2.0) added to TEST.BBOX_AUG and TEST.MASK_AUG: host clock around
         run() (which ends in a device synchronise), median and min..max over --steps.

One JSON line per measurement, appended to --out when given.

  python tools/bench_aspect_views.py [--frames 64] [--iters 20] [--rounds 7] [--steps 10]
                                     [--what blob,step] [--out FILE]
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
TEST_SCALE, TEST_MAX = 800, 1333
STRIDE = 32
HBM_PEAK = 8.0e12


def stage1_tables(W, War, dev):
    """The per-column taps and coefficients of the 8-bit width resize (vosdet.h)."""
    scale = 1.0 / (float(War) / float(W))
    dx = np.arange(War)
    fx = ((dx + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo, hi = sx < 0, sx >= W - 1
    fx[lo], sx[lo] = 0, 0
    fx[hi], sx[hi] = 0, W - 1
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int32)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return t(sx), t(np.minimum(sx + 1, W - 1)), t(a0)[None, None, :, None], \
        t(a1)[None, None, :, None]


def torch_im_ar(frames, tables, hflip):
    sx, sx1, a0, a1 = tables
    d = frames.index_select(2, sx).to(torch.int32) * a0 \
        + frames.index_select(2, sx1).to(torch.int32) * a1
    im_ar = (((d >> 9) + 2) >> 2).to(torch.uint8)
    return im_ar.flip(2).contiguous() if hflip else im_ar


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # microseconds per call


def spread(us, nbytes):
    a = np.sort(np.asarray(us))
    med = float(np.median(a))
    return {"median_us": round(med, 1), "min_us": round(float(a[0]), 1),
            "max_us": round(float(a[-1]), 1), "bytes": int(nbytes),
            "hbm_peak_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}


def blob_lines(F, iters, rounds, dev):
    from vosdetectron_amd import ops
    H, W = HW
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(dev)
    lut = torch.from_numpy(ops.pixel_lut()).to(dev)
    lines = []
    for ar in (0.5, 2.0):
        War = ops.aspect_width(W, ar)
        scale = ops.target_scale(H, War, TEST_SCALE, TEST_MAX)
        Hr, Wr = ops.resized_hw(H, War, scale)
        Hp, Wp = -(-Hr // STRIDE) * STRIDE, -(-Wr // STRIDE) * STRIDE
        same_size = torch.from_numpy(rng.integers(0, 256, (F, H, War, 3), dtype=np.uint8)).to(dev)
        tables = stage1_tables(W, War, dev)
        out = torch.empty((F, Hp, Wp, 3), dtype=torch.float32, device=dev)
        out2 = torch.empty_like(out)
        blob_b, src_b, ar_b = out.numel() * 4, frames.numel(), same_size.numel()
        for hflip in (False, True):
            variants = {
                "aspect": (lambda: ops.image_aspect_resize_to_blob(
                    frames, lut, ar, scale, Hp, Wp, hflip=hflip, nhwc=True, out=out),
                    src_b + blob_b),
                "resize": (lambda: ops.image_resize_to_blob(
                    same_size, lut, scale, Hp, Wp, nhwc=True, out=out2), ar_b + blob_b),
                "two_step": (lambda: ops.image_resize_to_blob(
                    torch_im_ar(frames, tables, hflip), lut, scale, Hp, Wp, nhwc=True, out=out2),
                    src_b + 2 * ar_b + blob_b)}
            variants["aspect"][0]()
            variants["two_step"][0]()
            torch.cuda.synchronize()
            equal = bool(torch.equal(out, out2))
            us = {k: [] for k in variants}
            for r in range(rounds + 1):
                for k, (fn, _) in variants.items():  # alternated inside every round
                    t = timed(fn, iters)
                    if r:  # round 0 warms every variant
                        us[k].append(t)
            line = {"what": "aspect_blob", "frames": F, "frame_hw": list(HW), "ar": ar,
                    "hflip": hflip, "War": War, "im_scale": scale,
                    "path": "area2" if scale == 0.5 else "linear", "blob_hw": [Hp, Wp],
                    "layout": "nhwc", "iters": iters, "rounds": rounds,
                    "two_step_equals_aspect": equal,
                    **{k: spread(us[k], variants[k][1]) for k in variants}}
            lines.append(line)
            print(json.dumps(line), flush=True)
        del same_size, out, out2
        torch.cuda.empty_cache()
    return lines


def step_lines(steps, warmup, dev):
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import AugFramePipeline
    from vosdetectron_amd.weights import build_model
    frames = torch.from_numpy(np.random.RandomState(1000).randint(
        0, 256, (1,) + HW + (3,), np.uint8)).to(dev)
    model, lines = None, []
    for ratios in ((), (0.5, 2.0)):
        cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
        for aug in (cfg.TEST.BBOX_AUG, cfg.TEST.MASK_AUG):
            aug.update(ENABLED=True, ASPECT_RATIOS=ratios)
        vcfg.check_supported(cfg, test_aug=True, aspect_views=True)
        if model is None:
            model, _ = build_model(cfg, device=dev, channels_last=True)
        pipe = AugFramePipeline(model, cfg, frame_hw=HW, batch=1, device=dev, channels_last=True)
        for _ in range(warmup):
            pipe.run(frames)
        ms = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.run(frames)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        a = np.sort(np.asarray(ms))
        line = {"what": "aspect_step", "frames": 1, "frame_hw": list(HW),
                "aspect_ratios": list(ratios), "box_views": len(pipe.box_views),
                "mask_views": len(pipe.mask_views), "detections": out["counts_host"],
                "steps": steps, "warmup": warmup, "median_ms": round(float(np.median(a)), 3),
                "min_ms": round(float(a[0]), 3), "max_ms": round(float(a[-1]), 3)}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del pipe
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", default="blob,step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_aspect_views: no GPU; nothing is measured without one")
    dev = torch.device("cuda")
    lines = []
    if "blob" in a.what.split(","):
        lines += blob_lines(a.frames, a.iters, a.rounds, dev)
    if "step" in a.what.split(","):
        lines += step_lines(a.steps, a.warmup, dev)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
