#!/usr/bin/env python
"""viz_mask_result's label maps: what the vd_label_maps launch costs against the two
routes a user had before it.

Shapes: 16 frames of 480 x 854 and 64 frames of 800 x 1333, 100 detections per frame at
det_cap 256, 28 x 28 masks, thresh 0.25, rvt_cls_threshold 0.6.  The box sizes are drawn
(with replacement) from the detections of a real step of the R-50-FPN engine on seeded
frames of that size; centres are uniform over the frame, scores are distinct.

  (a)  ops.label_maps: the prep + paint launches (and the few torch ops that cut the counts
       to the mask rows), label and gt.
  (b)  the device composition out of kernels the parent commit has: ops.paste_masks planes
       of every detection, then torch: the planes times their painting rank (0 = not
       painted), the maximum over a frame's detections, and a gather of id / gt id.  The
       rank tables are made outside the timed window (in (b)'s favour).  Its maps are
       compared with (a)'s.
  (c)  the host route: segm.encode_masks (the fused RLE launch, the strings copied to the
       host), dets / classes copied to the host (timed separately), then numpy: every RLE
       decoded and the planes painted as the reference does.  One thread, wall clock; on
       the first --host-frames frames of the step (decoding is seconds), scaled to F.

(a) and (b) are timed over `--reps` alternating windows of `--calls` calls between two HIP
events after a warm-up, as replayed hipGraphs (device time: the headline) and eagerly.
bytes_written / time of (a) is given as a share of the 8 TB/s HBM peak.

One JSON line per shape, appended to --out when given.

  python tools/bench_label_map.py [--calls 5] [--reps 9] [--host-frames 8] [--out FILE]
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
from vosdetectron_amd import ops, segm  # noqa: E402

CAP, N, R = 256, 100, 28
THRESH, GT_THRESH = 0.25, 0.6
HBM_PEAK = 8e12


def step_box_sizes(h, w, dev):
    """(w, h) of every detection of one real engine step on two seeded h x w frames."""
    import bench
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.e2e_mask_rcnn_R_50_FPN_1x()
    cfg.TEST.SCALE = h
    model, _ = build_model(cfg, seed=0, device=dev, channels_last=True)
    pipe = FramePipeline(model, cfg, frame_hw=(h, w), batch=2, device=dev, channels_last=True)
    with torch.no_grad():
        out = pipe.run(torch.from_numpy(bench.synthetic_frames(2, 31, h, w)).to(dev))
    d = np.concatenate([out["dets"][f, :k].cpu().numpy()
                        for f, k in enumerate(out["counts_host"])])
    assert len(d) >= 16, "the step found too few detections to draw sizes from"
    return np.stack([d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]], 1)


def make_inputs(F, h, w, sizes, seed):
    from tests.label_map_ref import blob
    rng = np.random.default_rng(seed)
    protos = np.stack([blob(rng, R) for _ in range(64)])
    masks = protos[rng.integers(0, len(protos), F * N)]
    wh = sizes[rng.integers(0, len(sizes), (F, N))]
    c = np.stack([rng.uniform(0, w, (F, N)), rng.uniform(0, h, (F, N))], 2)
    dets = np.zeros((F, CAP, 5), np.float32)
    dets[:, :N, :4] = np.concatenate([c - wh / 2, c + wh / 2], 2)
    for f in range(F):  # distinct scores, a fifth of them under the threshold
        dets[f, :N, 4] = rng.permutation(np.linspace(0.05, 0.99, N))
    classes = np.zeros((F, CAP), np.int32)
    classes[:, :N] = rng.integers(1, 81, (F, N))
    return masks, dets, classes, np.full((F,), N, np.int32)


def rank_tables(dets, classes):
    """Per frame: weight [F,N] uint8 = 1 + painting rank (0: not painted), and the id / gt
    id of each weight [F,N+1] uint8 (entry 0 = 0)."""
    from tests.label_map_ref import order_of
    F = dets.shape[0]
    weight = np.zeros((F, N), np.uint8)
    ids, gids = np.zeros((F, N + 1), np.uint8), np.zeros((F, N + 1), np.uint8)
    for f in range(F):
        for r, i in enumerate(order_of(dets[f, :N, 4], THRESH)):
            weight[f, i] = r + 1
            ids[f, r + 1] = classes[f, i]
            gids[f, r + 1] = classes[f, i] if dets[f, i, 4] > np.float32(GT_THRESH) else 0
    return weight, ids, gids


def host_route(t, F, h, w, frames):
    """(c) on the first `frames` frames: (rle_us, d2h_us, numpy_us), each scaled to F."""
    from tests.label_map_ref import paint, rle_decode
    masks, dets, classes = t["masks"][:frames * N], t["dets"][:frames], t["classes"][:frames]
    boxes = dets[:, :N].reshape(-1, 5).contiguous()
    torch.set_num_threads(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rles = segm.encode_masks(masks, boxes, h, w, 0.5)
    t1 = time.perf_counter()
    d, c = dets.cpu().numpy(), classes.cpu().numpy()
    t2 = time.perf_counter()
    maps = []
    for f in range(frames):
        planes = np.stack([rle_decode(r) for r in rles[f * N:(f + 1) * N]])
        maps.append(paint(planes, d[f, :N, 4], c[f, :N], THRESH, GT_THRESH))
    t3 = time.perf_counter()
    k = F / frames * 1e6
    return (t1 - t0) * k, (t2 - t1) * k, (t3 - t2) * k, maps


def shape_line(F, h, w, a, dev):
    sizes = step_box_sizes(h, w, dev)
    host = make_inputs(F, h, w, sizes, 7 * F + h)
    t = dict(zip(("masks", "dets", "classes", "counts"),
                 [torch.from_numpy(x).to(dev) for x in host]))
    boxes = t["dets"][:, :N].reshape(-1, 5).contiguous()
    weight, ids, gids = (torch.from_numpy(x).to(dev) for x in rank_tables(host[1], host[2]))
    planes = torch.empty((F * N, h, w), dtype=torch.uint8, device=dev)

    def new():
        return ops.label_maps(t["masks"], t["dets"], t["classes"], t["counts"], h, w, THRESH,
                              GT_THRESH)

    def composed():
        pv = ops.paste_masks(t["masks"], boxes, h, w, 0.5, out=planes).view(F, N, h, w)
        pv.mul_(weight[:, :, None, None])
        best = pv.amax(1).view(F, -1).long()
        return (torch.gather(ids, 1, best).view(F, h, w),
                torch.gather(gids, 1, best).view(F, h, w))

    for _ in range(2):
        got, ref = new(), composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]))
    runs = {"a_eager": lambda: [new() for _ in range(a.calls)],
            "b_eager": lambda: [composed() for _ in range(a.calls)]}
    runs["a_graph"] = captured(runs["a_eager"])
    runs["b_graph"] = captured(runs["b_eager"])
    tm = windows(runs, a.reps, a.calls)
    hf = min(a.host_frames, F)
    rle_us, d2h_us, numpy_us, maps = host_route(t, F, h, w, hf)
    host_same = all(np.array_equal(got[0][f].cpu().numpy(), maps[f][0]) and
                    np.array_equal(got[1][f].cpu().numpy(), maps[f][1]) for f in range(hf))
    a_us, b_us = tm["a_graph"]["median_us"], tm["b_graph"]["median_us"]
    written = 2 * F * h * w
    wh = np.sort(sizes.prod(1))
    return {"what": "vd_label_maps", "frames": F, "frame_hw": [h, w], "dets_per_frame": N,
            "det_cap": CAP, "mask_size": R, "thresh": THRESH, "gt_thresh": GT_THRESH,
            "box_area_quartiles_px": [round(float(wh[int(q * (len(wh) - 1))])) for q in
                                      (0.25, 0.5, 0.75)],
            "label_nonzero_share": round(float((got[0] != 0).float().mean()), 3),
            "calls_per_window": a.calls, "windows": a.reps,
            "a_label_maps_graph": tm["a_graph"], "a_label_maps_eager": tm["a_eager"],
            "b_paste_torch_graph": tm["b_graph"], "b_paste_torch_eager": tm["b_eager"],
            "b_equal_a": same, "b_over_a_graph": round(b_us / a_us, 1),
            "a_bytes_written": written,
            "a_written_share_of_hbm_peak": round(written / (a_us * 1e-6) / HBM_PEAK, 4),
            "c_host_route": {"frames_timed": hf, "scaled_to_frames": F,
                             "rle_and_strings_us": round(rle_us, 1),
                             "d2h_dets_classes_us": round(d2h_us, 1),
                             "numpy_decode_paint_us": round(numpy_us, 1),
                             "total_us": round(rle_us + d2h_us + numpy_us, 1),
                             "equal_a": bool(host_same)},
            "c_over_a_graph": round((rle_us + d2h_us + numpy_us) / a_us, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--shapes", default="16x480x854,64x800x1333")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_map needs a GPU")
    dev = torch.device("cuda")
    for spec in a.shapes.split(","):
        F, h, w = (int(v) for v in spec.split("x"))
        s = json.dumps(shape_line(F, h, w, a, dev))
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
