#!/usr/bin/env python
"""Label maps as DAVIS annotation files: what encoding the PNGs on the device
(vd_label_pngs) costs against the route it replaces.

Shapes: 16 frames of 480 x 854 and 64 frames of 800 x 1333.  The maps are ops.label_maps'
`label` on the synthetic detections of tools/bench_label_map.py (100 per frame, box sizes
drawn from a real R-50-FPN step), made once outside every timed window.

  (a)  ops.label_pngs: png_strip_kernel + png_frame_kernel.  Device time between two HIP
       events over windows of `--calls` calls after a warm-up, as a replayed hipGraph and
       eagerly: the median over `--reps` windows.
  (b)  (a) + vis.png_bytes: the files as `bytes` on the host (one read of the lengths, one
       copy of the streams up to the longest).  Wall clock around a synchronised call,
       median of `--reps`.
  (c)  the route before: the label maps copied to the host (timed by itself), then
       PIL.Image.save(..., 'PNG') of a 'P' image per frame into memory -- on one thread,
       on 16 threads of this process, and on 16 worker processes (started and warmed
       outside the window; the maps reach them pickled, which is part of that route).
       Wall clock, median of `--host-reps`.

Every stream of (a) is decoded with PIL and compared with its map.  Sizes of (a)'s files
and PIL's are given per shape.  One JSON line per shape, appended to --out when given.

  python tools/bench_label_png.py [--calls 5] [--reps 21] [--host-reps 5] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 16


def pil_encode(job):
    """One frame's file as PIL writes it (runs in the workers too: no torch here)."""
    from PIL import Image
    raw, h, w, pal = job
    im = Image.frombytes("P", (w, h), raw)
    im.putpalette(pal)
    b = io.BytesIO()
    im.save(b, "PNG")
    return b.getvalue()


def _median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def _wall(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(_median(ts), 1), "min_us": round(min(ts), 1),
            "max_us": round(max(ts), 1), "n": len(ts)}


def shape_line(F, h, w, a, dev, pool):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_label_map as blm
    from bench_oks_nms import captured, windows
    from vosdetectron_amd import ops, vis
    sizes = blm.step_box_sizes(h, w, dev)
    host = blm.make_inputs(F, h, w, sizes, 7 * F + h)
    t = [torch.from_numpy(x).to(dev) for x in host]
    label, _ = ops.label_maps(t[0], t[1], t[2], t[3], h, w, blm.THRESH, blm.GT_THRESH)
    pal = vis.davis_palette().to(dev)
    pal_bytes = vis.davis_palette().numpy().tobytes()
    out = torch.empty((F, ops.label_png_bound(h, w)), dtype=torch.uint8, device=dev)

    def encode():
        return ops.label_pngs(label, pal, out)

    for _ in range(3):
        streams, lengths = encode()
    files = vis.png_bytes(streams, lengths)
    maps = label.cpu().numpy()
    from PIL import Image
    decoded = True
    for f in range(F):
        im = Image.open(io.BytesIO(files[f]))
        im.load()
        decoded = decoded and im.mode == "P" and np.array_equal(np.asarray(im), maps[f])
    runs = {"eager": lambda: [encode() for _ in range(a.calls)]}
    runs["graph"] = captured(runs["eager"])
    tm = windows(runs, a.reps, a.calls)
    b = _wall(lambda: vis.png_bytes(*encode()), a.reps)

    # (c) the route before
    torch.set_num_threads(1)
    d2h = _wall(lambda: label.cpu(), a.reps)

    def jobs():
        m = label.cpu().numpy()
        return [(m[f].tobytes(), h, w, pal_bytes) for f in range(F)]

    pil_files = [pil_encode(j) for j in jobs()]
    c1 = _wall(lambda: [pil_encode(j) for j in jobs()], a.host_reps)
    with ThreadPoolExecutor(THREADS) as tp:
        list(tp.map(pil_encode, jobs()))
        c16t = _wall(lambda: list(tp.map(pil_encode, jobs())), a.host_reps)
    pool.map(pil_encode, jobs())
    c16p = _wall(lambda: pool.map(pil_encode, jobs()), a.host_reps)
    ours = np.array([len(x) for x in files])
    theirs = np.array([len(x) for x in pil_files])
    best_c = min(c1["median_us"], c16t["median_us"], c16p["median_us"])
    return {"what": "vd_label_pngs", "frames": F, "frame_hw": [h, w],
            "label_nonzero_share": round(float((label != 0).float().mean()), 3),
            "calls_per_window": a.calls, "windows": a.reps, "streams_decode_to_maps": bool(decoded),
            "a_device_graph": tm["graph"], "a_device_eager": tm["eager"],
            "b_device_plus_png_bytes_wall": b,
            "c_d2h_label_maps_wall": d2h, "c_d2h_bytes": int(F * h * w),
            "c_d2h_plus_pil_1_thread_wall": c1, "c_d2h_plus_pil_16_threads_wall": c16t,
            "c_d2h_plus_pil_16_processes_wall": c16p,
            "b_d2h_bytes": int(F * int(ours.max())),
            "file_bytes_device": {"mean": round(float(ours.mean()), 1), "min": int(ours.min()),
                                  "max": int(ours.max())},
            "file_bytes_pil": {"mean": round(float(theirs.mean()), 1), "min": int(theirs.min()),
                               "max": int(theirs.max())},
            "raw_bytes_per_frame": h * w,
            "best_c_over_b": round(best_c / b["median_us"], 1),
            "device_route_is_faster": bool(b["median_us"] < best_c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--shapes", default="16x480x854,64x800x1333")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import multiprocessing as mp
    pool = mp.get_context("spawn").Pool(THREADS)  # before the GPU is opened; workers never open it
    try:
        pool.map(pil_encode, [(b"\0" * 12, 3, 4, b"\0" * 768)] * (4 * THREADS))
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_label_png needs a GPU")
        dev = torch.device("cuda")
        for spec in a.shapes.split(","):
            F, h, w = (int(v) for v in spec.split("x"))
            s = json.dumps(shape_line(F, h, w, a, dev, pool))
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(s + "\n")
    finally:
        pool.terminate()
        pool.join()


if __name__ == "__main__":
    main()
