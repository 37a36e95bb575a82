#!/usr/bin/env python
"""Per-kernel A/B of the split GEMMs: the six-product bf16 kernel (gemm_split3_bias_act)
against the three-product fp16 one (gemm_h2_bias_act) on the GEMM shapes of one 64-frame
R-50-FPN step (800 x 1344 frames, 1000 RoIs per frame for the box head, 100 for the mask
head).  HIP events, 10 launches after 2 warm-ups, the mean per launch; one JSON line per
shape and a table.  The table decides ops.h2_route.

    python tools/bench_gemm_h2.py [--frames 64] [--out FILE.jsonl] [--cfg-sweep]

--cfg-sweep adds the three-product kernel's time at every tile configuration that serves
the shape (h2_cfg1 .. h2_cfg5) beside the automatic choice.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vosdetectron_amd import ops  # noqa: E402

DEV = torch.device("cuda")


def shapes(frames):
    px = lambda s: frames * (800 // s) * (1344 // s)  # noqa: E731
    rois, mrois = frames * 1000, frames * 100
    # name, M, N, K, kind, extra
    return [
        ("fc6", rois, 1024, 12544, "plain", None),
        ("fc7", rois, 1024, 1024, "plain", None),
        ("cls+bbox", rois, 448, 1024, "norelu", None),
        ("res2 conv1 256->64", px(4), 64, 256, "plain", None),
        ("res2 conv3+downsample (64+64)->256", px(4), 256, 128, "a2", 64),
        ("res3 conv1 512->128", px(8), 128, 512, "plain", None),
        ("res3 conv3 128->512 +res", px(8), 512, 128, "res", None),
        ("res3 downsample s2 256->512", px(8), 512, 256, "s2", (200, 336)),
        ("res4 conv1 1024->256", px(16), 256, 1024, "plain", None),
        ("res4 conv3 256->1024 +res", px(16), 1024, 256, "res", None),
        ("res4 downsample s2 512->1024", px(16), 1024, 512, "s2", (100, 168)),
        ("res5 conv1 2048->512", px(32), 512, 2048, "plain", None),
        ("res5 conv3 512->2048 +res", px(32), 2048, 512, "res", None),
        ("P5 conv_top 2048->256", px(32), 256, 2048, "norelu", None),
        ("P4 lateral 1024->256", px(16), 256, 1024, "up", (50, 84)),
        ("P3 lateral 512->256", px(8), 256, 512, "up", (100, 168)),
        ("P2 lateral 256->256", px(4), 256, 256, "up", (200, 336)),
        ("mask tail", mrois * 196, 1024, 256, "mask", 14),
    ]


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, M, N, K, kind, extra, frames, sweep=False):
    g = torch.Generator(device="cuda").manual_seed(1)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** .5
    b = torch.randn(N, device=DEV, generator=g) * .1
    kw = dict(relu=kind != "norelu" and kind != "up")
    if kind == "s2":
        H, W = extra
        a = torch.randn(frames * H * W, K, device=DEV, generator=g).relu_()
        kw.update(sub_hw=(H, W), relu=False)
    elif kind == "a2":
        a = torch.randn(M, K - extra, device=DEV, generator=g).relu_()
        kw.update(a2=torch.randn(M, extra, device=DEV, generator=g).relu_())
    else:
        a = torch.randn(M, K, device=DEV, generator=g).relu_()
    if kind == "res":
        kw.update(residual=torch.randn(M, N, device=DEV, generator=g))
    if kind == "up":
        kw.update(residual=torch.randn(M // 4, N, device=DEV, generator=g), up_hw=extra)
    w6, w3 = ops.gemm_split3_weight(w), ops.gemm_h2_weight(w)
    if kind == "mask":
        cw = torch.randn(81, 256, device=DEV, generator=g) / 16
        cb = torch.randn(81, device=DEV, generator=g)
        ch = torch.randint(1, 81, (M // 196,), device=DEV, generator=g, dtype=torch.int32)
        out = torch.empty(M // 196, 28, 28, device=DEV)
        six = lambda: ops.mask_head_upconv_logits(a, w6, b, cw, cb, ch, extra, out=out)  # noqa
        h2 = lambda: ops.mask_head_upconv_logits(a, w3, b, cw, cb, ch, extra, out=out)  # noqa
    else:
        out = torch.empty(M, N, device=DEV)
        six = lambda: ops.gemm_split3_bias_act(a, w6, b, out=out, **kw)  # noqa: E731
        h2 = lambda: ops.gemm_h2_bias_act(a, w3, b, out=out, **kw)  # noqa: E731
    t6, t3 = timed(six), timed(h2)
    row = dict(shape=name, M=M, N=N, K=K, six_ms=round(t6, 4), h2_ms=round(t3, 4),
               speedup=round(t6 / t3, 3), h2_route=ops.h2_route(M, N, K))
    if sweep and kind != "mask":
        for cfg in (1, 2, 3, 4, 5):
            if N % {1: 256, 2: 128, 3: 64, 4: 128, 5: 256}[cfg] == 0:
                row["h2_cfg%d" % cfg] = round(timed(
                    lambda: ops.gemm_h2_bias_act(a, w3, b, out=out, cfg=cfg, **kw)), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cfg-sweep", action="store_true")
    args = ap.parse_args()
    rows = []
    for s in shapes(args.frames):
        rows.append(run(*s, frames=args.frames, sweep=args.cfg_sweep))
        print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rows[-1]) + "\n")
        torch.cuda.empty_cache()
    print("\n| shape | M | N | K | six-product ms | three-product ms | speed-up | routed |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %(shape)s | %(M)d | %(N)d | %(K)d | %(six_ms).3f | %(h2_ms).3f | %(speedup).2f "
              "| %(h2_route)s |" % r)
    print("sum: six %.2f ms, h2 %.2f ms" % (sum(r["six_ms"] for r in rows),
                                             sum(r["h2_ms"] for r in rows)))


if __name__ == "__main__":
    main()
