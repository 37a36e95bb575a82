#!/usr/bin/env python3
"""The F(4x4) Winograd block plan (csrc/conv3x3_wino4.hip) per shape: HIP-event us per
call of the stacked entry under today's layout (VOSDET_WINO4_PLAN=0), the planner's
choice (unset) and any forced plans given, with the block counts the planner reports,
so a planned shape's time can be set against its predicted ratio (blocks / blocks
today).  One JSON line per shape.
usage: tools/bench_wino4_plan.py [--plans tall,1 wide,4 ...] [NxCxHxWxCout ...]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vosdetectron_amd import ops  # noqa: E402

DEFAULT = ["64x256x200x336x256", "64x64x200x336x64", "64x256x100x168x256",
           "64x128x100x168x128", "64x256x50x84x256", "64x256x25x42x256",
           "64x512x25x42x512"]


def timed(fn, iters=10):
    s = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def with_plan(plan, fn):
    if plan is None:
        os.environ.pop("VOSDET_WINO4_PLAN", None)
    else:
        os.environ["VOSDET_WINO4_PLAN"] = plan
    try:
        return fn()
    finally:
        os.environ.pop("VOSDET_WINO4_PLAN", None)


def main():
    args = sys.argv[1:]
    plans = []
    if args and args[0] == "--plans":
        args = args[1:]
        while args and not args[0][0].isdigit():
            plans.append(args.pop(0))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for N, C, H, W, Co in ([int(v) for v in a.split("x")] for a in (args or DEFAULT)):
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(N, C, H, W, device="cuda", generator=g).contiguous(
            memory_format=torch.channels_last)
        w = torch.randn(Co, C, 3, 3, device="cuda", generator=g) / (9 * C) ** .5
        b = torch.randn(Co, device="cuda", generator=g)
        u = ops.conv3x3_wino4_weight(w)
        out = torch.empty((N, Co, H, W), device="cuda").contiguous(
            memory_format=torch.channels_last)
        run = lambda: ops.conv3x3_wino4_bias_act(x, u, b, relu=True, out=out, mosaic="rows")
        row = {"shape": [N, C, H, W, Co], "n_cu": n_cu}
        ref = None
        for plan in ["0", None] + plans:
            p = with_plan(plan, lambda: ops.conv3x3_wino4_plan(N, H, W, C, Co, True, n_cu))
            us = with_plan(plan, lambda: timed(run))
            y = out.clone()
            ref = y if ref is None else ref
            row["auto" if plan is None else plan] = {
                "plan": list(p), "us": round(us, 1), "bit_identical": bool(torch.equal(ref, y))}
        b0 = row["0"]
        for k, v in row.items():
            if isinstance(v, dict) and k != "0":
                v["blocks_ratio"] = round(v["plan"][2] / b0["plan"][2], 4)
                v["time_ratio"] = round(v["us"] / b0["us"], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
