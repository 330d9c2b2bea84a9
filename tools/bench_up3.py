#!/usr/bin/env python3
"""up_3 of the PSPNet decoder alone (3x3 conv, 64 -> 64 channels, on the x2 upsample of its input; f16x3) at the two shapes of the headline
configuration: the patch-resident plan the tuner used to pick (the fastest of tile_cfg 13 / 15 / 20 / 21 / 22, chosen here the same way)
against the persistent kernel (tile_cfg 23, csrc/conv_up2_c64.hip).

    python tools/bench_up3.py [--json FILE] [--windows 7] [--window-s 0.25] [--shapes 11x256x512,1x512x1024]

The two plans are timed in interleaved windows (old, new, old, new, ...) of at least --window-s seconds each, HIP events around each window;
per plan the median window and the spread (max - min) / median of its windows are reported.  One JSON object on stdout."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

OLD_CFGS = (13, 15, 20, 21, 22)


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return 1e3 * s.elapsed_time(e) / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--shapes", default="11x256x512,1x512x1024", help="N x H x W of the conv (upsampled) size")
    args = ap.parse_args()
    if args.windows < 5 or args.window_s < 0.2:
        ap.error("at least 5 windows of at least 0.2 s")
    from arseg_amd import _lib, ops
    from arseg_amd.packing import PackedConv

    ops.set_conv_math("f16x3")
    dev = torch.device("cuda:0")
    g = np.random.Generator(np.random.PCG64(5))
    w = torch.from_numpy((g.standard_normal((64, 64, 3, 3)) * np.sqrt(2.0 / (9 * 64))).astype(np.float32))
    pc = PackedConv(w, None, (torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64)), 1, 1, 1, _lib.ACT_PRELU, 0.25, dev)
    rows = []
    for shape in args.shapes.split(","):
        N, H, W = (int(v) for v in shape.split("x"))
        x = torch.from_numpy(g.standard_normal((N, H // 2, W // 2, 64)).astype(np.float32)).to(dev)
        out = torch.empty((N, H, W, 64), device=dev)
        flops = 2.0 * N * H * W * 64 * 9 * 64
        first = {}
        for cfg in OLD_CFGS:
            try:
                ops.conv2d(x, pc, out=out, up2=True, tile_cfg=cfg, split_k=1)
                first[cfg] = window(lambda: ops.conv2d(x, pc, out=out, up2=True, tile_cfg=cfg, split_k=1), 30)
            except _lib.ArsegError:
                pass
        old_cfg = min(first, key=first.get)
        plans = {"old": lambda: ops.conv2d(x, pc, out=out, up2=True, tile_cfg=old_cfg, split_k=1),
                 "new": lambda: ops.conv2d(x, pc, out=out, up2=True, tile_cfg=23, split_k=1)}
        plans["old"]()
        ref = out.clone()
        plans["new"]()
        diff = float((out - ref).abs().max())
        reps = {k: max(10, int(args.window_s * 1e6 / window(f, 20)) + 1) for k, f in plans.items()}
        us = {"old": [], "new": []}
        for _ in range(args.windows):
            for k in ("old", "new"):
                us[k].append(window(plans[k], reps[k]))
        row = {"N": N, "H": H, "W": W, "gflop": flops / 1e9, "old_cfg": old_cfg, "old_candidates_us": {str(k): round(v, 2) for k, v in first.items()},
               "max_abs_new_vs_old": diff}
        for k in ("old", "new"):
            med = statistics.median(us[k])
            row[k] = {"us_median": round(med, 2), "us_windows": [round(v, 2) for v in us[k]], "spread": round((max(us[k]) - min(us[k])) / med, 4),
                      "calls_per_window": reps[k], "tflops": round(flops / med / 1e6, 1)}
        row["speedup"] = round(row["old"]["us_median"] / row["new"]["us_median"], 3)
        rows.append(row)
    res = {"tool": "tools/bench_up3.py", "layer": "up_3: conv3x3(up2(x)), 64 -> 64, f16x3, PReLU epilogue", "windows": args.windows, "window_s": args.window_s,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
