#!/usr/bin/env python3
"""What the output half costs: the egress launch (csrc/egress.hip) against the evaluator tail it shares its label rule with, on the same
logits.  One process, forms alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream), median and
min-max; the protocol of tools/bench_ingest.py.  Every form is the bare ABI call on preallocated buffers, so the host side is the same.

Shapes: CamVid PSPNet's tail (12 classes, 512x1024 logits at label size: the same-size route) and BiSeNet's (19 classes, 128x256 head
logits -> 1024x2048: the x8 run route), each for the 11 non-keyframes of a GOP and for one keyframe.  Forms:
  tail_pred          arseg_argmax_confusion_fwd, pred int32 only: the yardstick (the labels a caller would build its output from)
  labels8            arseg_segment_egress_fwd, the uint8 label plane only: the same logits read, a quarter of the bytes written
  labels8_nv12       labels + NV12 overlay out of place (source planes read, destination planes written)
  nv12_in_place      labels + NV12 overlay painted into the source planes
Per form: us per launch, the bytes it MUST move (logits + source planes + destination planes + labels), GB/s of those against the 8 TB/s
datasheet rate and against the stream-copy rate measured here (arseg_peak_stream_copy, bench.py's peaks_measured).  `spread` is the
(max - min) / median of tail_pred's windows: labels8 is held to tail_pred's median plus that.  Labels are compared with the tail's before
anything is timed.  One JSON line on stdout, the same written to --out (default profiles/egress.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from arseg_amd import _lib, egress

DATASHEET_GBPS = 8000.0


def window_ms(fn, min_s):
    fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < 1e3 * min_s:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(8):
            fn()
        e.record()
        e.synchronize()
        total += s.elapsed_time(e)
        n += 8
    return total / n


def alternate(forms, repeats, window):
    ms = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            ms[k].append(window_ms(fn, window))
    return {k: {"us_median": 1e3 * statistics.median(v), "us_min": 1e3 * min(v), "us_max": 1e3 * max(v)} for k, v in ms.items()}


def copy_gbps(dev, repeats, window):
    lib, n = _lib.load(), 256 << 20
    a, b = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lambda: _lib.check(lib.arseg_peak_stream_copy(a.data_ptr(), b.data_ptr(), n, st), "stream_copy")
    return 2 * n / (1e-3 * statistics.median(window_ms(fn, window) for _ in range(repeats))) / 1e9


def shape_cost(N, n_cls, h, w, H, W, align, repeats, window, dev, copy_rate):
    lib = _lib.load()
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, h, w)).astype(np.float32)).to(dev)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    lab = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    y = torch.from_numpy(g.integers(0, 256, (N, H, W), dtype=np.uint8)).to(dev)
    uv = torch.from_numpy(g.integers(0, 256, (N, H // 2, W // 2, 2), dtype=np.uint8)).to(dev)
    y2, uv2, y3, uv3 = torch.empty_like(y), torch.empty_like(uv), y.clone(), uv.clone()
    pal = egress.Palette((egress.CAMVID_PALETTE if n_cls == 12 else egress.CITYSCAPES_PALETTE)[:n_cls], 0.5)
    codes = pal.codes(_lib.SRC_NV12, _lib.COLOUR_BT709_LIMITED)
    pal_c, wt_c = (ctypes.c_uint8 * (3 * n_cls))(*codes.reshape(-1).tolist()), (ctypes.c_uint16 * n_cls)(*pal.weights.tolist())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    al = 1 if align else 0

    def tail():
        _lib.check(lib.arseg_argmax_confusion_fwd(P(logits), null, P(pred), null, N, n_cls, h, w, H, W, 255, al, st), "tail")

    def eg(src, dst):
        def run():
            s = (P(src[0]), P(src[1]), null, W, W, 0, H * W, H * W // 2, 0) if src else (null, null, null, 0, 0, 0, 0, 0, 0)
            d = (P(dst[0]), P(dst[1]), null, W, W, 0, H * W, H * W // 2, 0) if dst else (null, null, null, 0, 0, 0, 0, 0, 0)
            _lib.check(lib.arseg_segment_egress_fwd(P(logits), N, n_cls, h, w, H, W, al, None, P(lab), W, H * W, _lib.SRC_NV12, *s, *d,
                                                    pal_c if dst else None, wt_c if dst else None, st), "egress")
        return run

    forms = {"tail_pred": tail, "labels8": eg(None, None), "labels8_nv12": eg((y, uv), (y2, uv2)), "nv12_in_place": eg((y3, uv3), (y3, uv3))}
    tail()
    forms["labels8"]()
    torch.cuda.synchronize()
    if int((lab.int() != pred).sum()) != 0:
        raise SystemExit(f"{N}x{n_cls}x{h}x{w} -> {H}x{W}: labels8 differs from the tail's pred")
    res = alternate(forms, repeats, window)
    lo, px = logits.numel() * 4, N * H * W
    needed = {"tail_pred": lo + 4 * px, "labels8": lo + px, "labels8_nv12": lo + px + 3 * px, "nv12_in_place": lo + px + 3 * px}
    for k, r in res.items():
        r["bytes_needed"] = needed[k]
        r["GBps"] = needed[k] / (r["us_median"] * 1e-6) / 1e9
        r["of_datasheet"] = r["GBps"] / DATASHEET_GBPS
        r["of_stream_copy"] = r["GBps"] / copy_rate
    base = res["tail_pred"]
    spread = (base["us_max"] - base["us_min"]) / base["us_median"]
    res["labels8"]["time_over_tail"] = res["labels8"]["us_median"] / base["us_median"]
    res["labels8"]["within_spread_of_tail"] = bool(res["labels8"]["us_median"] <= base["us_median"] * (1.0 + spread))
    print(f"{N}x{n_cls}x{h}x{w} -> {H}x{W}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; tail spread {100 * spread:.1f}%", file=sys.stderr)
    return {"logits": [N, n_cls, h, w], "labels": [H, W], "align_corners": bool(align), "tail_spread": spread, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "egress.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_egress.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    rate = copy_gbps(dev, a.repeats, a.window)
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "datasheet_GBps": DATASHEET_GBPS,
           "stream_copy_GBps": rate, "shapes": []}
    for N in (11, 1):
        res["shapes"].append(shape_cost(N, 12, 512, 1024, 512, 1024, True, a.repeats, a.window, dev, rate))
        res["shapes"].append(shape_cost(N, 19, 128, 256, 1024, 2048, False, a.repeats, a.window, dev, rate))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
