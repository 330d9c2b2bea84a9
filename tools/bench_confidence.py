#!/usr/bin/env python3
"""What the online quality signal costs: the confidence launch (csrc/confidence.hip) against the evaluator tail it shares its label rule
with, against the egress launch, and against the same result composed in torch, on the same logits.  One process, forms alternated,
--repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of tools/bench_egress.py.
The kernel forms are bare ABI calls on preallocated buffers.

Shapes: the four of tools/bench_egress.py -- CamVid PSPNet's tail (12 classes, 512x1024 logits at label size: the same-size route) and
BiSeNet's (19 classes, 128x256 head logits -> 1024x2048: the x8 run route), each for the 11 non-keyframes of a GOP and for one keyframe.
Forms:
  tail_pred          arseg_argmax_confusion_fwd, pred int32 only: the yardstick
  labels8            arseg_segment_egress_fwd, the uint8 label plane only
  conf_labels_stats  arseg_segment_confidence_fwd: conf8 + labels8 + stats in one launch
  stats_only         arseg_segment_confidence_fwd: stats alone (no plane is written)
  torch              interpolate -> softmax -> max -> codes, lt + sum, bincount: what a caller would build from the head logits today
                     (fp32, allocating; writes and re-reads the full-resolution probabilities)
Before anything is timed, on frame 0 of each shape: the kernel's codes are held to the comparison rule of tests/confidence_oracle.py
against a float64 torch composition on the GPU (|q - q_ref| <= 1 everywhere, equal outside 0.025 codes of a rounding boundary, at most
10 % boundary pixels, at least 64 distinct codes), labels8 must equal the tail's pred, the statistics must equal the planes', and the fp32
torch composition must be within one code of the kernel.  One JSON line on stdout, the same written to --out (default
profiles/confidence.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from arseg_amd import _lib


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


def torch_form(logits, H, W, align, low, dtype=torch.float32):
    """(codes uint8 [N,H,W], labels int64 [N,H,W], stats int64 [N,34]) composed from torch ops."""
    N, n_cls = logits.shape[:2]
    x = logits.to(dtype)
    if tuple(x.shape[-2:]) != (H, W):
        x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align))
    p1, lab = torch.softmax(x, dim=1).max(dim=1)
    q = torch.floor(255.0 * p1 + 0.5).to(torch.uint8)
    stats = torch.zeros((N, _lib.CONF_NSTATS), dtype=torch.int64, device=logits.device)
    stats[:, 0] = q.sum(dim=(1, 2), dtype=torch.int64)
    stats[:, 1] = q.lt(low).sum(dim=(1, 2))
    for n in range(N):
        stats[n, 2:2 + n_cls] = torch.bincount(lab[n].reshape(-1), minlength=n_cls)
    return q, lab, stats, p1


def shape_cost(N, n_cls, h, w, H, W, align, repeats, window, dev):
    lib = _lib.load()
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(np.clip(g.standard_normal((N, n_cls, h, w)) * 3.0, -8.0, 8.0).astype(np.float32)).to(dev)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    lab, conf = torch.empty((N, H, W), dtype=torch.uint8, device=dev), torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    stats = torch.zeros((N, _lib.CONF_NSTATS), dtype=torch.int64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    al, low = 1 if align else 0, 128

    def tail():
        _lib.check(lib.arseg_argmax_confusion_fwd(P(logits), null, P(pred), null, N, n_cls, h, w, H, W, 255, al, st), "tail")

    def labels8():
        _lib.check(lib.arseg_segment_egress_fwd(P(logits), N, n_cls, h, w, H, W, al, None, P(lab), W, H * W, 0, null, null, null, 0, 0, 0, 0, 0, 0,
                                                null, null, null, 0, 0, 0, 0, 0, 0, None, None, st), "egress")

    def conf_form(planes):
        def run():
            c, l = (P(conf), P(lab)) if planes else (null, null)
            _lib.check(lib.arseg_segment_confidence_fwd(P(logits), N, n_cls, h, w, H, W, al, _lib.CONF_TOP1, low, None, c, W, H * W, l, W, H * W,
                                                        P(stats), st), "confidence")
        return run

    forms = {"tail_pred": tail, "labels8": labels8, "conf_labels_stats": conf_form(True), "stats_only": conf_form(False),
             "torch": lambda: torch_form(logits, H, W, align, low)}

    # ---- correctness first
    tail()
    stats.zero_()
    forms["conf_labels_stats"]()
    torch.cuda.synchronize()
    name = f"{N}x{n_cls}x{h}x{w} -> {H}x{W}"
    if int((lab.int() != pred).sum()) != 0:
        raise SystemExit(f"{name}: labels8 differs from the tail's pred")
    want = torch.zeros_like(stats)
    want[:, 0] = conf.sum(dim=(1, 2), dtype=torch.int64)
    want[:, 1] = conf.lt(low).sum(dim=(1, 2))
    for n in range(N):
        want[n, 2:2 + n_cls] = torch.bincount(pred[n].reshape(-1).long(), minlength=n_cls)
    if not torch.equal(stats, want):
        raise SystemExit(f"{name}: the statistics differ from the planes'")
    keep = stats.clone()
    stats.zero_()
    forms["stats_only"]()
    torch.cuda.synchronize()
    if not torch.equal(stats, keep):
        raise SystemExit(f"{name}: stats alone differ from stats with planes")
    p1_64 = torch_form(logits[0:1], H, W, align, low, torch.float64)[3]
    x = 255.0 * p1_64
    q_ref = torch.floor(x + 0.5).to(torch.int64)
    boundary = (x - (torch.floor(x) + 0.5)).abs() <= 0.025
    diff = (conf[0:1].long() - q_ref).abs()
    share, distinct = float(boundary.double().mean()), int(len(torch.unique(q_ref)))
    q32 = torch_form(logits[0:1], H, W, align, low)[0]
    torch_off = int((q32.long() - conf[0:1].long()).abs().max())
    check = {"max_abs_diff": int(diff.max()), "differing_outside_boundary": int((diff[~boundary] != 0).sum()),
             "differing_inside_boundary": int((diff[boundary] != 0).sum()), "boundary_share": share, "distinct_codes": distinct,
             "torch_fp32_max_abs_diff_to_kernel": torch_off, "torch_fp32_differing": int((q32 != conf[0:1]).sum())}
    if check["max_abs_diff"] > 1 or check["differing_outside_boundary"] or share > 0.10 or distinct < 64 or torch_off > 1:
        raise SystemExit(f"{name}: the kernel's codes miss the comparison rule: {check}")
    del p1_64, x, q_ref, boundary, diff, q32

    res = alternate(forms, repeats, window)
    lo, px = logits.numel() * 4, N * H * W
    needed = {"tail_pred": lo + 4 * px, "labels8": lo + px, "conf_labels_stats": lo + 2 * px, "stats_only": lo}
    base = res["tail_pred"]
    spread = (base["us_max"] - base["us_min"]) / base["us_median"]
    for k, r in res.items():
        r["time_over_tail"] = r["us_median"] / base["us_median"]
        if k in needed:
            r["bytes_needed"] = needed[k]
            r["GBps"] = needed[k] / (r["us_median"] * 1e-6) / 1e9
    print(f"{name}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; tail spread {100 * spread:.1f}%", file=sys.stderr)
    return {"logits": [N, n_cls, h, w], "labels": [H, W], "align_corners": bool(align), "kind": "top1", "low": low, "tail_spread": spread,
            "check_frame0": check, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "confidence.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_confidence.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for N in (11, 1):
        res["shapes"].append(shape_cost(N, 12, 512, 1024, 512, 1024, True, a.repeats, a.window, dev))
        res["shapes"].append(shape_cost(N, 19, 128, 256, 1024, 2048, False, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
