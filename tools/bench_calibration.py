#!/usr/bin/env python3
"""What the reliability table costs: the calibration launch (csrc/calibration.hip) against the grouped evaluator tail it shares its loads
and label rule with, against the same table composed from the confidence launch's planes, and against the torch composition from the
resized logits, on the same logits and labels.  One process, forms alternated, --repeats windows of >= --window seconds each (HIP events
on the launch stream), median and min-max; the protocol of tools/bench_confidence.py.  The kernel forms are bare ABI calls on
preallocated buffers.

Shapes: the four of tools/bench_confidence.py -- CamVid PSPNet's tail (12 classes, 512x1024 logits at label size: the same-size route)
and BiSeNet's (19 classes, 128x256 head logits -> 1024x2048: the x8 run route), each for the 11 non-keyframes of a GOP (groups 1 .. 11
of 12) and for one keyframe (group 0).
Forms:
  tail_hist              arseg_argmax_confusion_grouped_fwd, hist only (no pred): the yardstick -- the same loads and the same label rule
  calibration            arseg_calibration_fwd on spread logits (clipped normal draws: the codes cover most of 0..255)
  planes_bincount        arseg_segment_confidence_fwd (conf8 + labels8) + the key and two torch.bincount: the composition there was before
  torch                  interpolate -> softmax -> max -> codes -> the same two bincounts (fp32, allocating)
  calibration_saturated  arseg_calibration_fwd on saturated logits: every pixel of every frame in the one bin (class 3, code 255, right)
Before anything is timed, per shape: the kernel's table must equal the planes' table exactly on both sets of logits, its sums over the
codes must be the columns and the diagonal of the tail's hist, and the saturated table must hold all its pixels in one bin.  One JSON line
on stdout, the same written to --out (default profiles/calibration.json)."""
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


def table_of(k, q, label, grp, n_groups, n_cls):
    """k, q integer [N,H,W] (any integer dtype), label int64 [N,H,W], grp int64 [N,1,1] -> int64 [n_groups, n_cls, 256, 2]."""
    k = k.long()
    counting = (label >= 0) & (label < n_cls) & (label != 255)
    key = ((grp * n_cls + k) * 256 + q.long()) * 2
    size = n_groups * n_cls * 512
    return (torch.bincount(key[counting], minlength=size) + torch.bincount(key[counting & (label == k)] + 1, minlength=size)).reshape(n_groups, n_cls, 256, 2)


def shape_cost(N, n_cls, h, w, H, W, align, repeats, window, dev):
    lib = _lib.load()
    g = np.random.Generator(np.random.PCG64(5))
    spread = torch.from_numpy(np.clip(g.standard_normal((N, n_cls, h, w)) * 3.0, -8.0, 8.0).astype(np.float32)).to(dev)
    hot = torch.zeros_like(spread)
    hot[:, 3] = 30.0
    n_groups = 12
    ids = list(range(1, N + 1)) if N > 1 else [0]
    group = torch.tensor(ids, dtype=torch.int32, device=dev)
    grp64 = group.long().reshape(N, 1, 1)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    al = 1 if align else 0
    lab8, conf = torch.empty((N, H, W), dtype=torch.uint8, device=dev), torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    _lib.check(lib.arseg_argmax_confusion_fwd(P(spread), null, P(pred), null, N, n_cls, h, w, H, W, 255, al, st), "tail")
    r = torch.from_numpy(g.random((N, H, W)).astype(np.float32)).to(dev)
    label = torch.where(r < 0.6, pred.long(), torch.from_numpy(g.integers(0, n_cls, (N, H, W))).to(dev))
    label[r > 0.95] = 255
    label_hot = torch.full((N, H, W), 3, dtype=torch.int64, device=dev)
    del r, pred
    cal = torch.zeros((n_groups, n_cls, 256, 2), dtype=torch.int64, device=dev)
    hist = torch.zeros((n_groups, n_cls, n_cls), dtype=torch.int64, device=dev)

    def tail_hist():
        _lib.check(lib.arseg_argmax_confusion_grouped_fwd(P(spread), P(label), P(group), null, P(hist), N, n_groups, n_cls, h, w, H, W, 255, al, st), "tail")

    def calibration(logits, lab):
        def run():
            _lib.check(lib.arseg_calibration_fwd(P(logits), P(lab), P(group), P(cal), N, n_groups, n_cls, h, w, H, W, 255, al, _lib.CONF_TOP1, st),
                       "calibration")
        return run

    def planes(logits, lab):
        _lib.check(lib.arseg_segment_confidence_fwd(P(logits), N, n_cls, h, w, H, W, al, _lib.CONF_TOP1, 128, None, P(conf), W, H * W, P(lab8), W, H * W,
                                                    null, st), "confidence")
        return table_of(lab8, conf, lab, grp64, n_groups, n_cls)

    def torch_form():
        x = spread
        if (h, w) != (H, W):
            x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align))
        p1, k = torch.softmax(x, dim=1).max(dim=1)
        return table_of(k, torch.floor(255.0 * p1 + 0.5), label, grp64, n_groups, n_cls)

    forms = {"tail_hist": tail_hist, "calibration": calibration(spread, label), "planes_bincount": lambda: planes(spread, label), "torch": torch_form,
             "calibration_saturated": calibration(hot, label_hot)}

    # ---- correctness first
    name = f"{N}x{n_cls}x{h}x{w} -> {H}x{W}"
    check = {}
    for what, logits, lab in (("spread", spread, label), ("saturated", hot, label_hot)):
        cal.zero_()
        calibration(logits, lab)()
        want = planes(logits, lab)
        differing = int((cal != want).sum())
        check[what] = {"differing_counters": differing, "bins_in_use": int((cal[..., 0] > 0).sum()), "pixels": int(cal[..., 0].sum())}
        if differing:
            raise SystemExit(f"{name}: the {what} table differs from the planes' table in {differing} counters")
    if check["saturated"]["bins_in_use"] != len(ids) or int(cal[:, 3, 255, 1].sum()) != N * H * W:
        raise SystemExit(f"{name}: the saturated logits do not fall into one bin per group: {check['saturated']}")
    cal.zero_()
    hist.zero_()
    forms["calibration"]()
    tail_hist()
    if not torch.equal(cal[..., 0].sum(dim=2), hist.sum(dim=1)) or not torch.equal(cal[..., 1].sum(dim=2), hist.diagonal(dim1=1, dim2=2)):
        raise SystemExit(f"{name}: the table's sums over the codes are not the tail's columns and diagonal")
    off = torch_form() - cal
    check["torch_fp32_differing_counters"] = int((off != 0).sum())                    # (fp32 rounding at code boundaries: reported, not held)
    del off, want
    torch.cuda.synchronize()

    res = alternate(forms, repeats, window)
    base = res["tail_hist"]
    for k, v in res.items():
        v["time_over_tail"] = v["us_median"] / base["us_median"]
    b, c, e = res["calibration"], res["planes_bincount"], res["calibration_saturated"]
    aims = {"calibration_over_planes_bincount": b["us_median"] / c["us_median"], "calibration_beats_planes_bincount": b["us_median"] < c["us_median"],
            "saturated_over_spread": e["us_median"] / b["us_median"],
            "saturated_within_spread_of_measurements": e["us_median"] <= b["us_median"] + (b["us_max"] - b["us_min"]) + (e["us_max"] - e["us_min"])}
    print(f"{name}: " + ", ".join(f"{k} {v['us_median']:.1f} us ({v['us_min']:.1f}-{v['us_max']:.1f})" for k, v in res.items()), file=sys.stderr)
    return {"logits": [N, n_cls, h, w], "labels": [H, W], "align_corners": bool(align), "kind": "top1", "groups": ids, "check": check, "aims": aims,
            "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "calibration.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibration.py measures on the GPU; none found")
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
