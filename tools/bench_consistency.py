#!/usr/bin/env python3
"""What the temporal-consistency signal costs: the consistency launch (csrc/consistency.hip) against the egress launch that writes the label
plane alone, and against the same result composed in torch, on the same logits, reference plane and motion field.  One process, forms
alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of
tools/bench_confidence.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: the four of tools/bench_egress.py -- CamVid PSPNet's tail (12 classes, 512x1024 logits at label size: the same-size route) and
BiSeNet's (19 classes, 128x256 head logits -> 1024x2048: the x8 run route), each for the 11 non-keyframes of a GOP and for one keyframe-sized
batch.  The reference plane is shared by the frames (the keyframe's); the field is block constant (16 x 16) with a few pixels of motion.
Forms:
  labels8              arseg_segment_egress_fwd, the uint8 label plane only: the yardstick
  labels_change_stats  arseg_segment_consistency_fwd: labels8 + change8 + stats in one launch
  stats_only           arseg_segment_consistency_fwd: stats alone (no plane is written)
  torch                interpolate -> argmax, the target index from mv_q, a gather, two compares, three bincounts: what a caller would
                       build from the head logits today (allocating; writes and re-reads the full-resolution logits)
Before anything is timed, for each shape: labels8, change8 and the statistics of the fused launch must equal the torch composition fed
the tail's own pred bit for bit, and stats alone must equal stats with planes.  One JSON line on stdout, the same written to --out (default
profiles/consistency.json)."""
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


def round_half_even_div4(v):
    b, r = v >> 2, v & 3
    return torch.where(r < 2, b, torch.where(r > 2, b + 1, b + (b & 1)))


def torch_form(logits, ref, mv, H, W, align, lab=None):
    """(change uint8 [N,H,W], labels int64 [N,H,W], stats int64 [N,TC_NSTATS]) composed from torch ops; ``lab``: labels to use instead of
    the composition's own interpolate -> argmax (the correctness check feeds the tail's pred)."""
    N, n_cls = logits.shape[:2]
    if lab is None:
        x = logits
        if tuple(x.shape[-2:]) != (H, W):
            x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align))
        lab = x.argmax(dim=1)
    ys, xs = torch.meshgrid(torch.arange(H, device=logits.device), torch.arange(W, device=logits.device), indexing="ij")
    tx, ty = xs + round_half_even_div4(mv[..., 0].long()), ys + round_half_even_div4(mv[..., 1].long())
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    r = ref.reshape(-1)[(ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)).reshape(N, -1)].reshape(N, H, W).long()
    compared = inside & (r < n_cls)
    agree = compared & (r == lab)
    change = torch.where(compared, torch.where(agree, 0, 255), 128).to(torch.uint8)
    stats = torch.zeros((N, _lib.TC_NSTATS), dtype=torch.int64, device=logits.device)
    stats[:, 0], stats[:, 1] = compared.sum(dim=(1, 2)), (~inside).sum(dim=(1, 2))
    stats[:, 2] = H * W - stats[:, 0] - stats[:, 1]
    for n in range(N):
        stats[n, 3:3 + n_cls] = torch.bincount(lab[n][compared[n]], minlength=n_cls)
        stats[n, 35:35 + n_cls] = torch.bincount(r[n][compared[n]], minlength=n_cls)
        stats[n, 67:67 + n_cls] = torch.bincount(lab[n][agree[n]], minlength=n_cls)
    return change, lab, stats


def shape_cost(N, n_cls, h, w, H, W, align, repeats, window, dev):
    lib = _lib.load()
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(np.clip(g.standard_normal((N, n_cls, h, w)) * 3.0, -8.0, 8.0).astype(np.float32)).to(dev)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    lab, chg = torch.empty((N, H, W), dtype=torch.uint8, device=dev), torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    stats = torch.zeros((N, _lib.TC_NSTATS), dtype=torch.int64, device=dev)
    blocks = g.integers(-24, 25, (N, H // 16, W // 16, 2)).astype(np.int16)
    mv = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(blocks, 16, axis=1), 16, axis=2))).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    al = 1 if align else 0

    def tail():
        _lib.check(lib.arseg_argmax_confusion_fwd(P(logits), null, P(pred), null, N, n_cls, h, w, H, W, 255, al, st), "tail")

    def labels8():
        _lib.check(lib.arseg_segment_egress_fwd(P(logits), N, n_cls, h, w, H, W, al, None, P(lab), W, H * W, 0, null, null, null, 0, 0, 0, 0, 0, 0,
                                                null, null, null, 0, 0, 0, 0, 0, 0, None, None, st), "egress")

    tail()
    ref = torch.roll(pred[0], shifts=(2, -3), dims=(0, 1)).to(torch.uint8).contiguous()          # the keyframe's plane: frame 0's labels, displaced
    ref[H // 4:H // 4 + H // 16, W // 4:W // 4 + W // 8] = 255

    def tc_form(planes):
        def run():
            l, c = (P(lab), P(chg)) if planes else (null, null)
            _lib.check(lib.arseg_segment_consistency_fwd(P(logits), N, n_cls, h, w, H, W, al, P(ref), W, 0, P(mv), None, l, W, H * W, c, W, H * W,
                                                         P(stats), st), "consistency")
        return run

    forms = {"labels8": labels8, "labels_change_stats": tc_form(True), "stats_only": tc_form(False),
             "torch": lambda: torch_form(logits, ref, mv, H, W, align)}

    # ---- correctness first: bit for bit against the composition fed the tail's pred
    stats.zero_()
    forms["labels_change_stats"]()
    torch.cuda.synchronize()
    name = f"{N}x{n_cls}x{h}x{w} -> {H}x{W}"
    if int((lab.int() != pred).sum()) != 0:
        raise SystemExit(f"{name}: labels8 differs from the tail's pred")
    want_c, _, want_s = torch_form(logits, ref, mv, H, W, align, lab=pred.long())
    if not torch.equal(chg, want_c):
        raise SystemExit(f"{name}: change8 differs from the composition in {int((chg != want_c).sum())} pixels")
    if not torch.equal(stats, want_s):
        raise SystemExit(f"{name}: the statistics differ from the composition's")
    keep = stats.clone()
    stats.zero_()
    forms["stats_only"]()
    torch.cuda.synchronize()
    if not torch.equal(stats, keep):
        raise SystemExit(f"{name}: stats alone differ from stats with planes")
    own = torch_form(logits[0:1], ref, mv[0:1], H, W, align)[1]
    check = {"compared": keep[:, 0].tolist(), "outside": keep[:, 1].tolist(), "void": keep[:, 2].tolist(),
             "agree": keep[:, 67:].sum(dim=1).tolist(), "torch_argmax_differing_from_tail_frame0": int((own != pred[0:1].long()).sum())}
    del want_c, want_s, own

    res = alternate(forms, repeats, window)
    lo, px = logits.numel() * 4, N * H * W
    needed = {"labels8": lo + px, "labels_change_stats": lo + 4 * px + px + 2 * px, "stats_only": lo + 4 * px + px}          # + mv_q and the gathered reference bytes
    base = res["labels8"]
    spread = (base["us_max"] - base["us_min"]) / base["us_median"]
    for k, r in res.items():
        r["time_over_labels8"] = r["us_median"] / base["us_median"]
        if k in needed:
            r["bytes_needed"] = needed[k]
            r["GBps"] = needed[k] / (r["us_median"] * 1e-6) / 1e9
    print(f"{name}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; labels8 spread {100 * spread:.1f}%", file=sys.stderr)
    return {"logits": [N, n_cls, h, w], "labels": [H, W], "align_corners": bool(align), "labels8_spread": spread, "check": check, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "consistency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency.py measures on the GPU; none found")
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
