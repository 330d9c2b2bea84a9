#!/usr/bin/env python3
"""What the contour F-measure counts cost on the GPU: arseg_contour_f_fwd (csrc/bands.hip) alone, against arseg_boundary_iou_fwd at the same
radii, the evaluator tail it follows and a stream copy of the bytes it must move, on the same frames.  One process, forms alternated,
--repeats windows of >= --window seconds each, HIP events on the launch stream, median and min-max; the protocol of
tools/bench_boundary_iou.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: N = 11 (the non-keyframes of a GOP) at 512x1024 with 12 classes and at 1024x2048 with 19, the blob planes of tests/rle_oracle.py as
int64 labels with a void strip.  Two predictions: the label plane shifted one pixel to the right (nearly every contour pixel matched in
the first ring or two) and shifted eight pixels (long searches).  Radii: DAVIS's 0.8 % of the diagonal, (10,) and (19,), and (1, 2, 4, 8).
Forms:
  tail                 arseg_argmax_confusion_grouped_fwd alone (same-size logits, labels and pred): a yardstick
  copy                 arseg_peak_stream_copy over the bytes a call with counts alone must move (8 NHW label bytes and 4 NHW prediction
                       bytes in, 2 NHW workspace bytes out and in): a yardstick
  boundary_R           arseg_boundary_iou_fwd at radii R, counts alone, on the one-pixel shift: a yardstick
  contour_R_sS         the whole call at radii R on the prediction shifted S pixels, counts alone
  contour_planes_R_sS  the same with both match planes
  contour_0_s1         the whole call at radius 0: no halo, one ring -- the marks, the staging, the lists and the tally without a search
Before anything is timed, per shape, prediction and radii: frame 0's counts must equal evaluation.contour_f_numpy's bit for bit.  The share
of contour pixels and the share of them left unmatched are recorded.  No time is fixed in advance; the ratios are reported, not gated.
One JSON line on stdout, the same written to --out (default profiles/contour_f.json)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import rle_oracle
from arseg_amd import _lib, evaluation, ops
from bench_regions import alternate

SHIFTS = (1, 8)


def shape_cost(N, H, W, n_cls, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    all_radii = ((ops.contour_radius(H, W),), (1, 2, 4, 8))
    planes = rle_oracle.blob_planes(5, N, H, W, n_cls=n_cls).astype(np.int64)
    planes[:, :3, :] = 255                                                     # a void strip, as an annotation's border has
    shifted = {s: np.where(planes == 255, 0, np.roll(planes, s, axis=2)).astype(np.int32) for s in SHIFTS}
    label = torch.from_numpy(planes).to(dev)
    preds = {s: torch.from_numpy(p).to(dev) for s, p in shifted.items()}
    groups = torch.arange(1, N + 1, dtype=torch.int32, device=dev)
    G = N + 1
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, H, W)).astype(np.float32)).to(dev)
    tail_pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    tail_hist = torch.zeros((G, n_cls, n_cls), dtype=torch.int64, device=dev)
    lplane, pplane = (torch.empty((N, H, W), dtype=torch.uint8, device=dev) for _ in range(2))
    ws_bytes = lib.arseg_contour_f_workspace_bytes(N, H, W)
    bi_bytes = lib.arseg_boundary_iou_workspace_bytes(N, H, W)
    ws = torch.empty((max(ws_bytes, bi_bytes),), dtype=torch.uint8, device=dev)
    moved = (8 + 4 + 2 + 2) * N * H * W
    src, dst = (torch.empty((moved // 2 // 16 * 16,), dtype=torch.uint8, device=dev) for _ in range(2))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    counts = {(r, s): torch.zeros((G, 2, len(r) + 1, n_cls), dtype=torch.int64, device=dev) for r in all_radii + ((0,),) for s in SHIFTS}
    bi_counts = {r: torch.zeros((G, 3, len(r) + 1, n_cls), dtype=torch.int64, device=dev) for r in all_radii}

    def tail():
        _lib.check(lib.arseg_argmax_confusion_grouped_fwd(P(logits), P(label), P(groups), P(tail_pred), P(tail_hist), N, G, n_cls, H, W, H, W, 255, 1, st),
                   "tail")

    def copy():
        _lib.check(lib.arseg_peak_stream_copy(P(src), P(dst), src.numel(), st), "copy")

    def boundary(radii):
        arr = (ctypes.c_int * len(radii))(*radii)

        def run():
            _lib.check(lib.arseg_boundary_iou_fwd(P(label), P(preds[1]), P(groups), arr, len(radii), 1, null, W, H * W, null, W, H * W, P(bi_counts[radii]),
                                                  N, G, n_cls, H, W, 255, P(ws), bi_bytes, st), "boundary_iou")
        return run

    def contour(radii, shift, with_planes=False):
        arr = (ctypes.c_int * len(radii))(*radii)

        def run():
            _lib.check(lib.arseg_contour_f_fwd(P(label), P(preds[shift]), P(groups), arr, len(radii), P(lplane) if with_planes else null, W, H * W,
                                               P(pplane) if with_planes else null, W, H * W, P(counts[(radii, shift)]), N, G, n_cls, H, W, 255,
                                               P(ws), ws_bytes, st), "contour_f")
        return run

    # ---- correctness first: frame 0 bit for bit against the host form; the shares of contour and of unmatched pixels
    shares = {}
    for shift in SHIFTS:
        for radii in all_radii:
            c = counts[(radii, shift)]
            contour(radii, shift, with_planes=True)()
            torch.cuda.synchronize()
            if not np.array_equal(c[1].cpu().numpy(), evaluation.contour_f_numpy(planes[0], shifted[shift][0], radii, n_cls)):
                raise SystemExit(f"{name}, shift {shift}, {radii}: frame 0's counts differ from contour_f_numpy's")
            on = [int((p != 255).sum()) for p in (lplane, pplane)]
            off = [int((p == len(radii)).sum()) for p in (lplane, pplane)]
            per_band = c.sum((0, 3)).cpu().numpy().astype(np.float64)
            shares[f"s{shift}_" + "_".join(str(r) for r in radii)] = {
                "contour_pixel_share_label_pred": [v / (N * H * W) for v in on], "unmatched_share_label_pred": [u / max(v, 1) for u, v in zip(off, on)],
                "counting_share_per_band_label": (per_band[0] / max(per_band[0].sum(), 1)).tolist(),
                "counting_share_per_band_pred": (per_band[1] / max(per_band[1].sum(), 1)).tolist()}

    forms = {"tail": tail, "copy": copy, "contour_0_s1": contour((0,), 1)}
    for radii in all_radii:
        key = "_".join(str(r) for r in radii)
        forms[f"boundary_{key}"] = boundary(radii)
        for shift in SHIFTS:
            forms[f"contour_{key}_s{shift}"] = contour(radii, shift)
            forms[f"contour_planes_{key}_s{shift}"] = contour(radii, shift, with_planes=True)
    res = alternate(forms, repeats, window)
    t, c, zero = res["tail"]["us_median"], res["copy"]["us_median"], res["contour_0_s1"]["us_median"]
    verdict = {"tail_alone_us": t, "copy_us": c, "copy_bytes_moved": int(2 * src.numel()), "copy_tb_per_s": 2 * src.numel() / c / 1e6, "radius_0_us": zero}
    for radii in all_radii:
        key = "_".join(str(r) for r in radii)
        b = res[f"boundary_{key}"]["us_median"]
        for shift in SHIFTS:
            whole = res[f"contour_{key}_s{shift}"]["us_median"]
            verdict[f"{key}_s{shift}"] = {"call_us": whole, "with_planes_us": res[f"contour_planes_{key}_s{shift}"]["us_median"], "boundary_iou_us": b,
                                          "call_over_boundary_iou": whole / b, "call_over_tail": whole / t, "call_over_copy": whole / c,
                                          "share_beyond_radius_0": (whole - zero) / whole}
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()), file=sys.stderr)
    return {"planes": [N, H, W], "n_cls": n_cls, "radii": [list(r) for r in all_radii], "shifts": list(SHIFTS), "workspace_bytes": int(ws_bytes),
            "shares": shares, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_f.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contour_f.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for H, W, n_cls in ((512, 1024, 12), (1024, 2048, 19)):
        res["shapes"].append(shape_cost(11, H, W, n_cls, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
