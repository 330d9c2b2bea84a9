#!/usr/bin/env python3
"""What the Boundary IoU counts cost on the GPU: arseg_boundary_iou_fwd (csrc/bands.hip) alone, against two arseg_label_bands_fwd calls
(one per plane), the evaluator tail it follows and a stream copy of the bytes it must move, on the same frames.  One process, forms
alternated, --repeats windows of >= --window seconds each, HIP events on the launch stream, median and min-max; the protocol of
tools/bench_bands.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: N = 11 (the non-keyframes of a GOP) at 512x1024 with 12 classes and at 1024x2048 with 19, the blob planes of tests/rle_oracle.py as
int64 labels with a void strip; the prediction is the label plane shifted one pixel to the right.  Radii: (1, 2, 4, 8) and the paper's
2 % of the diagonal, (23,) and (46,).
Forms:
  tail                 arseg_argmax_confusion_grouped_fwd alone (same-size logits, labels and pred): a yardstick
  copy                 arseg_peak_stream_copy over the bytes a call with counts alone must move (8 NHW label bytes and 4 NHW prediction
                       bytes in, 4 NHW workspace bytes out and in): a yardstick
  boundary_R           the whole call at radii R, counts alone
  boundary_planes_R    the same with both band planes
  boundary_1           the whole call at radius 1: the smallest halo and one radius' ballots -- the difference to boundary_R is what the
                       halo of R rows and the further radii cost
  two_bands_R          two arseg_label_bands_fwd calls with hist, on the labels and on the prediction cast to int64 (where R <= 32)
  two_rows_R           the first launch of each of the two (band_out and hist NULL): what the row launch costs on two int64 planes (the
                       row launch of boundary_iou reads an int64 and an int32 plane instead); at R = 46 the radius is 32, which only
                       changes a cap.  The column launch of boundary_R is reported as the difference.
Before anything is timed, per shape and radii and for both border values: frame 0's counts must equal evaluation.boundary_iou_numpy's,
and the counts of all frames, summed over the bands, the row sums, column sums and diagonal of the plain confusion matrix, bit for bit.
No time is fixed in advance; the ratios are reported, not gated.  One JSON line on stdout, the same written to --out (default
profiles/boundary_iou.json)."""
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


def shape_cost(N, H, W, n_cls, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    all_radii = ((1, 2, 4, 8), (ops.boundary_radius(H, W),))
    planes = rle_oracle.blob_planes(5, N, H, W, n_cls=n_cls).astype(np.int64)
    planes[:, :3, :] = 255                                                     # a void strip, as an annotation's border has
    shifted = np.where(planes == 255, 0, np.roll(planes, 1, axis=2)).astype(np.int32)
    label, pred = torch.from_numpy(planes).to(dev), torch.from_numpy(shifted).to(dev)
    pred64 = pred.long()
    groups = torch.arange(1, N + 1, dtype=torch.int32, device=dev)
    G = N + 1
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, H, W)).astype(np.float32)).to(dev)
    tail_pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    tail_hist = torch.zeros((G, n_cls, n_cls), dtype=torch.int64, device=dev)
    lband, pband = (torch.empty((N, H, W), dtype=torch.uint8, device=dev) for _ in range(2))
    ws_bytes = lib.arseg_boundary_iou_workspace_bytes(N, H, W)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    bands_ws_bytes = lib.arseg_label_bands_workspace_bytes(N, H, W)
    moved = (8 + 4 + 4 + 4) * N * H * W
    src, dst = (torch.empty((moved // 2 // 16 * 16,), dtype=torch.uint8, device=dev) for _ in range(2))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    keys = all_radii + ((1,),)
    counts = {(r, b): torch.zeros((G, 3, len(r) + 1, n_cls), dtype=torch.int64, device=dev) for r in keys for b in (0, 1)}
    hists = {r: torch.zeros((G, len(r) + 1, n_cls, n_cls), dtype=torch.int64, device=dev) for r in all_radii if r[-1] <= 32}

    def tail():
        _lib.check(lib.arseg_argmax_confusion_grouped_fwd(P(logits), P(label), P(groups), P(tail_pred), P(tail_hist), N, G, n_cls, H, W, H, W, 255, 1, st),
                   "tail")

    def copy():
        _lib.check(lib.arseg_peak_stream_copy(P(src), P(dst), src.numel(), st), "copy")

    def boundary(radii, border=1, with_planes=False):
        arr = (ctypes.c_int * len(radii))(*radii)

        def run():
            _lib.check(lib.arseg_boundary_iou_fwd(P(label), P(pred), P(groups), arr, len(radii), border, P(lband) if with_planes else null, W, H * W,
                                                  P(pband) if with_planes else null, W, H * W, P(counts[(radii, border)]), N, G, n_cls, H, W, 255,
                                                  P(ws), ws_bytes, st), "boundary_iou")
        return run

    def two_bands(radii, tally=True):
        arr = (ctypes.c_int * len(radii))(*radii)

        def run():
            for plane in (label, pred64):
                _lib.check(lib.arseg_label_bands_fwd(P(plane), P(pred) if tally else null, P(groups), arr, len(radii), null, W, H * W,
                                                     P(hists[radii]) if tally else null, N, G, n_cls, H, W, 255, P(ws), bands_ws_bytes, st), "bands")
        return run

    # ---- correctness first: bit for bit against the host form and the plain confusion matrix
    keep = (label != 255) & (pred >= 0) & (pred < n_cls)
    grp_of = groups.long()[:, None, None].expand(N, H, W)
    plain = torch.bincount(((grp_of * n_cls + label) * n_cls + pred.long())[keep], minlength=G * n_cls * n_cls).view(G, n_cls, n_cls)
    shares = {}
    for radii in all_radii:
        for border in (0, 1):
            c = counts[(radii, border)]
            boundary(radii, border)()
            torch.cuda.synchronize()
            if not np.array_equal(c[1].cpu().numpy(), evaluation.boundary_iou_numpy(planes[0], shifted[0], radii, n_cls, border=bool(border))):
                raise SystemExit(f"{name}, {radii}, border {border}: frame 0's counts differ from boundary_iou_numpy's")
            total = c.sum(2)
            if not (torch.equal(total[:, 0], plain.sum(2)) and torch.equal(total[:, 1], plain.sum(1)) and
                    torch.equal(total[:, 2], torch.diagonal(plain, dim1=1, dim2=2))):
                raise SystemExit(f"{name}, {radii}, border {border}: the bands do not sum to the plain confusion matrix")
        per_band = counts[(radii, 1)][:, 0].sum((0, 2)).cpu().numpy().astype(np.float64)
        shares[str(radii)] = (per_band / per_band.sum()).tolist()

    forms = {"tail": tail, "copy": copy, "boundary_1": boundary((1,))}
    for radii in all_radii:
        key = "_".join(str(r) for r in radii)
        forms[f"boundary_{key}"] = boundary(radii)
        forms[f"boundary_planes_{key}"] = boundary(radii, with_planes=True)
        if radii[-1] <= 32:
            forms[f"two_bands_{key}"] = two_bands(radii)
            forms[f"two_rows_{key}"] = two_bands(radii, tally=False)
        else:
            hists[(32,)] = None
            forms[f"two_rows_{key}"] = two_bands((32,), tally=False)
    res = alternate(forms, repeats, window)
    t, c, one = res["tail"]["us_median"], res["copy"]["us_median"], res["boundary_1"]["us_median"]
    verdict = {"tail_alone_us": t, "copy_us": c, "copy_bytes_moved": int(2 * src.numel()), "copy_tb_per_s": 2 * src.numel() / c / 1e6, "radius_1_us": one}
    for radii in all_radii:
        key = "_".join(str(r) for r in radii)
        whole, rows = res[f"boundary_{key}"]["us_median"], res[f"two_rows_{key}"]["us_median"]
        v = {"call_us": whole, "with_planes_us": res[f"boundary_planes_{key}"]["us_median"], "rows_us_two_int64_planes": rows, "columns_us": whole - rows,
             "call_over_tail": whole / t, "call_over_copy": whole / c, "share_beyond_radius_1": (whole - one) / whole}
        if f"two_bands_{key}" in res:
            two = res[f"two_bands_{key}"]["us_median"]
            v.update({"two_label_bands_us": two, "call_over_two_label_bands": whole / two, "no_more_than_two_label_bands": bool(whole <= two)})
        verdict[key] = v
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()), file=sys.stderr)
    return {"planes": [N, H, W], "n_cls": n_cls, "radii": [list(r) for r in all_radii], "workspace_bytes": int(ws_bytes),
            "pixel_share_per_label_band": shares, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_iou.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundary_iou.py measures on the GPU; none found")
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
