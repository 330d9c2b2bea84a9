#!/usr/bin/env python3
"""What the boundary bands cost on the GPU: arseg_label_bands_fwd (csrc/bands.hip) alone, against the evaluator tail it is added to and
against a stream copy of the bytes it must move, on the same frames.  One process, forms alternated, --repeats windows of >= --window
seconds each, HIP events on the launch stream, median and min-max; the protocol of tools/bench_fill.py.  The kernel forms are bare ABI
calls on preallocated buffers.

Shapes: N = 11 (the non-keyframes of a GOP) at 512x1024 with 12 classes and at 1024x2048 with 19, the blob planes of tests/rle_oracle.py as
int64 labels; the prediction is the label plane shifted one pixel to the right, so it differs from the labels in a thin band at the
boundaries.  Radii: (1, 2, 4, 8) and (32,).
Forms:
  tail                 arseg_argmax_confusion_grouped_fwd alone (same-size logits, labels and pred): a yardstick, the tail the call follows
  copy                 arseg_peak_stream_copy over the bytes a whole call must move (8 NHW label bytes and 4 NHW prediction bytes in, 2 NHW
                       workspace bytes out and in, NHW band bytes out): a yardstick
  bands_R              the whole call at radii R: hist and band_out
  bands_hist_R         the same without band_out
  rows_R               the first launch alone (band_out and hist NULL); the second launch is the difference to bands_R
Before anything is timed, per shape and radii: frame 0's band plane must equal evaluation.label_bands_numpy's and the histogram, summed
over the bands, the tail's, bit for bit.  No time is fixed in advance; the ratios are reported, not gated.  One JSON line on stdout, the same
written to --out (default profiles/bands.json)."""
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

RADII = ((1, 2, 4, 8), (32,))


def shape_cost(N, H, W, n_cls, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    planes = rle_oracle.blob_planes(5, N, H, W, n_cls=n_cls).astype(np.int64)
    planes[:, :3, :] = 255                                                     # a void strip, as an annotation's border has
    label = torch.from_numpy(planes).to(dev)
    pred = torch.from_numpy(np.where(planes == 255, 0, np.roll(planes, 1, axis=2)).astype(np.int32)).to(dev)
    groups = torch.arange(1, N + 1, dtype=torch.int32, device=dev)
    G = N + 1
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, H, W)).astype(np.float32)).to(dev)
    tail_pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    tail_hist = torch.zeros((G, n_cls, n_cls), dtype=torch.int64, device=dev)
    band = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    ws_bytes = lib.arseg_label_bands_workspace_bytes(N, H, W)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    moved = (8 + 4 + 2 + 2 + 1) * N * H * W
    src, dst = (torch.empty((moved // 2 // 16 * 16,), dtype=torch.uint8, device=dev) for _ in range(2))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    hists = {r: torch.zeros((G, len(r) + 1, n_cls, n_cls), dtype=torch.int64, device=dev) for r in RADII}

    def tail():
        _lib.check(lib.arseg_argmax_confusion_grouped_fwd(P(logits), P(label), P(groups), P(tail_pred), P(tail_hist), N, G, n_cls, H, W, H, W, 255, 1, st),
                   "tail")

    def copy():
        _lib.check(lib.arseg_peak_stream_copy(P(src), P(dst), src.numel(), st), "copy")

    def bands(radii, plane=True, tally=True):
        arr = (ctypes.c_int * len(radii))(*radii)

        def run():
            _lib.check(lib.arseg_label_bands_fwd(P(label), P(pred) if tally else null, P(groups), arr, len(radii), P(band) if plane else null, W, H * W,
                                                 P(hists[radii]) if tally else null, N, G, n_cls, H, W, 255, P(ws), ws_bytes, st), "bands")
        return run

    # ---- correctness first: bit for bit against the host form and the plain confusion matrix
    keep = (label != 255) & (pred >= 0) & (pred < n_cls)
    grp_of = groups.long()[:, None, None].expand(N, H, W)
    plain = torch.bincount(((grp_of * n_cls + label) * n_cls + pred.long())[keep], minlength=G * n_cls * n_cls).view(G, n_cls, n_cls)
    shares = {}
    for radii in RADII:
        bands(radii)()
        torch.cuda.synchronize()
        if not np.array_equal(band[0].cpu().numpy(), evaluation.label_bands_numpy(planes[0], radii, n_cls)):
            raise SystemExit(f"{name}, {radii}: frame 0's bands differ from label_bands_numpy's")
        if not torch.equal(hists[radii].sum(1), plain):
            raise SystemExit(f"{name}, {radii}: the bands do not sum to the plain confusion matrix")
        per_band = hists[radii].sum((0, 2, 3)).cpu().numpy().astype(np.float64)
        shares[str(radii)] = (per_band / per_band.sum()).tolist()

    forms = {"tail": tail, "copy": copy}
    for radii in RADII:
        key = "_".join(str(r) for r in radii)
        forms[f"bands_{key}"] = bands(radii)
        forms[f"bands_hist_{key}"] = bands(radii, plane=False)
        forms[f"rows_{key}"] = bands(radii, plane=False, tally=False)
    res = alternate(forms, repeats, window)
    t, c = res["tail"]["us_median"], res["copy"]["us_median"]
    verdict = {"tail_alone_us": t, "copy_us": c, "copy_bytes_moved": int(2 * src.numel()), "copy_tb_per_s": 2 * src.numel() / c / 1e6}
    for radii in RADII:
        key = "_".join(str(r) for r in radii)
        whole, rows = res[f"bands_{key}"]["us_median"], res[f"rows_{key}"]["us_median"]
        verdict[key] = {"call_us": whole, "rows_us": rows, "columns_us": whole - rows, "without_band_out_us": res[f"bands_hist_{key}"]["us_median"],
                        "call_over_tail": whole / t, "call_over_copy": whole / c, "dominant": "columns" if whole - rows > rows else "rows"}
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()), file=sys.stderr)
    return {"planes": [N, H, W], "n_cls": n_cls, "workspace_bytes": int(ws_bytes), "pixel_share_per_band": shares, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bands.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bands.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "radii": [list(r) for r in RADII], "shapes": []}
    for H, W, n_cls in ((512, 1024, 12), (1024, 2048, 19)):
        res["shapes"].append(shape_cost(11, H, W, n_cls, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
