#!/usr/bin/env python3
"""What the outlines of the masks' regions cost on the GPU, and what the host path they replace costs: arseg_rle_contours_fwd
(csrc/contours.hip) behind the run code and its regions, against pulling the run code to the host and tracing there.  One process, forms
alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream for the GPU forms, wall time for the host
form), median and min-max; the protocol of tools/bench_regions.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: N = 4 at 512x1024 and at 1024x2048, the blob planes of tests/rle_oracle.py (blob_planes: 19 classes, features of about 32 pixels)
uploaded as label planes.
Forms:
  regions8                 arseg_rle_regions_fwd (8-connectivity) alone: the launch that precedes the pass
  contours8                arseg_rle_contours_fwd alone on the run code and its run_region
  encode_regions_contours  arseg_labels_rle_fwd + arseg_rle_regions_fwd + arseg_rle_contours_fwd: the chain behind the label plane
  host_runs                RleFrames.to_host() + egress.contours_numpy per frame: the host path the run code offered before, end to end
Before anything is timed, for each shape and connectivity: counts, loops and vertices must equal egress.contours_numpy's bit for bit.
No ratio is fixed in advance; the host comparison is reported, not gated.  One JSON line on stdout, the same written to --out (default
profiles/contours.json)."""
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
from arseg_amd import _lib, egress
from bench_regions import alternate


def shape_cost(N, H, W, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    lab = torch.from_numpy(rle_oracle.blob_planes(5, N, H, W)).to(dev)
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    # ---- sizing pass, then buffers with a quarter of headroom; the outlines get the capacities that cannot overflow
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), null, 0, st), "rle sizing")
    needed = row_start[:, H].cpu().numpy().astype(np.int64)
    cap = int(needed.max()) * 5 // 4 + 16
    runs = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    n_regions = torch.empty((N,), dtype=torch.int32, device=dev)
    run_region = torch.empty((N, cap), dtype=torch.int32, device=dev)
    rws_bytes = lib.arseg_rle_regions_workspace_bytes(N, cap)
    rws = torch.empty((rws_bytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    loops = torch.empty((N, cap, 4), dtype=torch.int32, device=dev)
    verts = torch.empty((N, 4 * cap), dtype=torch.int32, device=dev)
    ws_bytes = lib.arseg_rle_contours_workspace_bytes(N, cap)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)

    def encode():
        _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), P(runs), cap, st), "rle encode")

    def regions(connectivity=8):
        _lib.check(lib.arseg_rle_regions_fwd(P(row_start), P(runs), cap, N, H, W, connectivity, P(n_regions), P(run_region), null, 0, P(rws),
                                             rws_bytes, st), "regions")

    def contours(connectivity=8):
        _lib.check(lib.arseg_rle_contours_fwd(P(row_start), P(runs), P(n_regions), P(run_region), cap, N, H, W, connectivity, P(counts),
                                              P(loops), cap, P(verts), 4 * cap, P(ws), ws_bytes, st), "contours")

    def chain():
        encode()
        regions()
        contours()

    # ---- correctness first: bit for bit against the host form
    encode()
    coded = egress.RleFrames(row_start, runs, H, W)
    host_code = coded.to_host()
    per_frame = {}
    for connectivity in (4, 8):
        regions(connectivity)
        contours(connectivity)
        torch.cuda.synchronize()
        got_counts, got_loops, got_verts = counts.cpu().numpy(), loops.cpu().numpy(), verts.cpu().numpy().view(np.uint32)
        for n, (rs, words) in enumerate(host_code):
            want = egress.contours_numpy(rs, words, H, W, connectivity)
            L, V = want[0]
            if not (np.array_equal(got_counts[n], want[0]) and np.array_equal(got_loops[n, :L], want[1]) and np.array_equal(got_verts[n, :V], want[2])):
                raise SystemExit(f"{name}, {connectivity}-connectivity, frame {n}: the outlines differ from contours_numpy's")
        per_frame[connectivity] = got_counts.tolist()
    regions()

    def host_runs():
        for rs, words in coded.to_host():
            egress.contours_numpy(rs, words, H, W, 8)

    res = alternate({"regions8": regions, "contours8": contours, "encode_regions_contours": chain, "host_runs": host_runs}, repeats, window)
    c, k = res["contours8"], res["encode_regions_contours"]
    verdict = {"contours8_alone_us": c["us_median"], "contours_over_regions": c["us_median"] / res["regions8"]["us_median"],
               "chain_us": k["us_median"], "host_runs_over_chain": res["host_runs"]["us_median"] / k["us_median"]}
    inputs = {"runs_per_frame": needed.tolist(), "loops_vertices_per_frame_4": per_frame[4], "loops_vertices_per_frame_8": per_frame[8],
              "capacity": cap, "workspace_bytes": int(ws_bytes), "jump_launches": int(np.ceil(np.log2(2 * cap)))}
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()) +
          f"; runs/frame {int(needed.mean())}, loops/frame {int(np.mean([p[0] for p in per_frame[8]]))}, "
          f"vertices/frame {int(np.mean([p[1] for p in per_frame[8]]))}", file=sys.stderr)
    return {"planes": [N, H, W], "inputs": inputs, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contours.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for H, W in ((512, 1024), (1024, 2048)):
        res["shapes"].append(shape_cost(4, H, W, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
