#!/usr/bin/env python3
"""What the connected regions of the masks cost on the GPU, and what the host path they replace costs: arseg_rle_regions_fwd
(csrc/regions.hip) behind the label plane and its run code, against pulling the run code (or the plane) to the host and labelling there.
One process, forms alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream for the GPU forms, wall time
for the host forms), median and min-max; the protocol of tools/bench_rle.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: N = 11 (the non-keyframes of a GOP) at 720x960 and at 1024x2048, the blob planes of tests/rle_oracle.py (blob_planes: 19 classes,
features of about 32 pixels) uploaded as label planes; head logits [N,19,H/8,W/8] whose x8 argmax route gives the yardstick its labels8 launch.
Forms:
  labels8_encode          arseg_segment_egress_fwd (the label plane) + arseg_labels_rle_fwd: the yardstick, the parent commit's code
  labels8_encode_regions  the same plus arseg_rle_regions_fwd (8-connectivity) on the run code
  regions4 / regions8     arseg_rle_regions_fwd alone on the blob planes' run code, either connectivity
  host_runs               RleFrames.to_host() + egress.regions_numpy per frame: the host path on the run code, end to end
  host_scipy              the plane device -> host + scipy.ndimage.label per value and frame (where scipy is importable)
Before anything is timed, for each shape and connectivity: run_region and the records must equal egress.regions_numpy's bit for bit.
The time regions add over the yardstick is set against the two min-max spreads together; no ratio is fixed in advance, and the host
comparison is reported, not gated.  One JSON line on stdout, the same written to --out (default profiles/regions.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import rle_oracle
from arseg_amd import _lib, egress


def window_ms(fn, min_s, host):
    fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < 1e3 * min_s:
        if host:
            t0 = time.perf_counter()
            fn()
            total += 1e3 * (time.perf_counter() - t0)
            n += 1
            continue
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
            ms[k].append(window_ms(fn, window, k.startswith("host_")))
    return {k: {"us_median": 1e3 * statistics.median(v), "us_min": 1e3 * min(v), "us_max": 1e3 * max(v)} for k, v in ms.items()}


def shape_cost(N, H, W, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    planes = rle_oracle.blob_planes(5, N, H, W)
    lab = torch.from_numpy(planes).to(dev)
    n_cls, h, w = 19, H // 8, W // 8
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, h, w)).astype(np.float32)).to(dev)
    lab8 = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    # ---- sizing passes, then buffers with a quarter of headroom
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), null, 0, st), "rle sizing")
    needed = row_start[:, H].cpu().numpy().astype(np.int64)
    cap = int(needed.max()) * 5 // 4 + 16
    runs = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), P(runs), cap, st), "rle encode")
    n_regions = torch.empty((N,), dtype=torch.int32, device=dev)
    run_region = torch.empty((N, cap), dtype=torch.int32, device=dev)
    ws_bytes = lib.arseg_rle_regions_workspace_bytes(N, cap)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _lib.check(lib.arseg_rle_regions_fwd(P(row_start), P(runs), cap, N, H, W, 4, P(n_regions), P(run_region), null, 0, P(ws), ws_bytes, st),
               "regions sizing")
    rcap = int(n_regions.max()) * 5 // 4 + 16
    records = torch.empty((N, rcap, 8), dtype=torch.int64, device=dev)

    def regions(connectivity, rs=row_start, words=runs):
        def run():
            _lib.check(lib.arseg_rle_regions_fwd(P(rs), P(words), cap, N, H, W, connectivity, P(n_regions), P(run_region), P(records), rcap,
                                                 P(ws), ws_bytes, st), "regions")
        return run

    # ---- correctness first: bit for bit against the host form
    coded = egress.RleFrames(row_start, runs, H, W)
    host_code = coded.to_host()
    per_frame = {}
    for connectivity in (4, 8):
        regions(connectivity)()
        torch.cuda.synchronize()
        got_n, got_rr, got_rec = n_regions.cpu().numpy(), run_region.cpu().numpy(), records.cpu().numpy()
        for n, (rs, words) in enumerate(host_code):
            rec, rr = egress.regions_numpy(rs, words, H, W, connectivity, return_run_region=True)
            if got_n[n] != len(rec) or not np.array_equal(got_rr[n, :len(rr)], rr):
                raise SystemExit(f"{name}, {connectivity}-connectivity, frame {n}: the region numbers differ from regions_numpy's")
            rows = got_rec[n, :len(rec)]
            same = all(np.array_equal(rows[:, k], rec[f]) for k, f in enumerate(egress.REGION_DTYPE.names[:6]))
            if not same or not np.array_equal(rows[:, 6] / rows[:, 1], rec["cx"]) or not np.array_equal(rows[:, 7] / rows[:, 1], rec["cy"]):
                raise SystemExit(f"{name}, {connectivity}-connectivity, frame {n}: the records differ from regions_numpy's")
        per_frame[connectivity] = got_n.tolist()

    # ---- the chain from logits: its own plane, run code and regions (noise logits: the yardstick's cost does not depend on the labels, the
    # regions' does, so the chain labels the blob planes' run code while labels8 + encode run on the logits' plane)
    rs2 = torch.empty_like(row_start)

    def labels8_encode():
        _lib.check(lib.arseg_segment_egress_fwd(P(logits), N, n_cls, h, w, H, W, 0, None, P(lab8), W, H * W, 0, null, null, null, 0, 0, 0, 0, 0, 0,
                                                null, null, null, 0, 0, 0, 0, 0, 0, None, None, st), "egress")
        _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(rs2), P(runs), cap, st), "rle encode")

    def chain():
        labels8_encode()
        regions(8, rs2)()

    pin = torch.empty((N, H, W), dtype=torch.uint8).pin_memory()

    def host_runs():
        for rs, words in coded.to_host():
            egress.regions_numpy(rs, words, H, W, 8)

    forms = {"labels8_encode": labels8_encode, "labels8_encode_regions": chain, "regions4": regions(4), "regions8": regions(8),
             "host_runs": host_runs}
    try:
        from scipy import ndimage

        structure = ndimage.generate_binary_structure(2, 2)

        def host_scipy():
            pin.copy_(lab, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            p = pin.numpy()
            for n in range(N):
                for v in np.unique(p[n]):
                    ndimage.label(p[n] == v, structure=structure)

        forms["host_scipy"] = host_scipy
    except ImportError:
        pass
    res = alternate(forms, repeats, window)
    y, c = res["labels8_encode"], res["labels8_encode_regions"]
    spreads = (y["us_max"] - y["us_min"]) + (c["us_max"] - c["us_min"])
    added = c["us_median"] - y["us_median"]
    verdict = {"regions_add_us": added, "spreads_us": spreads, "added_beyond_spreads": bool(added > spreads),
               "regions8_alone_us": res["regions8"]["us_median"], "chain_over_yardstick": c["us_median"] / y["us_median"],
               "host_runs_over_chain": res["host_runs"]["us_median"] / c["us_median"]}
    if "host_scipy" in res:
        verdict["host_scipy_over_chain"] = res["host_scipy"]["us_median"] / c["us_median"]
    inputs = {"runs_per_frame": needed.tolist(), "regions_per_frame_4": per_frame[4], "regions_per_frame_8": per_frame[8], "capacity": cap,
              "region_capacity": rcap, "workspace_bytes": int(ws_bytes)}
    print(f"{name}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; runs/frame {int(needed.mean())}, regions/frame {int(np.mean(per_frame[8]))}", file=sys.stderr)
    return {"planes": [N, H, W], "inputs": inputs, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for H, W in ((720, 960), (1024, 2048)):
        res["shapes"].append(shape_cost(11, H, W, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
