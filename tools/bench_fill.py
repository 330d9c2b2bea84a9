#!/usr/bin/env python3
"""What filling the polygons back into a mask costs on the GPU: arseg_contours_fill_fwd (csrc/fill.hip) alone, on the polygons of
arseg_contours_simplify_shared_fwd, with the reference plane and the counters, against the launches around it on the same frames.  One
process, forms alternated, --repeats windows of >= --window seconds each, HIP events on the launch stream, median and min-max; the
protocol of tools/bench_simplify.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: N = 4 at 512x1024 and at 1024x2048, the blob planes of tests/rle_oracle.py uploaded as label planes, 8-connectivity.
Tolerances: 0.5, 1 and 2 px.
Forms:
  contours8            arseg_rle_contours_fwd alone: a yardstick
  decode               arseg_rle_decode_fwd alone: a yardstick, the other way back to a plane
  shared_T             arseg_contours_simplify_shared_fwd alone at tolerance T: a yardstick, the launch that precedes the pass
  fill_T               arseg_contours_fill_fwd alone on shared_T's polygons
  fill_sizing_T        its sizing pass: the clear, count and scan launches (the scatter and row launches are the difference to fill_T)
  fill_exact           arseg_contours_fill_fwd on the exact outlines: two unit crossings per run
Before anything is timed, for each shape and tolerance: every output plane, gaps and excess must equal egress.fill_numpy's bit for bit
(gaps and excess are reported: 0 is what the shared borders promise).  After the timing the kernels of one call at 1 px are timed one
by one (torch.profiler's device times, the median of 20 calls; "unavailable" where the profiler gives none).  No time is fixed in advance; the ratios are reported, not
gated.  One JSON line on stdout, the same written to --out (default profiles/fill.json)."""
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
from arseg_amd import _lib, egress, ops
from bench_regions import alternate

TOLERANCES = (0.5, 1.0, 2.0)


def shape_cost(N, H, W, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    planes = rle_oracle.blob_planes(5, N, H, W)
    lab = torch.from_numpy(planes).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())

    # ---- the chain up to the polygons, through the package; capacities with a quarter of headroom
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    ops.labels_rle(lab, row_start, None)
    cap = int(row_start[:, H].max()) * 5 // 4 + 16
    frames = egress.rle_of_planes(lab, cap)
    found = egress.regions(frames, cap)
    outlines = egress.contours(found)
    shared = {t: egress.simplify_shared(outlines, t) for t in TOLERANCES}
    lcap, vcap, rcap, ecap = outlines.loop_capacity, outlines.vertex_capacity, found.capacity, 2 * cap
    out_plane = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    counts_out = torch.empty((N,), dtype=torch.int32, device=dev)
    stats = torch.empty((N, _lib.FILL_NSTATS), dtype=torch.int64, device=dev)
    ws_bytes = lib.arseg_contours_fill_workspace_bytes(N, H, W, lcap, max(s.vertex_capacity for s in shared.values()), ecap)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    decoded = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    sws_bytes = lib.arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap)

    def contours():
        _lib.check(lib.arseg_rle_contours_fwd(P(frames.row_start), P(frames.runs), P(found.n_regions), P(found.run_region), cap, N, H, W, 8,
                                              P(outlines.counts), P(outlines.loops), lcap, P(outlines.verts), vcap, P(outlines.workspace),
                                              outlines.workspace.numel() * 4, st), "contours")

    def decode():
        _lib.check(lib.arseg_rle_decode_fwd(P(frames.row_start), P(frames.runs), cap, N, H, W, P(decoded), W, H * W, st), "decode")

    def simplify(tolerance):
        got, tol2_q = shared[tolerance], ops.tolerance_q(tolerance)

        def run():
            _lib.check(lib.arseg_contours_simplify_shared_fwd(P(frames.row_start), P(frames.runs), cap, P(outlines.counts), P(outlines.loops), lcap,
                                                              P(outlines.verts), vcap, N, H, W, tol2_q, P(got.counts), P(got.loops), P(got.verts),
                                                              got.vertex_capacity, P(got.workspace), got.workspace.numel() * 4, st), "shared")
        return run

    def fill(polygons, sizing=False):
        def run():
            _lib.check(lib.arseg_contours_fill_fwd(P(polygons.counts), P(polygons.loops), lcap, P(polygons.verts), polygons.vertex_capacity,
                                                   P(found.n_regions), P(found.records), rcap, N, H, W, 255, null if sizing else P(lab), W, H * W,
                                                   null if sizing else P(out_plane), W, H * W, P(counts_out), null if sizing else P(stats),
                                                   0 if sizing else ecap, P(ws), ws_bytes, st), "fill")
        return run

    # ---- correctness first: bit for bit against the host form
    values = [rec["value"] for rec in found.to_host()]
    crossings, fidelity = {}, {}
    for key, polygons in [("exact", outlines)] + [(t, shared[t]) for t in TOLERANCES]:
        fill(polygons)()
        torch.cuda.synchronize()
        need = polygons.counts.cpu().numpy()
        got, rows = out_plane.cpu().numpy(), stats.cpu().numpy()
        for n in range(N):
            L, V = need[n]
            want, gaps, excess = egress.fill_numpy(need[n], polygons.loops[n, :L].cpu().numpy(), polygons.verts[n, :V].cpu().numpy(), values[n], H, W)
            if not np.array_equal(got[n], want) or (int(rows[n, 0]), int(rows[n, 1])) != (gaps, excess):
                raise SystemExit(f"{name}, {key}, frame {n}: the filled plane, gaps or excess differ from fill_numpy's")
            if int(rows[n, 2]) != int((want != planes[n]).sum()):
                raise SystemExit(f"{name}, {key}, frame {n}: changed differs from the planes' difference")
        crossings[str(key)] = counts_out.cpu().tolist()
        fidelity[str(key)] = {"gaps_per_frame": rows[:, 0].tolist(), "excess_per_frame": rows[:, 1].tolist(), "changed_per_frame": rows[:, 2].tolist()}

    forms = {"contours8": contours, "decode": decode, "fill_exact": fill(outlines)}
    for tolerance in TOLERANCES:
        forms[f"shared_{tolerance}"] = simplify(tolerance)
        forms[f"fill_{tolerance}"] = fill(shared[tolerance])
        forms[f"fill_sizing_{tolerance}"] = fill(shared[tolerance], True)
    res = alternate(forms, repeats, window)
    c, d = res["contours8"]["us_median"], res["decode"]["us_median"]
    verdict = {"contours8_alone_us": c, "decode_alone_us": d, "fill_exact_us": res["fill_exact"]["us_median"]}
    for tolerance in TOLERANCES:
        s, f, z = (res[f"{form}_{tolerance}"]["us_median"] for form in ("shared", "fill", "fill_sizing"))
        verdict[f"{tolerance}"] = {"fill_alone_us": f, "clear_count_scan_us": z, "scatter_rows_us": f - z, "fill_over_contours": f / c,
                                   "fill_over_decode": f / d, "fill_over_shared": f / s, "shared_alone_us": s}
    launches = per_launch(fill(shared[1.0]))
    inputs = {"runs_per_frame": frames.needed().cpu().tolist(), "loops_per_frame": outlines.counts[:, 0].cpu().tolist(),
              "crossings_per_frame": crossings, "fidelity": fidelity, "event_capacity": ecap, "workspace_bytes": int(ws_bytes),
              "shared_workspace_bytes": int(sws_bytes)}
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()) +
          f"; crossings/frame {crossings}; workspace {ws_bytes} bytes; launches at 1 px {launches}", file=sys.stderr)
    return {"planes": [N, H, W], "inputs": inputs, "verdict": verdict, "launches_1px_us": launches, "forms": res}


LAUNCHES = {"clear": "clear", "edges<false>": "count", "scan": "scan", "edges<true>": "scatter", "rows<false>": "rows", "rows<true>": "rows"}


def per_launch(run, calls=20):
    """The kernels of one call, timed one by one: {launch: median device time in us over `calls` calls}."""
    try:
        from torch.profiler import ProfilerActivity, profile
        run()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                run()
            torch.cuda.synchronize()
        times = {}
        for event in prof.events():
            if "fill_" in event.name and "_kernel" in event.name:
                kernel = event.name.split("fill_")[-1].split("(")[0].replace("_kernel", "").replace(" ", "")
                times.setdefault(LAUNCHES.get(kernel, kernel), []).append(float(getattr(event, "device_time", 0.0) or getattr(event, "cuda_time", 0.0)))
        return {k: float(np.median(v)) for k, v in times.items()} or "unavailable"
    except Exception as exc:                                      # the profiler is an aid: the timing above does not depend on it
        return f"unavailable ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fill.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "tolerances_px": list(TOLERANCES), "shapes": []}
    for H, W in ((512, 1024), (1024, 2048)):
        res["shapes"].append(shape_cost(4, H, W, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
