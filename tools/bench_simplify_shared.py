#!/usr/bin/env python3
"""What simplifying the outlines with shared borders costs on the GPU: arseg_contours_simplify_shared_fwd (csrc/simplify_shared.hip)
behind arseg_rle_contours_fwd, against the two yardsticks taken in the same run on the same frames -- arseg_contours_simplify_fwd alone
(the same walk without the run-code searches: what do the mark, scan and expand launches add?) and arseg_rle_contours_fwd alone.  One
process, forms alternated, --repeats windows of >= --window seconds each, HIP events on the launch stream, median and min-max; the
protocol of tools/bench_simplify.py.  The forms are bare ABI calls on preallocated buffers.

Shapes: N = 4 at 512x1024 and at 1024x2048, the blob planes of tests/rle_oracle.py uploaded as label planes, 8-connectivity.
Tolerances: 0.5, 1 and 2 px.
Forms:
  contours8            arseg_rle_contours_fwd alone
  simplify_T           arseg_contours_simplify_fwd alone at tolerance T
  shared_T             arseg_contours_simplify_shared_fwd alone at tolerance T
Before anything is timed, for each shape and tolerance: counts, loops and kept vertices must equal egress.simplify_shared_numpy's bit for
bit.  After the timing the kernels of one shared call at 1 px are timed one by one (torch.profiler's device times, the median of 20
calls; "unavailable" where the profiler gives none).  No time is fixed in advance; the comparisons are reported, not gated.  One JSON
line on stdout, the same written to --out (default profiles/simplify_shared.json)."""
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
    lab = torch.from_numpy(rle_oracle.blob_planes(5, N, H, W)).to(dev)
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    # ---- sizing pass, then buffers with a quarter of headroom; the outlines get the capacities that cannot overflow
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), null, 0, st), "rle sizing")
    cap = int(row_start[:, H].max()) * 5 // 4 + 16
    lcap, vcap = cap, 4 * cap
    runs = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    n_regions = torch.empty((N,), dtype=torch.int32, device=dev)
    run_region = torch.empty((N, cap), dtype=torch.int32, device=dev)
    rws_bytes = lib.arseg_rle_regions_workspace_bytes(N, cap)
    rws = torch.empty((rws_bytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    loops = torch.empty((N, lcap, 4), dtype=torch.int32, device=dev)
    verts = torch.empty((N, vcap), dtype=torch.int32, device=dev)
    cws_bytes = lib.arseg_rle_contours_workspace_bytes(N, cap)
    cws = torch.empty((cws_bytes,), dtype=torch.uint8, device=dev)
    counts_out = torch.empty((N, 2), dtype=torch.int32, device=dev)
    loops_out = torch.empty((N, lcap, 4), dtype=torch.int32, device=dev)
    verts_out = torch.empty((N, vcap + 2 * cap), dtype=torch.int32, device=dev)
    sws_bytes = lib.arseg_contours_simplify_workspace_bytes(N, lcap, vcap)
    sws = torch.empty((sws_bytes,), dtype=torch.uint8, device=dev)
    hws_bytes = lib.arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap)
    hws = torch.empty((hws_bytes,), dtype=torch.uint8, device=dev)

    def contours():
        _lib.check(lib.arseg_rle_contours_fwd(P(row_start), P(runs), P(n_regions), P(run_region), cap, N, H, W, 8, P(counts), P(loops), lcap,
                                              P(verts), vcap, P(cws), cws_bytes, st), "contours")

    def simplify(tolerance):
        tol2_q = ops.tolerance_q(tolerance)

        def run():
            _lib.check(lib.arseg_contours_simplify_fwd(P(counts), P(loops), lcap, P(verts), vcap, N, H, W, tol2_q, P(counts_out), P(loops_out),
                                                       P(verts_out), vcap, P(sws), sws_bytes, st), "simplify")
        return run

    def shared(tolerance):
        tol2_q = ops.tolerance_q(tolerance)

        def run():
            _lib.check(lib.arseg_contours_simplify_shared_fwd(P(row_start), P(runs), cap, P(counts), P(loops), lcap, P(verts), vcap, N, H, W, tol2_q,
                                                              P(counts_out), P(loops_out), P(verts_out), vcap + 2 * cap, P(hws), hws_bytes, st),
                       "simplify_shared")
        return run

    def outlines():
        _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), P(runs), cap, st), "rle encode")
        _lib.check(lib.arseg_rle_regions_fwd(P(row_start), P(runs), cap, N, H, W, 8, P(n_regions), P(run_region), null, 0, P(rws), rws_bytes, st),
                   "regions")
        contours()

    def to_host():
        need = counts.cpu().numpy()
        return need, loops[:, :int(need[:, 0].max())].cpu().numpy(), verts[:, :int(need[:, 1].max())].cpu().numpy()

    # ---- correctness first: bit for bit against the host form
    outlines()
    torch.cuda.synchronize()
    need, rows, words = to_host()
    codes = egress.RleFrames(row_start, runs, H, W).to_host()
    longest = int(max(rows[n, :need[n, 0], 2].max() for n in range(N)))
    kept, plain = {}, {}
    for tolerance in TOLERANCES:
        simplify(tolerance)()
        torch.cuda.synchronize()
        plain[tolerance] = counts_out.cpu().numpy()[:, 1].tolist()
        shared(tolerance)()
        torch.cuda.synchronize()
        got_counts, got_loops, got_verts = counts_out.cpu().numpy(), loops_out.cpu().numpy(), verts_out.cpu().numpy().view(np.uint32)
        for n in range(N):
            want = egress.simplify_shared_numpy(*codes[n], H, W, need[n], rows[n], words[n], tolerance)
            L, V = want[0]
            if not (np.array_equal(got_counts[n], want[0]) and np.array_equal(got_loops[n, :L], want[1]) and np.array_equal(got_verts[n, :V], want[2])):
                raise SystemExit(f"{name}, {tolerance} px, frame {n}: the outlines differ from simplify_shared_numpy's")
        kept[tolerance] = got_counts[:, 1].tolist()
    shared(0.0)()
    torch.cuda.synchronize()
    expanded = counts_out.cpu().numpy()[:, 1].tolist()

    forms = {"contours8": contours}
    for tolerance in TOLERANCES:
        forms[f"simplify_{tolerance}"] = simplify(tolerance)
        forms[f"shared_{tolerance}"] = shared(tolerance)
    res = alternate(forms, repeats, window)
    c = res["contours8"]["us_median"]
    verdict = {"contours8_alone_us": c}
    for tolerance in TOLERANCES:
        s, h = (res[f"{form}_{tolerance}"]["us_median"] for form in ("simplify", "shared"))
        verdict[f"{tolerance}"] = {"simplify_alone_us": s, "shared_alone_us": h, "shared_over_simplify": h / s, "shared_over_contours": h / c}
    launches = per_launch(shared(1.0))
    inputs = {"loops_per_frame": need[:, 0].tolist(), "vertices_in_per_frame": need[:, 1].tolist(), "runs_per_frame": row_start[:, H].tolist(),
              "expanded_vertices_per_frame": expanded, "vertices_out_per_frame": {str(t): v for t, v in kept.items()},
              "vertices_out_per_frame_simplify": {str(t): v for t, v in plain.items()}, "longest_loop_vertices": longest, "loop_capacity": lcap,
              "vertex_capacity": vcap, "workspace_bytes": int(hws_bytes), "workspace_bytes_simplify": int(sws_bytes)}
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()) +
          f"; vertices/frame {int(need[:, 1].mean())} -> expanded {int(np.mean(expanded))} -> " +
          ", ".join(f"{int(np.mean(v))} at {t} px" for t, v in kept.items()) + f"; longest loop {longest}; launches at 1 px {launches}", file=sys.stderr)
    return {"planes": [N, H, W], "inputs": inputs, "verdict": verdict, "launches_1px_us": launches, "forms": res}


def per_launch(run, calls=20):
    """The kernels of one call, timed one by one: {kernel name: median device time in us over `calls` calls}."""
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
            if "simplify_shared" in event.name:
                kernel = event.name.split("simplify_shared_")[-1].split("_kernel")[0]
                times.setdefault(kernel, []).append(float(getattr(event, "device_time", 0.0) or getattr(event, "cuda_time", 0.0)))
        return {k: float(np.median(v)) for k, v in times.items()} or "unavailable"
    except Exception as exc:                                      # the profiler is an aid: the timing above does not depend on it
        return f"unavailable ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_shared.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify_shared.py measures on the GPU; none found")
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
