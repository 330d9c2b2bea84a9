#!/usr/bin/env python3
"""What it costs to get a GOP's decoder motion into mv_q, the int16 field the fast paths read.  One process, routes alternated, --repeats
windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of tools/bench_ingest.py.

Shapes: 720x960 and 1024x2048, 11 P-frames per GOP, motion from synth.make_record_chain / make_mv_chain (8- and 16-pixel blocks).  Routes:
  records            ingest.MotionChain.push_gop from block records already on the device (reset + 11 x (scatter, compose))
  dense              ops.merge_motion from the dense per-frame fields already on the device: the yardstick, the code this route replaces,
                     run in the same process
  records_upload     `records` plus the pinned-host -> device copy of its input (11 record buffers)
  dense_upload       `dense` plus the pinned-host -> device copy of its input (the [12,H,W,3] dumps)
Per route: us per GOP, the bytes the route MUST move (its input once + its output once), the size of its workspace, and for the upload
routes the bytes that cross the link.  The two device routes are compared bit for bit before anything is timed.  One JSON line on stdout,
the same written to --out (default profiles/mv_records.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from arseg_amd import _lib, ingest, ops, synth


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
    return {k: {"us_per_gop_median": 1e3 * statistics.median(v), "us_per_gop_min": 1e3 * min(v), "us_per_gop_max": 1e3 * max(v)} for k, v in ms.items()}


def shape_cost(H, W, F, repeats, window, dev):
    flows = synth.make_mv_chain(7, H, W, F)
    recs = synth.make_record_chain(7, H, W, F)
    lib = _lib.load()
    rec_dev = [torch.from_numpy(r).to(dev) for r in recs]
    rec_pin = [torch.from_numpy(r).pin_memory() for r in recs]
    rec_stage = [torch.empty_like(r) for r in rec_dev]
    dense_dev = torch.from_numpy(flows).to(dev)
    dense_pin = torch.from_numpy(flows).pin_memory()
    dense_stage = torch.empty_like(dense_dev)
    chain = ingest.MotionChain(H, W, gop=F + 1, device=dev)

    def records_upload():
        for s, p in zip(rec_stage, rec_pin):
            s.copy_(p, non_blocking=True)
        return chain.push_gop(rec_stage)

    def dense_upload():
        dense_stage.copy_(dense_pin, non_blocking=True)
        return ops.merge_motion(dense_stage)

    forms = {"records": lambda: chain.push_gop(rec_dev), "dense": lambda: ops.merge_motion(dense_dev), "records_upload": records_upload, "dense_upload": dense_upload}
    want = ops.merge_motion(dense_dev)
    equal = {k: bool(torch.equal(fn(), want)) for k, fn in forms.items()}
    if not all(equal.values()):
        raise SystemExit(f"{H}x{W}: the routes disagree: {equal}")
    res = alternate(forms, repeats, window)
    rec_bytes = sum(r.nbytes for r in recs)
    out_b = F * H * W * 4                                               # the F frames of mv_q the fast paths read
    info = {"records": {"bytes_needed": rec_bytes + out_b, "workspace_bytes": int(lib.arseg_mv_records_workspace_bytes(H, W)), "upload_bytes": 0},
            "dense": {"bytes_needed": F * H * W * 6 + out_b, "workspace_bytes": int(lib.arseg_merge_motion_workspace_bytes(F, H, W)), "upload_bytes": 0}}
    info["records_upload"] = dict(info["records"], upload_bytes=rec_bytes)
    info["dense_upload"] = dict(info["dense"], upload_bytes=int(flows.nbytes))
    for k, r in res.items():
        r.update(info[k])
        r["GBps_of_needed_bytes"] = r["bytes_needed"] / (r["us_per_gop_median"] * 1e-6) / 1e9
        r["equals_merge_motion"] = equal[k]
    res["records"]["time_over_dense"] = res["records"]["us_per_gop_median"] / res["dense"]["us_per_gop_median"]
    res["records_upload"]["time_over_dense_upload"] = res["records_upload"]["us_per_gop_median"] / res["dense_upload"]["us_per_gop_median"]
    print(f"{H}x{W}, {F} P-frames, {sum(r.shape[0] for r in recs)} records ({rec_bytes} B): " +
          ", ".join(f"{k} {r['us_per_gop_median']:.1f} us ({r['us_per_gop_min']:.1f}-{r['us_per_gop_max']:.1f})" for k, r in res.items()), file=sys.stderr)
    return {"frame": [H, W], "p_frames": F, "records_per_frame": [int(r.shape[0]) for r in recs], "record_bytes_per_gop": rec_bytes,
            "dense_bytes_per_gop": int(flows.nbytes), "routes": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", default="720x960,1024x2048")
    ap.add_argument("--p-frames", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mv_records.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_records.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for s in a.shapes.split(","):
        H, W = (int(v) for v in s.lower().split("x"))
        res["shapes"].append(shape_cost(H, W, a.p_frames, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
