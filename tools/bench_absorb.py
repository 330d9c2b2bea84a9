#!/usr/bin/env python3
"""What absorbing the small regions of the masks costs on the GPU, and what the host path it replaces costs: arseg_rle_absorb_fwd
(csrc/absorb.hip) between two arseg_rle_regions_fwd, against pulling the run code and the records to the host, absorbing there and
uploading the new code.  One process, forms alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream for
the GPU forms, wall time for the host form), median and min-max; the protocol of tools/bench_regions.py.  The kernel forms are bare ABI
calls on preallocated buffers.

Shapes: N = 4 at 512x1024 and at 1024x2048, the blob planes of tests/rle_oracle.py (blob_planes: 19 classes, features of about 32 pixels)
salted with specks: one pixel in 500 set to a random class, a quarter of them grown to 2x2.  min_area 16, nothing protected.
Forms:
  regions8                arseg_rle_regions_fwd (8-connectivity) on the salted planes' run code: the launch that precedes the pass
  absorb                  arseg_rle_absorb_fwd alone (pair capacity 3 x run capacity)
  regions_absorb_regions  regions8, absorb, regions8 on the new code: the device chain
  host_absorb             the run code and the records device -> host (RleFrames.to_host, RegionFrames.to_host), egress.absorb_numpy per
                          frame, the new code host -> device: what the parent commit offers
Before anything is timed, for each shape: the new code and the targets must equal egress.absorb_numpy's bit for bit.
No ratio is fixed in advance; the comparisons are reported, not gated.  One JSON line on stdout, the same written to --out (default
profiles/absorb.json)."""
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

MIN_AREA = 16


def salted(seed, N, H, W, n_cls=19):
    planes = rle_oracle.blob_planes(seed, N, H, W, n_cls=n_cls)
    g = np.random.Generator(np.random.PCG64(seed + 1))
    for n in range(N):
        count = H * W // 500
        ys, xs, vs = g.integers(0, H - 1, count), g.integers(0, W - 1, count), g.integers(0, n_cls, count).astype(np.uint8)
        planes[n, ys, xs] = vs
        big = slice(0, count // 4)
        for dy, dx in ((0, 1), (1, 0), (1, 1)):
            planes[n, ys[big] + dy, xs[big] + dx] = vs[big]
    return planes


def shape_cost(N, H, W, repeats, window, dev):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    lab = torch.from_numpy(salted(5, N, H, W)).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    # ---- sizing passes, then buffers with a quarter of headroom
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), null, 0, st), "rle sizing")
    needed = row_start[:, H].cpu().numpy().astype(np.int64)
    cap = int(needed.max()) * 5 // 4 + 16
    runs = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), P(runs), cap, st), "rle encode")
    n_regions, run_region = torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N, cap), dtype=torch.int32, device=dev)
    reg_ws_bytes = lib.arseg_rle_regions_workspace_bytes(N, cap)
    reg_ws = torch.empty((reg_ws_bytes,), dtype=torch.uint8, device=dev)
    _lib.check(lib.arseg_rle_regions_fwd(P(row_start), P(runs), cap, N, H, W, 8, P(n_regions), P(run_region), null, 0, P(reg_ws), reg_ws_bytes,
                                         st), "regions sizing")
    rcap = int(n_regions.max()) * 5 // 4 + 16
    records = torch.empty((N, rcap, 8), dtype=torch.int64, device=dev)
    pcap = 3 * cap
    ws_bytes = lib.arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, pcap)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    out_rs, out_runs = torch.zeros_like(row_start), torch.empty_like(runs)
    target, n_absorbed = torch.empty((N, rcap), dtype=torch.int32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev)
    n_regions2, run_region2, records2 = torch.empty_like(n_regions), torch.empty_like(run_region), torch.empty_like(records)

    def regions(rs=row_start, words=runs, n=n_regions, rr=run_region, rec=records):
        _lib.check(lib.arseg_rle_regions_fwd(P(rs), P(words), cap, N, H, W, 8, P(n), P(rr), P(rec), rcap, P(reg_ws), reg_ws_bytes, st), "regions")

    def absorb():
        _lib.check(lib.arseg_rle_absorb_fwd(P(row_start), P(runs), P(n_regions), P(run_region), cap, P(records), rcap, N, H, W, MIN_AREA, None,
                                            P(out_rs), P(out_runs), cap, P(target), rcap, P(n_absorbed), pcap, P(ws), ws_bytes, st), "absorb")

    def chain():
        regions()
        absorb()
        regions(out_rs, out_runs, n_regions2, run_region2, records2)

    # ---- correctness first: bit for bit against the host form
    chain()
    torch.cuda.synchronize()
    coded = egress.RleFrames(row_start, runs, H, W)
    found = egress.RegionFrames(n_regions, run_region, records, coded)
    cleaned = egress.AbsorbedFrames(out_rs, out_runs, H, W, target, n_absorbed, found, pcap)
    got, got_targets = cleaned.to_host(), cleaned.targets_to_host()
    for n, (rs, words) in enumerate(coded.to_host()):
        want = egress.absorb_numpy(rs, words, H, W, MIN_AREA)
        if not (np.array_equal(got[n][0], want[0]) and np.array_equal(got[n][1], want[1]) and np.array_equal(got_targets[n], want[2])):
            raise SystemExit(f"{name}, frame {n}: the new code or the targets differ from absorb_numpy's")

    up_rs, up_runs = torch.empty_like(row_start), torch.empty_like(runs)

    def host_absorb():
        found.to_host()
        for n, (rs, words) in enumerate(coded.to_host()):
            new_rs, new_words, _ = egress.absorb_numpy(rs, words, H, W, MIN_AREA)
            up_rs[n].copy_(torch.from_numpy(new_rs))
            up_runs[n, :len(new_words)].copy_(torch.from_numpy(new_words.view(np.int32)))
        torch.cuda.synchronize()

    res = alternate({"regions8": regions, "absorb": absorb, "regions_absorb_regions": chain, "host_absorb": host_absorb}, repeats, window)
    verdict = {"absorb_over_regions8": res["absorb"]["us_median"] / res["regions8"]["us_median"],
               "host_absorb_over_absorb": res["host_absorb"]["us_median"] / res["absorb"]["us_median"],
               "host_absorb_over_chain": res["host_absorb"]["us_median"] / res["regions_absorb_regions"]["us_median"]}
    inputs = {"runs_per_frame": needed.tolist(), "runs_after": out_rs[:, H].cpu().tolist(), "regions_per_frame": n_regions.cpu().tolist(),
              "regions_after": n_regions2.cpu().tolist(), "absorbed_per_frame": n_absorbed.cpu().tolist(), "min_area": MIN_AREA, "capacity": cap,
              "region_capacity": rcap, "pair_capacity": pcap, "workspace_bytes": int(ws_bytes)}
    print(f"{name}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; runs/frame {int(needed.mean())}, regions/frame {int(n_regions.float().mean())}, absorbed/frame {int(n_absorbed.float().mean())}",
          file=sys.stderr)
    return {"planes": [N, H, W], "inputs": inputs, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absorb.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_absorb.py measures on the GPU; none found")
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
