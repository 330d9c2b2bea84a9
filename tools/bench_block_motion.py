#!/usr/bin/env python3
"""What block motion estimation costs per frame, next to the chain step that consumes its records.  One process, forms alternated,
--repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of
tools/bench_mv_records.py.

Cases: 720x960 at search 16 and 1024x2048 at search 32, blocks of 16 and of 8; NV12 luma planes on the device, the current frame a window
of the reference's noise canvas moved by (5, -3) with +-2 of noise on every sample (so that no SAD is 0 and the search has to find the
shift).  Forms per case:
  estimate   ingest.MotionEstimator.estimate: the one launch of arseg_block_motion_fwd
  push       ingest.MotionChain.push of the records it left (frame 1 of a GOP of 2, pushed again and again: the index map is clean after
             every step), the plain P entry
Before anything is timed, on a noise-free copy of the pair: every block whose true displacement is a candidate must come back with exactly
that vector and SAD 0 (the translation check of tests/test_block_motion.py at full size), and no block may be intra.
Per form: us per frame.  One JSON line on stdout, the same written to --out (default profiles/block_motion.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from arseg_amd import _lib, ingest
from bench_mv_brecords import alternate

SHIFT = (5, -3)          # cur[y][x] = ref[y + sy][x + sx], (sx, sy)


def frames(H, W, dev, noisy):
    g = np.random.Generator(np.random.PCG64(11))
    m = 8
    cv = g.integers(0, 256, (H + 2 * m, W + 2 * m), dtype=np.uint8)
    ref, cur = cv[m:m + H, m:m + W], cv[m + SHIFT[1]:m + SHIFT[1] + H, m + SHIFT[0]:m + SHIFT[0] + W]
    if noisy:
        cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(torch.from_numpy(np.ascontiguousarray(p)).to(dev), uv) for p in (cur, ref)]


def check_translation(H, W, B, R, dev):
    cur, ref = frames(H, W, dev, noisy=False)
    est = ingest.MotionEstimator(H, W, block=B, search=R, lam=2, intra=20, device=dev, with_sad=True)
    rec = est.estimate(cur, ref).to(torch.int64)
    x0, y0, w, h = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    inside = (x0 + SHIFT[0] >= 0) & (x0 + w + SHIFT[0] <= W) & (y0 + SHIFT[1] >= 0) & (y0 + h + SHIFT[1] <= H)
    ok = (rec[:, 4] == 4 * SHIFT[0]) & (rec[:, 5] == 4 * SHIFT[1]) & (rec[:, 6] == 0) & (est.sad == 0)
    if not bool(ok[inside].all()) or int(inside.sum()) < rec.shape[0] // 2:
        raise SystemExit(f"{H}x{W} B {B} R {R}: {int((~ok[inside]).sum())} of {int(inside.sum())} blocks did not come back with the shift and SAD 0")
    return int(inside.sum())


def case_cost(H, W, B, R, repeats, window, dev):
    recovered = check_translation(H, W, B, R, dev)
    cur, ref = frames(H, W, dev, noisy=True)
    est = ingest.MotionEstimator(H, W, block=B, search=R, lam=2, intra=20, device=dev)
    chain = ingest.MotionChain(H, W, gop=2, max_ref=1, device=dev)
    rec = est.estimate(cur, ref)
    stats = est.stats_row().tolist()

    def push():
        chain.f = 0
        chain.push(rec)

    res = alternate({"estimate": lambda: est.estimate(cur, ref), "push": push}, repeats, window)
    res = {k: {key.replace("per_gop", "per_frame"): v for key, v in r.items()} for k, r in res.items()}
    print(f"{H}x{W} B {B} R {R}: " + ", ".join(f"{k} {r['us_per_frame_median']:.1f} us ({r['us_per_frame_min']:.1f}-{r['us_per_frame_max']:.1f})"
                                                for k, r in res.items()), file=sys.stderr)
    return {"frame": [H, W], "block": B, "search": R, "blocks": est.n_blocks, "candidates_per_block": (2 * R + 1) ** 2,
            "blocks_checked_for_the_shift": recovered, "stats_intra_zero_sad_pixels": stats, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--cases", default="720x960x16,1024x2048x32", help="HxWxR, each at blocks of 16 and of 8")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "block_motion.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_motion.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "cases": []}
    for c in a.cases.split(","):
        H, W, R = (int(v) for v in c.lower().split("x"))
        for B in (16, 8):
            res["cases"].append(case_cost(H, W, B, R, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
