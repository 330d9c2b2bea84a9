#!/usr/bin/env python3
"""What the quad-tree split of 16 x 16 block motion costs per frame, next to the estimator without it and next to estimating on blocks of 8,
and what each finds.  One process, forms alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream), median
and min-max: the protocol of tools/bench_block_motion.py.

Frames: NV12 luma on the device, a two-layer scene -- two noise canvases that meet at a vertical border in the middle of a block column, the
left sliding by (0, +3) and the right by (0, -2) per frame, +-2 of noise on every sample of the current frame -- so that one block column
straddles two motions and the split has work to do.  Before anything is timed the split's outputs on each shape are compared with
ingest.block_motion_split_numpy on the records the device's own search wrote.

Shapes: 720x960 at search 16 (full search) and 1024x2048 with levels=2 (search 8 on the top level, refine 1).  Forms per shape:
  estimate/b16        MotionEstimator(block=16).estimate: the estimator as it is without the split -- the yardstick
  estimate/b8         MotionEstimator(block=8).estimate: what a caller can do without the split
  estimate/b16+split  MotionEstimator(block=16, split_refine=2).estimate: the search and the one split launch
  push/<form>         MotionChain(track_links=True).push of that form's list: n, 4 n or 5 n records
Every form with "/graph" is the same call captured once in a HIP graph and replayed: the device's time without the host's enqueue time.
Quality, computed on the host forms on a 360x480 scene of the same kind without sensor noise: the share of pixels whose vector is exactly the
layer's true one for B = 16, B = 8 and B = 16 + split.  The synthetic scene says nothing about accuracy on real video.
One JSON line on stdout, the same written to --out (default profiles/block_motion_split.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from arseg_amd import _lib, ingest
from bench_block_motion_pyr import graphed
from bench_mv_brecords import alternate

LEFT, RIGHT = (0, 3), (0, -2)
SPLIT = dict(r=2, lam=2, intra=20, gain=32)


def planes(H, W, noisy, seed=13):
    """(cur, ref, border) uint8 [H,W]: cur[y][x] = ref[y + 3][x] left of the border and ref[y - 2][x] right of it."""
    g = np.random.Generator(np.random.PCG64(seed))
    m, border = 8, (W // 32) * 16 + 8
    a, b = (g.integers(0, 256, (H + 2 * m, W), dtype=np.uint8) for _ in range(2))
    left = np.arange(W)[None, :] < border
    ref = np.where(left, a[m:m + H], b[m:m + H])
    cur = np.where(left, a[m + LEFT[1]:m + LEFT[1] + H], b[m + RIGHT[1]:m + RIGHT[1] + H])
    if noisy:
        cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(cur), np.ascontiguousarray(ref), border


def frames(H, W, dev, noisy=True):
    cur, ref, _ = planes(H, W, noisy)
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    return [ingest.DecodedFrames.nv12(torch.from_numpy(p).to(dev), uv) for p in (cur, ref)], (cur, ref)


def estimator(H, W, dev, B, search, levels, split):
    return ingest.MotionEstimator(H, W, block=B, search=search, lam=SPLIT["lam"], intra=SPLIT["intra"], device=dev, with_sad=True, levels=levels, refine=1,
                                  split_refine=SPLIT["r"] if split else 0, split_gain=SPLIT["gain"])


def quality(H=360, W=480, R=6):
    cur, ref, border = planes(H, W, noisy=False, seed=17)
    truth = np.zeros((H, W, 2), dtype=np.int16)
    truth[:, :border], truth[:, border:] = (4 * LEFT[0], 4 * LEFT[1]), (4 * RIGHT[0], 4 * RIGHT[1])
    share = lambda rec: float(((ingest.records_to_dense(rec, H, W)[..., :2] == truth).all(axis=-1) & (ingest.records_to_dense(rec, H, W)[..., 2] == 0)).mean())
    b16 = ingest.block_motion_numpy(cur, ref, B=16, R=R, lam=SPLIT["lam"], intra=SPLIT["intra"])[0]
    b8 = ingest.block_motion_numpy(cur, ref, B=8, R=R, lam=SPLIT["lam"], intra=SPLIT["intra"])[0]
    children, _, st = ingest.block_motion_split_numpy(cur, ref, b16, SPLIT["r"], SPLIT["lam"], SPLIT["intra"], SPLIT["gain"])
    return {"frame": [H, W], "search": R, "border_x": border, "share_of_pixels_with_the_true_vector": {"b16": share(b16), "b8": share(b8),
            "b16+split": share(np.concatenate([b16, children]))}, "split_stats": [int(v) for v in st]}


def shape_cost(H, W, search, levels, repeats, window, dev):
    (cur, ref), (cur_np, ref_np) = frames(H, W, dev)
    ests = {"b16": estimator(H, W, dev, 16, search, levels, False), "b8": estimator(H, W, dev, 8, search, levels, False),
            "b16+split": estimator(H, W, dev, 16, search, levels, True)}
    sp = ests["b16+split"]
    out = sp.estimate(cur, ref)
    torch.cuda.synchronize()
    want = ingest.block_motion_split_numpy(cur_np, ref_np, sp.records.cpu().numpy(), SPLIT["r"], SPLIT["lam"], SPLIT["intra"], SPLIT["gain"])
    if not (np.array_equal(sp.children.cpu().numpy(), want[0]) and np.array_equal(sp.child_sad.cpu().numpy().view(np.uint32), want[1])
            and np.array_equal(sp.split_stats_row().cpu().numpy(), want[2]) and tuple(out.shape) == (5 * sp.n_blocks, 8)):
        raise SystemExit(f"{H}x{W}: the split's outputs differ from block_motion_split_numpy")
    forms, lists = {}, {}
    for name, est in ests.items():
        forms[f"estimate/{name}"] = lambda est=est: est.estimate(cur, ref)
        lists[name] = est.estimate(cur, ref)
    for name, rec in lists.items():
        chain = ingest.MotionChain(H, W, gop=2, max_ref=1, device=dev, track_links=True)

        def push(chain=chain, rec=rec):
            chain.f = 0
            return chain.push(rec)
        forms[f"push/{name}"] = push
    for k in list(forms):
        forms[k + "/graph"] = graphed(forms[k])
    res = alternate(forms, repeats, window)
    res = {k: {key.replace("per_gop", "per_frame"): v for key, v in r.items()} for k, r in res.items()}
    print(f"{H}x{W} search {search} levels {levels}: " + ", ".join(f"{k} {r['us_per_frame_median']:.1f} us ({r['us_per_frame_min']:.1f}-{r['us_per_frame_max']:.1f})"
                                                                  for k, r in res.items()), file=sys.stderr)
    return {"frame": [H, W], "search": search, "levels": levels, "records": {k: int(v.shape[0]) for k, v in lists.items()},
            "split_stats": [int(v) for v in want[2]], "parents": sp.n_blocks, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shapes", default="720x960x16x0,1024x2048x8x2", help="HxWxsearchxlevels")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "block_motion_split.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_motion_split.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "split": SPLIT, "quality_host": quality(), "shapes": []}
    for c in a.shapes.split(","):
        H, W, search, levels = (int(v) for v in c.lower().split("x"))
        res["shapes"].append(shape_cost(H, W, search, levels, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
