#!/usr/bin/env python3
"""What the hierarchical block search costs per frame next to the full search, and what it finds.  One process, forms alternated, --repeats
windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of tools/bench_block_motion.py,
whose frames these are: NV12 luma on the device, the current frame a window of the reference's noise canvas moved by (5, -3), with +-2 of
noise on every sample where it is timed.

Cases: the four of tools/bench_block_motion.py -- 720x960 at search 16 and 1024x2048 at search 32, blocks of 16 and of 8 -- each with the
hierarchical configurations of --configs beside it (levels:Rt:r; the defaults have a reach just above the full search's, and 1024x2048 also
one of 67).  Forms per case, all timed in the same process:
  full             MotionEstimator.estimate, the one launch of arseg_block_motion_fwd
  pyr_build        LumaPyramid.build of one frame: the one launch of arseg_luma_pyramid_fwd
  pyr_search/<c>   MotionEstimator(levels=L).estimate on two built pyramids: the L + 1 launches of arseg_block_motion_pyr_fwd
  pyr_estimate/<c> the same on two frames: two builds and the search (what a caller pays who keeps no pyramids)
Quality per configuration, on the noise-free and on the noisy pair: the share of blocks whose record equals the full search's, and the sum of
the winners' SAD over the full search's; and on the noise-free pair how many of the whole blocks whose level-L ancestor, moved by the shift,
lies inside the frame came back with exactly the shift and SAD 0.  Every form with "/graph" is the same call captured once in a HIP graph and
replayed: the device's time without the host's enqueue time, which is what counts inside a captured GOP graph.
One JSON line on stdout, the same written to --out (default profiles/block_motion_pyr.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from arseg_amd import _lib, ingest
from bench_block_motion import SHIFT, frames
from bench_mv_brecords import alternate

DEFAULT_CONFIGS = {16: ["2:4:1"], 32: ["2:8:1", "2:16:1"]}          # by the full search's radius


def estimator(H, W, B, dev, R=None, cfg=None):
    if cfg is None:
        return ingest.MotionEstimator(H, W, block=B, search=R, lam=2, intra=20, device=dev, with_sad=True)
    L, Rt, r = cfg
    return ingest.MotionEstimator(H, W, block=B, search=Rt, lam=2, intra=20, device=dev, with_sad=True, levels=L, refine=r)


def check_translation(H, W, B, cfg, dev):
    """(interior blocks, how many came back with the shift and SAD 0) on the noise-free pair.  Reported, not required: recovery is a property
    of the input, and box-filtered white noise half a pixel out of phase barely correlates on blocks of 8."""
    cur, ref = frames(H, W, dev, noisy=False)
    est = estimator(H, W, B, dev, cfg=cfg)
    rec = est.estimate(cur, ref).to(torch.int64)
    S = B << cfg[0]
    x0, y0, w, h = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    ax, ay = x0 // S * S, y0 // S * S
    inside = (w == B) & (h == B) & (ax + SHIFT[0] >= 0) & (ax + S + SHIFT[0] <= W) & (ay + SHIFT[1] >= 0) & (ay + S + SHIFT[1] <= H)
    ok = (rec[:, 4] == 4 * SHIFT[0]) & (rec[:, 5] == 4 * SHIFT[1]) & (rec[:, 6] == 0) & (est.sad == 0)
    return int(inside.sum()), int(ok[inside].sum())


def graphed(fn):
    """fn captured once in a HIP graph: the replay is what a caller of the captured GOP graph pays, without the host's enqueue time."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def quality(H, W, B, R, cfg, dev):
    out = {}
    for name, noisy in (("noise_free", False), ("noisy", True)):
        cur, ref = frames(H, W, dev, noisy=noisy)
        full, hier = estimator(H, W, B, dev, R=R), estimator(H, W, B, dev, cfg=cfg)
        fr, hr = full.estimate(cur, ref).clone(), hier.estimate(cur, ref).clone()
        fs, hs = int(full.sad.to(torch.int64).sum()), int(hier.sad.to(torch.int64).sum())
        out[name] = {"blocks_equal_to_full": float((fr == hr).all(dim=1).float().mean()), "sad_sum_full": fs, "sad_sum_pyr": hs,
                     "sad_ratio": hs / fs if fs else (1.0 if hs == 0 else float("inf")), "intra_full": int(full.stats_row()[0]), "intra_pyr": int(hier.stats_row()[0])}
    return out


def case_cost(H, W, B, R, configs, repeats, window, dev):
    cur, ref = frames(H, W, dev, noisy=True)
    full = estimator(H, W, B, dev, R=R)
    forms, info = {"full": lambda: full.estimate(cur, ref)}, {}
    forms["full/graph"] = graphed(forms["full"])
    for text in configs:
        cfg = tuple(int(v) for v in text.split(":"))
        interior, recovered = check_translation(H, W, B, cfg, dev)
        est = estimator(H, W, B, dev, cfg=cfg)
        pa, pb = ingest.LumaPyramid(H, W, cfg[0], dev).build(cur), ingest.LumaPyramid(H, W, cfg[0], dev).build(ref)
        if "pyr_build" not in forms:
            forms["pyr_build"] = lambda pa=pa: pa.build(cur)
        forms[f"pyr_search/{text}"] = lambda est=est, pa=pa, pb=pb: est.estimate(pa, pb)
        forms[f"pyr_estimate/{text}"] = lambda est=est: est.estimate(cur, ref)
        forms[f"pyr_search/{text}/graph"] = graphed(forms[f"pyr_search/{text}"])
        forms[f"pyr_estimate/{text}/graph"] = graphed(forms[f"pyr_estimate/{text}"])
        info[text] = {"levels": cfg[0], "search_top": cfg[1], "refine": cfg[2], "reach": est.reach, "interior_blocks": interior, "interior_blocks_with_the_shift_and_sad_0": recovered,
                      "quality_vs_full": quality(H, W, B, R, cfg, dev)}
    res = alternate(forms, repeats, window)
    res = {k: {key.replace("per_gop", "per_frame"): v for key, v in r.items()} for k, r in res.items()}
    print(f"{H}x{W} B {B} R {R}: " + ", ".join(f"{k} {r['us_per_frame_median']:.1f} us ({r['us_per_frame_min']:.1f}-{r['us_per_frame_max']:.1f})"
                                                for k, r in res.items()), file=sys.stderr)
    return {"frame": [H, W], "block": B, "search_full": R, "blocks": full.n_blocks, "configs": info, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--cases", default="720x960x16,1024x2048x32", help="HxWxR, each at blocks of 16 and of 8")
    ap.add_argument("--configs", default="", help="levels:Rt:r[,levels:Rt:r ...] for every case; default: a reach just above R, and 67 beside R = 32")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "block_motion_pyr.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_motion_pyr.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shift": list(SHIFT), "cases": []}
    for c in a.cases.split(","):
        H, W, R = (int(v) for v in c.lower().split("x"))
        configs = a.configs.split(",") if a.configs else DEFAULT_CONFIGS.get(R, [f"2:{max(1, -(-R // 4))}:1"])
        for B in (16, 8):
            res["cases"].append(case_cost(H, W, B, R, configs, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
