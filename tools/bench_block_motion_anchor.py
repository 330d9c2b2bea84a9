#!/usr/bin/env python3
"""What keyframe anchoring costs per frame next to the hierarchical search it follows, and what it buys over a GOP.  One process, forms
alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max: the protocol of
tools/bench_block_motion_pyr.py.

Content: a GOP of 12 NV12 frames cut from one noise canvas, panned by (3, -2) per frame, +-2 of noise on every sample of every frame but
the keyframe.  Cases: 720x960 and 1024x2048, blocks of 16 and of 8, anchor radius r = 1, 2, 3.  The hop search is
MotionEstimator(levels=2, search=4, refine=1) (reach 19), the chain MotionChain(gop=12, max_ref=16).  Forms per case, timed at frame 6 of the
GOP (the chain holds frames 1 .. 5), all in the same process:
  pyr_search             MotionEstimator.estimate on two built pyramids: the 3 launches of arseg_block_motion_pyr_fwd
  anchor/r               the one launch of arseg_block_motion_anchor_fwd on level 0 of the two pyramids, records and merged[5] given
  estimate_anchored/r    MotionEstimator.estimate_anchored on two built pyramids: the search and the anchor
Every form with "/graph" is the same call captured once in a HIP graph and replayed: the device's time without the host's enqueue time.
Quality per r: the share of interior blocks (whole blocks whose position displaced by 11 (3, -2) lies inside the keyframe) all of whose
pixels carry exactly the true displacement in mv_q of frame 11, plain pushes against anchored pushes, and the anchor counts over the GOP.
One JSON line on stdout, the same written to --out (default profiles/block_motion_anchor.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from arseg_amd import _lib, ingest, ops
from bench_block_motion_pyr import graphed
from bench_mv_brecords import alternate

PAN, GOP, AT = (3, -2), 12, 6
LEVELS, SEARCH, REFINE, LAM, INTRA = 2, 4, 1, 2, 20


def gop_frames(H, W, dev):
    g = np.random.Generator(np.random.PCG64(13))
    m = 3 * GOP + 4
    cv = g.integers(0, 256, (H + 2 * m, W + 2 * m), dtype=np.uint8)
    uv = torch.zeros((H // 2, W // 2, 2), dtype=torch.uint8, device=dev)
    out = []
    for f in range(GOP):
        p = cv[m + PAN[1] * f:m + PAN[1] * f + H, m + PAN[0] * f:m + PAN[0] * f + W]
        if f:
            p = np.clip(p.astype(np.int64) + g.integers(-2, 3, p.shape), 0, 255).astype(np.uint8)
        out.append(ingest.DecodedFrames.nv12(torch.from_numpy(np.ascontiguousarray(p)).to(dev), uv))
    return out


def estimator(H, W, B, dev, r):
    return ingest.MotionEstimator(H, W, block=B, search=SEARCH, lam=LAM, intra=INTRA, device=dev, levels=LEVELS, refine=REFINE, anchor_refine=r, anchor_intra=INTRA)


def run_gop(est, chain, pyr, upto, anchored):
    chain.reset()
    est.reset_stats()
    if anchored:
        est.set_key(pyr[0])
    for f in range(1, upto + 1):
        chain.push(est.estimate_anchored(pyr[f], pyr[f - 1], chain) if anchored else est.estimate(pyr[f], pyr[f - 1]))


def share_exact(mv, H, W, B, f):
    """Of the whole blocks whose position displaced by f PAN lies inside the keyframe: the share all of whose pixels carry 4 f PAN."""
    by, bx = H // B, W // B
    ok = (mv[:by * B, :bx * B] == torch.tensor([4 * f * PAN[0], 4 * f * PAN[1]], dtype=mv.dtype, device=mv.device)).all(dim=-1)
    ok = ok.reshape(by, B, bx, B).all(dim=3).all(dim=1)
    y0, x0 = torch.arange(by, device=mv.device)[:, None] * B, torch.arange(bx, device=mv.device)[None, :] * B
    inside = (x0 + f * PAN[0] >= 0) & (x0 + B + f * PAN[0] <= W) & (y0 + f * PAN[1] >= 0) & (y0 + B + f * PAN[1] <= H)
    return int(inside.sum()), float(ok[inside].float().mean())


def case_cost(H, W, B, radii, repeats, window, dev):
    frames = gop_frames(H, W, dev)
    pyr = [ingest.LumaPyramid(H, W, LEVELS, dev).build(f) for f in frames]
    chain = ingest.MotionChain(H, W, gop=GOP, max_ref=16, device=dev, track_links=True)
    info = {}
    plain = estimator(H, W, B, dev, 0)
    run_gop(plain, chain, pyr, GOP - 1, False)
    interior, plain_share = share_exact(chain.merged[GOP - 1], H, W, B, GOP - 1)
    plain_flagged = int(chain.link_stats()[GOP - 1][3])
    forms = {"pyr_search": lambda: plain.estimate(pyr[AT], pyr[AT - 1])}
    forms["pyr_search/graph"] = graphed(forms["pyr_search"])
    keep = []
    for r in radii:
        est = estimator(H, W, B, dev, r)
        run_gop(est, chain, pyr, GOP - 1, True)
        _, share = share_exact(chain.merged[GOP - 1], H, W, B, GOP - 1)
        st = est.anchor_stats_row().tolist()
        info[str(r)] = {"interior_blocks": interior, "share_exact_plain": plain_share, "share_exact_anchored": share, "flagged_pixels_plain": plain_flagged,
                        "flagged_pixels_anchored": int(chain.link_stats()[GOP - 1][3]),
                        "anchor_stats_over_the_gop": {"anchored": st[0], "healed": st[1], "kept": st[2], "drift_px": st[3], "blocks": est.n_blocks * (GOP - 1)}}
        # the state at frame AT: its own chain, so that the forms of every r read what their own GOP left
        ch = ingest.MotionChain(H, W, gop=GOP, max_ref=16, device=dev)
        run_gop(est, ch, pyr, AT - 1, True)
        hops = est.estimate(pyr[AT], pyr[AT - 1]).clone()
        out, stats = torch.zeros_like(hops), torch.zeros(_lib.BMA_NSTATS, dtype=torch.int64, device=dev)
        cur0, key0, mp = pyr[AT].level(0), pyr[0].level(0), ch.merged[AT - 1]
        keep.append((est, ch, hops, out, stats))
        forms[f"anchor/{r}"] = lambda r=r, hops=hops, out=out, stats=stats, cur0=cur0, key0=key0, mp=mp: ops.block_motion_anchor(
            cur0, key0, hops, mp, AT, B, r, LAM, INTRA, out=out, sad=False, stats=stats)
        forms[f"estimate_anchored/{r}"] = lambda est=est, ch=ch: est.estimate_anchored(pyr[AT], pyr[AT - 1], ch)
        forms[f"anchor/{r}/graph"] = graphed(forms[f"anchor/{r}"])
        forms[f"estimate_anchored/{r}/graph"] = graphed(forms[f"estimate_anchored/{r}"])
    res = alternate(forms, repeats, window)
    res = {k: {key.replace("per_gop", "per_frame"): v for key, v in r.items()} for k, r in res.items()}
    print(f"{H}x{W} B {B}: " + ", ".join(f"{k} {r['us_per_frame_median']:.1f} us ({r['us_per_frame_min']:.1f}-{r['us_per_frame_max']:.1f})" for k, r in res.items()),
          file=sys.stderr)
    print(f"{H}x{W} B {B}: " + ", ".join(f"r {r}: exact {v['share_exact_plain']:.4f} -> {v['share_exact_anchored']:.4f}" for r, v in info.items()), file=sys.stderr)
    return {"frame": [H, W], "block": B, "blocks": plain.n_blocks, "quality": info, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--cases", default="720x960,1024x2048", help="HxW, each at blocks of 16 and of 8")
    ap.add_argument("--radii", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "block_motion_anchor.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_motion_anchor.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    radii = [int(v) for v in a.radii.split(",")]
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "pan": list(PAN), "gop": GOP, "timed_at_frame": AT,
           "hop_search": {"levels": LEVELS, "search_top": SEARCH, "refine": REFINE, "lam": LAM, "intra": INTRA}, "cases": []}
    for c in a.cases.split(","):
        H, W = (int(v) for v in c.lower().split("x"))
        for B in (16, 8):
            res["cases"].append(case_cost(H, W, B, radii, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
