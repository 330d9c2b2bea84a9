#!/usr/bin/env python3
"""What the link bytes cost the motion chain.  One process, forms alternated, --repeats windows of >= --window seconds each (HIP events on
the launch stream), median and min-max; the protocol of tools/bench_mv_records.py.

Shapes: 512x1024 and 1024x2048, one GOP of 12 (11 frames pushed), records already on the device; the records and the IBBP GOP are those of
tools/bench_mv_brecords.py, so the forms without links repeat what profiles/mv_brecords.json holds.  Forms:
  p_chain            ingest.MotionChain().push_gop on the P-only records of synth.make_record_chain: the yardstick, the parent's code path
                     (the LINK = false instantiations), run in the same process
  p_chain_link       the same with track_links=True: one more launch per GOP (arseg_mv_link_reset), the LINK = true compose kernel
  ibbp_list0         MotionChain(bidirectional=True, bipred="list0") on the IBBP GOP in decode order 3 1 2 6 4 5 9 7 8 11 10
  ibbp_list0_link    the same with track_links=True
Before anything is timed: merged of each linked form torch.equal to its plain form, link and link_stats equal to
ingest.chain_records_numpy(return_link=True) at the first shape, link_stats equal to the counts of the link planes at every shape.
Per form: us per GOP, the ratio to its plain form next to the ratio of the bytes per pixel and frame the kernels must move (P step: 4 atomic
+ 4 index read + 4 index clear + 4 gather + 4 store = 20, + 1 link gather + 1 link store = 22), and where the plain form stands against the
min-max spread profiles/mv_brecords.json records for it.  One JSON line on stdout, the same written to --out (default profiles/mv_link.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from arseg_amd import _lib, ingest, synth
from bench_mv_brecords import IBBP_ORDER, alternate, ibbp_gop

BYTES_PER_PIXEL = {"p_chain": 20, "p_chain_link": 22, "ibbp_list0": 28, "ibbp_list0_link": 30}          # two maps: 12 + 8 more; one gather under list0
PLAIN_OF = {"p_chain_link": "p_chain", "ibbp_list0_link": "ibbp_list0"}
PARENT_FORM = {"p_chain": "p_chain", "ibbp_list0": "bi_ibbp_list0"}                                       # the names in profiles/mv_brecords.json


def counts_of(link):
    """link uint8 [gop,H,W] on the device -> int64 [gop, LINK_NSTATS] computed from the planes with torch (verification only)."""
    flat = link.reshape(link.shape[0], -1).to(torch.int64)
    cols = [((flat >> b) & 1).sum(dim=1) for b in range(3)] + [((flat & 7) != 0).sum(dim=1)] + [((flat >> 4) == h).sum(dim=1) for h in range(16)]
    out = torch.stack(cols, dim=1)
    out[0] = 0                                                           # row 0 is never added to
    return out


def shape_cost(H, W, repeats, window, dev, verify, parent):
    F = len(IBBP_ORDER)
    p_host = synth.make_record_chain(7, H, W, F)
    pushes, bi_fraction = ibbp_gop(7, H, W)
    p_recs = [torch.from_numpy(r).to(dev) for r in p_host]
    b_recs = [torch.from_numpy(r).to(dev) for _, r in pushes]
    chains = {"p_chain": ingest.MotionChain(H, W, gop=F + 1, device=dev),
              "p_chain_link": ingest.MotionChain(H, W, gop=F + 1, device=dev, track_links=True),
              "ibbp_list0": ingest.MotionChain(H, W, gop=F + 1, device=dev, bidirectional=True),
              "ibbp_list0_link": ingest.MotionChain(H, W, gop=F + 1, device=dev, bidirectional=True, track_links=True)}
    forms = {k: (lambda c=c: c.push_gop(p_recs)) if k.startswith("p_") else (lambda c=c: c.push_gop(b_recs, order=IBBP_ORDER)) for k, c in chains.items()}
    flagged = {}
    for linked, plain in PLAIN_OF.items():
        if not torch.equal(forms[linked](), forms[plain]()):
            raise SystemExit(f"{H}x{W}: {linked} leaves another merged than {plain}")
        c = chains[linked]
        if not torch.equal(c.link_stats(), counts_of(c.link())):
            raise SystemExit(f"{H}x{W}: {linked}: link_stats are not the counts of the link planes")
        if verify:
            host = list(enumerate(p_host, start=1)) if plain == "p_chain" else pushes
            _, want = ingest.chain_records_numpy(host, H, W, F + 1, 3, "list0", return_link=True)
            if not np.array_equal(c.link().cpu().numpy(), want):
                raise SystemExit(f"{H}x{W}: {linked}: link differs from chain_records_numpy")
        flagged[linked] = (c.link_stats()[1:, :4].double() / (H * W)).mean(dim=0).tolist()
    res = alternate(forms, repeats, window)
    for k, r in res.items():
        r["bytes_per_pixel_and_frame"] = BYTES_PER_PIXEL[k]
        if k in PLAIN_OF:
            r["over_plain"] = r["us_per_gop_median"] / res[PLAIN_OF[k]]["us_per_gop_median"]
            r["bytes_over_plain"] = BYTES_PER_PIXEL[k] / BYTES_PER_PIXEL[PLAIN_OF[k]]
            r["mean_share_intra_uncovered_clamped_any"] = flagged[k]
        elif parent is not None and PARENT_FORM[k] in parent:
            was = parent[PARENT_FORM[k]]
            r["parent"] = {key: was[key] for key in ("us_per_gop_median", "us_per_gop_min", "us_per_gop_max")}
            r["over_parent_median"] = r["us_per_gop_median"] / was["us_per_gop_median"]
            r["median_inside_parent_min_max"] = bool(was["us_per_gop_min"] <= r["us_per_gop_median"] <= was["us_per_gop_max"])
    print(f"{H}x{W}, {F} frames: " + ", ".join(f"{k} {r['us_per_gop_median']:.1f} us ({r['us_per_gop_min']:.1f}-{r['us_per_gop_max']:.1f})" for k, r in res.items()),
          file=sys.stderr)
    return {"frame": [H, W], "frames_pushed": F, "decode_order": list(IBBP_ORDER), "bi_fraction_of_b_blocks": bi_fraction,
            "merged_equal_with_and_without_links": True, "link_stats_equal_plane_counts": True, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", default="512x1024,1024x2048")
    ap.add_argument("--parent", default=os.path.join(root, "profiles", "mv_brecords.json"), help="the recorded profile the plain forms are held against")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mv_link.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_link.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    parent = {}
    if os.path.exists(a.parent):
        with open(a.parent) as f:
            parent = {tuple(s["frame"]): s["forms"] for s in json.load(f)["shapes"]}
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for i, s in enumerate(a.shapes.split(",")):
        H, W = (int(v) for v in s.lower().split("x"))
        res["shapes"].append(shape_cost(H, W, a.repeats, a.window, dev, verify=i == 0, parent=parent.get((H, W))))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
