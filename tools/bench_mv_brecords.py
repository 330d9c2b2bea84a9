#!/usr/bin/env python3
"""What the two-list (B-frame) record chain costs against the P-frame chain it extends.  One process, forms alternated, --repeats windows
of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of tools/bench_mv_records.py.

Shapes: 512x1024 and 1024x2048, one GOP of 12 (11 frames pushed), records already on the device.  Forms:
  p_chain            ingest.MotionChain(bidirectional=False).push_gop on the P-only records of synth.make_record_chain: the yardstick, the
                     code this entry extends, unchanged by it, run in the same process
  bi_on_p            ingest.MotionChain(bidirectional=True).push_gop on the same P-only records, in order (one list empty)
  bi_ibbp_<policy>   the same chain on an IBBP GOP in decode order 3 1 2 6 4 5 9 7 8 11 10: P-frames reach back to the previous anchor,
                     B-frames hold 16x16 blocks of which about half are bi-predicted (list 0 to the anchor before, list 1 to the anchor
                     after), a quarter each single-list; under "list0", "near" and "mean"
p_chain and bi_on_p are compared bit for bit before anything is timed, and bi_ibbp_mean with ingest.chain_records_numpy at the first shape.
--forms limits what is timed (for a kernel trace of one form at a time; p_chain always runs, it is the yardstick of the ratios).
Per form: us per GOP and the bytes per pixel and frame its kernels must move.  One JSON line on stdout, the same written to --out (default
profiles/mv_brecords.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from arseg_amd import _lib, ingest, synth

IBBP_ORDER = (3, 1, 2, 6, 4, 5, 9, 7, 8, 11, 10)
ANCHORS = (0, 3, 6, 9, 11)
# atomic + index read + index clear per map, one gather per usable list, one store; records come on top
BYTES_PER_PIXEL = {"p_chain": 4 + 4 + 4 + 4 + 4, "bi_on_p": 4 + 2 * (4 + 4) + 4 + 4, "bi_ibbp_mean": 2 * (4 + 4 + 4) + 2 * 4 + 4}


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


def ibbp_gop(seed, H, W, bs=16):
    """[(f, int16 [n,8])] in IBBP_ORDER; returns it with the fraction of B-frame blocks that are bi-predicted."""
    g = np.random.default_rng(seed)
    hb, wb = (H + bs - 1) // bs, (W + bs - 1) // bs
    by, bx = (v.ravel() for v in np.mgrid[0:hb, 0:wb])
    n = by.size
    pushes, bi_blocks, b_blocks = [], 0, 0

    def records(f, target, lst, keep):
        r = np.zeros((n, 8), dtype=np.int16)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3] = bx * bs, by * bs, bs, bs
        r[:, 4:6] = g.integers(-70, 71, (n, 2))
        r[:, 6] = f - target - 1 if target < f else f - target
        r[:, 7] = lst
        return r[keep]

    for f in IBBP_ORDER:
        if f in ANCHORS:
            pushes.append((f, records(f, ANCHORS[ANCHORS.index(f) - 1], 0, np.ones(n, bool))))
            continue
        before, after = max(a for a in ANCHORS if a < f), min(a for a in ANCHORS if a > f)
        kind = g.choice(4, n, p=[0.5, 0.25, 0.25, 0.0])                 # 0: both lists, 1: list 0 only, 2: list 1 only
        bi_blocks, b_blocks = bi_blocks + int((kind == 0).sum()), b_blocks + n
        both = np.concatenate([records(f, before, 0, kind != 2), records(f, after, 1, kind != 1)])
        pushes.append((f, np.ascontiguousarray(both[g.permutation(both.shape[0])])))
    return pushes, bi_blocks / b_blocks


def shape_cost(H, W, repeats, window, dev, verify, only):
    F = len(IBBP_ORDER)
    p_recs = [torch.from_numpy(r).to(dev) for r in synth.make_record_chain(7, H, W, F)]
    pushes, bi_fraction = ibbp_gop(7, H, W)
    b_recs = [torch.from_numpy(r).to(dev) for _, r in pushes]
    p_chain = ingest.MotionChain(H, W, gop=F + 1, device=dev)
    bi = {pol: ingest.MotionChain(H, W, gop=F + 1, device=dev, bidirectional=True, bipred=pol) for pol in ingest.BIPRED}
    forms = {"p_chain": lambda: p_chain.push_gop(p_recs), "bi_on_p": lambda: bi["list0"].push_gop(p_recs)}
    for pol in ingest.BIPRED:
        forms["bi_ibbp_" + pol] = lambda c=bi[pol]: c.push_gop(b_recs, order=IBBP_ORDER)
    if not torch.equal(forms["p_chain"](), forms["bi_on_p"]()):
        raise SystemExit(f"{H}x{W}: the two-list chain differs from the P-frame chain on P-only records")
    if verify and not np.array_equal(forms["bi_ibbp_mean"]().cpu().numpy(), ingest.chain_records_numpy(pushes, H, W, F + 1, 3, "mean")):
        raise SystemExit(f"{H}x{W}: the two-list chain differs from chain_records_numpy on the IBBP GOP")
    res = alternate({k: fn for k, fn in forms.items() if only is None or k in only or k == "p_chain"}, repeats, window)
    for k, r in res.items():
        r["over_p_chain"] = r["us_per_gop_median"] / res["p_chain"]["us_per_gop_median"]
        if k in BYTES_PER_PIXEL:
            r["bytes_per_pixel_and_frame"] = BYTES_PER_PIXEL[k]
    print(f"{H}x{W}, {F} frames, {bi_fraction:.2f} of the B-frame blocks bi-predicted: " +
          ", ".join(f"{k} {r['us_per_gop_median']:.1f} us ({r['us_per_gop_min']:.1f}-{r['us_per_gop_max']:.1f})" for k, r in res.items()), file=sys.stderr)
    return {"frame": [H, W], "frames_pushed": F, "decode_order": list(IBBP_ORDER), "bi_fraction_of_b_blocks": bi_fraction,
            "p_records_per_frame": [int(r.shape[0]) for r in p_recs], "ibbp_records_per_frame": [int(r.shape[0]) for r in b_recs],
            "bi_on_p_equals_p_chain": True, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", default="512x1024,1024x2048")
    ap.add_argument("--forms", default=None, help="comma-separated subset of the forms to time")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mv_brecords.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_brecords.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for i, s in enumerate(a.shapes.split(",")):
        H, W = (int(v) for v in s.lower().split("x"))
        res["shapes"].append(shape_cost(H, W, a.repeats, a.window, dev, verify=i == 0, only=a.forms.split(",") if a.forms else None))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
