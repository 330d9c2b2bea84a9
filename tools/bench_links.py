#!/usr/bin/env python3
"""What linking the regions of a GOP's frames to the keyframe's regions costs on the GPU, and what the host path it replaces costs:
arseg_region_links_fwd (csrc/links.hip) behind the label plane, its run code and its regions, against pulling both run codes, run_region
and the motion field to the host and linking there.  One process, forms alternated, --repeats windows of >= --window seconds each (HIP
events on the launch stream for the GPU forms, wall time for the host forms), median and min-max; the protocol of tools/bench_regions.py.
The kernel forms are bare ABI calls on preallocated buffers.

Shapes: N = 11 (the non-keyframes of a GOP) at 720x960 and at 1024x2048.  The keyframe's mask is a blob plane of tests/rle_oracle.py
(blob_planes: 19 classes, features of about 32 pixels); the motion is synth.make_clip's (block-constant fields on a random 8..64-pixel
tiling around a pan that grows with the distance to the keyframe); the mask of frame d is the keyframe's fetched through its field, as
make_clip forms its frames.  Head logits [N,19,H/8,W/8] whose x8 argmax route gives the yardstick its labels8 launch.
Forms:
  labels8_encode_regions        arseg_segment_egress_fwd + arseg_labels_rle_fwd + arseg_rle_regions_fwd: the yardstick, the parent commit's code
  labels8_encode_regions_links  the same plus arseg_region_links_fwd against the keyframe's regions through mv_q
  links_mv / links_zero         arseg_region_links_fwd alone, with the field and with mv_q = NULL
  host_links                    to_host() of both sides + run_region and mv_q device -> host + egress.links_numpy per frame, end to end
Before anything is timed, for each shape, with and without the field: n_pairs, links and back must equal egress.links_numpy's bit for bit.
The time links add over the yardstick is set against the two min-max spreads together; the field's bytes over links_mv's time are set
against the stream-copy rate measured in the same process (arseg_peak_stream_copy, as bench.py measures it).  No ratio is fixed in advance,
and the host comparison is reported, not gated.  One JSON line on stdout, the same written to --out (default profiles/links.json)."""
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
from arseg_amd import _lib, egress, synth
from bench_regions import alternate

LINK_FIELDS, BACK_FIELDS = egress.LINK_DTYPE.names, egress.BACK_DTYPE.names


def gop_masks(N, H, W):
    """(keyframe mask uint8 [1,H,W], masks of the N frames behind it uint8 [N,H,W], mv_q int16 [N,H,W,2])."""
    key = rle_oracle.blob_planes(5, 1, H, W)
    g = synth._rng(5, f"clip{H}x{W}")
    pan = g.uniform(-3.0, 3.0, 2)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cur, mvs = np.empty((N, H, W), dtype=np.uint8), np.empty((N, H, W, 2), dtype=np.int16)
    for d in range(1, N + 1):
        mv = synth._block_mv(g, H, W, pan, d)
        mvs[d - 1] = mv
        cur[d - 1] = key[0][np.clip(yy + mv[..., 1] // 4, 0, H - 1), np.clip(xx + mv[..., 0] // 4, 0, W - 1)]
    return key, cur, mvs


def stream_copy_gbps(lib, dev, st):
    n = 256 << 20
    src, dst = torch.zeros((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev)
    best = None
    for _ in range(6):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _lib.check(lib.arseg_peak_stream_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n, st), "peak_stream_copy")
        e.record()
        e.synchronize()
        t = s.elapsed_time(e) * 1e-3
        best = t if best is None or t < best else best
    return 2.0 * n / best / 1e9


def shape_cost(N, H, W, repeats, window, dev, copy_gbps):
    lib = _lib.load()
    name = f"{N}x{H}x{W}"
    key_np, cur_np, mv_np = gop_masks(N, H, W)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    mv_q = torch.from_numpy(mv_np).to(dev)

    # ---- both sides through the host layer, with a quarter of headroom over what the sizing passes ask for
    def coded(planes):
        lab = torch.from_numpy(planes).to(dev)
        need = int(egress.rle_of_planes(lab, 0).needed().max())
        frames = egress.rle_of_planes(lab, need * 5 // 4 + 16)
        regions = int(egress.regions(frames, 0).needed().max())
        return lab, egress.regions(frames, regions * 5 // 4 + 16)

    lab, cur = coded(cur_np)
    _, key = coded(key_np)
    cap, rcap, kcap, ref_cap = cur.frames.capacity, cur.capacity, key.capacity, key.frames.capacity
    pcap = 4 * cap
    linked = egress.links(cur, key, mv_q, pair_capacity=pcap)
    ws_bytes = lib.arseg_region_links_workspace_bytes(N, pcap)

    def links(field, rs=cur.frames.row_start, nreg=cur.n_regions, rr=cur.run_region):
        def run():
            _lib.check(lib.arseg_region_links_fwd(P(rs), P(cur.frames.runs), P(nreg), P(rr), cap, P(key.frames.row_start), P(key.frames.runs),
                                                  P(key.n_regions), P(key.run_region), ref_cap, 1, P(field) if field is not None else null, N, H, W,
                                                  P(linked.n_pairs), P(linked.links), rcap, P(linked.back), kcap, pcap, P(linked.workspace),
                                                  ws_bytes, st), "links")
        return run

    # ---- correctness first: bit for bit against the host form
    cur_code, key_code = cur.frames.to_host(), key.frames.to_host()
    cur_rr, key_rr = cur.run_region.cpu().numpy(), key.run_region.cpu().numpy()
    pairs = {}
    for tag, field, field_np in (("mv", mv_q, mv_np), ("zero", None, None)):
        links(field)()
        torch.cuda.synchronize()
        got = linked.to_host()
        for n in range(N):
            want = egress.links_numpy(cur_code[n][0], cur_code[n][1], cur_rr[n], key_code[0][0], key_code[0][1], key_rr[0], H, W,
                                      None if field_np is None else field_np[n])
            for side, fields in ((0, LINK_FIELDS), (1, BACK_FIELDS)):
                if len(got[n][side]) != len(want[side]) or any(not np.array_equal(got[n][side][f], want[side][f]) for f in fields):
                    raise SystemExit(f"{name}, {tag}, frame {n}: the {'links' if side == 0 else 'back'} records differ from links_numpy's")
        pairs[tag] = linked.n_pairs.cpu().tolist()

    # ---- the chain from logits (noise logits: the yardstick's cost does not depend on the labels, so labels8 runs on the logits' plane
    # while the encoder, the regions and the links work on the GOP's masks)
    n_cls, h, w = 19, H // 8, W // 8
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, h, w)).astype(np.float32)).to(dev)
    lab8 = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    rs2, nreg2, rr2 = torch.empty_like(cur.frames.row_start), torch.empty_like(cur.n_regions), torch.empty_like(cur.run_region)
    reg_ws_bytes = lib.arseg_rle_regions_workspace_bytes(N, cap)

    def yardstick():
        _lib.check(lib.arseg_segment_egress_fwd(P(logits), N, n_cls, h, w, H, W, 0, None, P(lab8), W, H * W, 0, null, null, null, 0, 0, 0, 0, 0, 0,
                                                null, null, null, 0, 0, 0, 0, 0, 0, None, None, st), "egress")
        _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(rs2), P(cur.frames.runs), cap, st), "rle encode")
        _lib.check(lib.arseg_rle_regions_fwd(P(rs2), P(cur.frames.runs), cap, N, H, W, 8, P(nreg2), P(rr2), P(cur.records), rcap,
                                             P(cur.workspace), reg_ws_bytes, st), "regions")

    chain_links = links(mv_q, rs2, nreg2, rr2)

    def chain():
        yardstick()
        chain_links()

    pin = torch.empty((N, H, W, 2), dtype=torch.int16).pin_memory()

    def host_links():
        a, b = cur.frames.to_host(), key.frames.to_host()
        ra, rb = cur.run_region.cpu().numpy(), key.run_region.cpu().numpy()
        pin.copy_(mv_q, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        field = pin.numpy()
        for n in range(N):
            egress.links_numpy(a[n][0], a[n][1], ra[n], b[0][0], b[0][1], rb[0], H, W, field[n])

    forms = {"labels8_encode_regions": yardstick, "labels8_encode_regions_links": chain, "links_mv": links(mv_q), "links_zero": links(None),
             "host_links": host_links}
    res = alternate(forms, repeats, window)
    y, c = res["labels8_encode_regions"], res["labels8_encode_regions_links"]
    spreads = (y["us_max"] - y["us_min"]) + (c["us_max"] - c["us_min"])
    added = c["us_median"] - y["us_median"]
    field_gbps = mv_q.numel() * 2 / (res["links_mv"]["us_median"] * 1e-6) / 1e9
    verdict = {"links_add_us": added, "spreads_us": spreads, "added_beyond_spreads": bool(added > spreads),
               "links_mv_alone_us": res["links_mv"]["us_median"], "chain_over_yardstick": c["us_median"] / y["us_median"],
               "field_GBps_over_links_mv": field_gbps, "stream_copy_GBps": copy_gbps, "field_rate_over_stream_copy": field_gbps / copy_gbps,
               "host_links_over_chain": res["host_links"]["us_median"] / c["us_median"]}
    inputs = {"runs_per_frame": cur.frames.needed().cpu().tolist(), "regions_per_frame": cur.needed().cpu().tolist(),
              "keyframe_runs": key.frames.needed().cpu().tolist(), "keyframe_regions": key.needed().cpu().tolist(), "pairs_per_frame_mv": pairs["mv"],
              "pairs_per_frame_zero": pairs["zero"], "capacity": cap, "region_capacity": rcap, "pair_capacity": pcap,
              "workspace_bytes": int(ws_bytes), "mv_q_bytes": mv_q.numel() * 2}
    print(f"{name}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; pairs/frame {int(np.mean(pairs['mv']))}, field at {field_gbps:.0f} GB/s of {copy_gbps:.0f}", file=sys.stderr)
    return {"planes": [N, H, W], "inputs": inputs, "verdict": verdict, "forms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_links.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    copy_gbps = stream_copy_gbps(_lib.load(), dev, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "stream_copy_GBps": copy_gbps, "shapes": []}
    for H, W in ((720, 960), (1024, 2048)):
        res["shapes"].append(shape_cost(11, H, W, a.repeats, a.window, dev, copy_gbps))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
