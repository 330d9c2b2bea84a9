#!/usr/bin/env python3
"""What the keyframe prior costs: the stabilise launch (csrc/stabilise.hip) against the consistency launch it shares its thread mapping
with, and against the same result composed in torch, on the same logits, reference plane and motion field.  One process, forms alternated,
--repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of
tools/bench_confidence.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: the four of tools/bench_egress.py -- CamVid PSPNet's tail (12 classes, 512x1024 logits at label size: the same-size route) and
BiSeNet's (19 classes, 128x256 head logits -> 1024x2048: the x8 run route), each for the 11 non-keyframes of a GOP and for one keyframe.
The reference plane is the tail's own pred of frame 0 displaced by (3, -5) pixels with a void rectangle; mv_q is constant over 16x16
blocks and points back, except in a fifth of the blocks (wrong by several pixels) and in the top block row (off the frame); a tenth of
the blocks is flagged in the link plane; the reference's confidence codes are uniform in 100..255 and the gate is at 128; beta = 1.
Forms:
  consistency        arseg_segment_consistency_fwd: labels8 + change8 + stats, the yardstick (the parent's kernel; it reads neither the link
                     plane nor the confidence plane)
  stab_labels_hold_stats   arseg_segment_stabilise_fwd: labels8 + hold8 + stats, both gates on
  stab_labels        arseg_segment_stabilise_fwd: labels8 alone, both gates on
  torch              interpolate -> max -> index arithmetic -> gathers -> compares -> where: what a caller would build today (fp32, allocating;
                     writes and re-reads the full-resolution logits)
Before anything is timed, on frame 0 of each shape, the comparison rule of tests/stabilise_oracle.py: with k* the tail's pred every fused
label is k* or c_ref; the HELD / OWN decision equals a float64 torch composition's wherever |d64 - beta| > 2e-5 (everywhere on the
same-size route, where d is an exact fp32 subtraction); at most 0.5 % of the pixels lie inside that band; the statistics are what the two
planes say.  One JSON line on stdout, the same written to --out (default profiles/stabilise.json)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from arseg_amd import _lib
from bench_confidence import alternate

BAND, BAND_CAP, LINK_MASK, REF_LOW, BLOCK = 2e-5, 0.005, _lib.LINK_INTRA | _lib.LINK_UNCOVERED, 128, 16


def torch_form(logits, ref, mv, beta, link, conf, H, W, align, dtype=torch.float32, k=None):
    """(labels uint8 [N,H,W], held bool, differing-with-a-prior bool, d, k int64) composed from torch ops; ref / conf [1,H,W].  ``k``: decide
    on these classes instead of the composition's own argmax (the check: the tail's pred)."""
    N, n_cls = logits.shape[:2]
    x = logits.to(dtype)
    if tuple(x.shape[-2:]) != (H, W):
        x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align))
    if k is None:
        m, k = x.max(dim=1)
    else:
        m = x.gather(1, k[:, None])[:, 0]
    ys, xs = torch.meshgrid(torch.arange(H, device=x.device), torch.arange(W, device=x.device), indexing="ij")
    q = torch.round(mv.to(torch.float32) / 4.0).long()                      # halves to even, exact on quarters
    tx, ty = xs[None] + q[..., 0], ys[None] + q[..., 1]
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    at = (ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)).reshape(N, -1)
    c = ref.reshape(1, -1).expand(N, -1).gather(1, at).reshape(N, H, W).long()
    cq = conf.reshape(1, -1).expand(N, -1).gather(1, at).reshape(N, H, W)
    prior = inside & (c < n_cls) & ((link & LINK_MASK) == 0) & (cq >= REF_LOW)
    d = m - x.gather(1, c.clamp(max=n_cls - 1)[:, None])[:, 0]
    differ = prior & (c != k)
    held = differ & (d < beta.to(dtype)[:, None, None])
    return torch.where(held, c, k).to(torch.uint8), held, differ, d, k


def shape_cost(N, n_cls, h, w, H, W, align, repeats, window, dev):
    lib = _lib.load()
    g = np.random.Generator(np.random.PCG64(5))
    logits = torch.from_numpy(np.clip(g.standard_normal((N, n_cls, h, w)) * 3.0, -8.0, 8.0).astype(np.float32)).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    al = 1 if align else 0
    pred = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    _lib.check(lib.arseg_argmax_confusion_fwd(P(logits), null, P(pred), null, N, n_cls, h, w, H, W, 255, al, st), "tail")
    ref = torch.roll(pred[0:1], shifts=(3, -5), dims=(1, 2)).to(torch.uint8).contiguous()
    ref[0, H // 4:H // 4 + H // 8, W // 3:W // 3 + W // 6] = 255
    by, bx = H // BLOCK, W // BLOCK
    blocks = np.tile(np.array([-20, 12], dtype=np.int16), (N, by, bx, 1))                 # points back: round(-20 / 4) = -5, 12 / 4 = 3
    blocks[g.random((N, by, bx)) < 0.2] = (-46, 30)                                       # -11.5 -> -12, 7.5 -> 8
    blocks[:, 0] = (0, -4 * BLOCK - 2)                                                    # the top block row leaves the frame
    mv = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(blocks, BLOCK, axis=1), BLOCK, axis=2))).to(dev)
    flags = np.where(g.random((N, by, bx)) < 0.1, _lib.LINK_UNCOVERED, 0).astype(np.uint8) | 0x30
    link = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(flags, BLOCK, axis=1), BLOCK, axis=2))).to(dev)
    conf = torch.from_numpy(g.integers(100, 256, (1, H, W)).astype(np.uint8)).to(dev)
    beta = torch.ones((N,), dtype=torch.float32, device=dev)
    lab, plane = torch.empty((N, H, W), dtype=torch.uint8, device=dev), torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    tc_stats = torch.zeros((N, _lib.TC_NSTATS), dtype=torch.int64, device=dev)
    st_stats = torch.zeros((N, _lib.ST_NSTATS), dtype=torch.int64, device=dev)

    def consistency():
        _lib.check(lib.arseg_segment_consistency_fwd(P(logits), N, n_cls, h, w, H, W, al, P(ref), W, 0, P(mv), None, P(lab), W, H * W, P(plane), W,
                                                     H * W, P(tc_stats), st), "consistency")

    def stab(full):
        def run():
            hold, stats = (P(plane), P(st_stats)) if full else (null, null)
            _lib.check(lib.arseg_segment_stabilise_fwd(P(logits), N, n_cls, h, w, H, W, al, P(ref), W, 0, P(mv), P(beta), P(link), W, H * W, LINK_MASK,
                                                       P(conf), W, 0, REF_LOW, None, P(lab), W, H * W, hold, W, H * W, stats, st), "stabilise")
        return run

    forms = {"consistency": consistency, "stab_labels_hold_stats": stab(True), "stab_labels": stab(False),
             "torch": lambda: torch_form(logits, ref, mv, beta, link, conf, H, W, align)}

    # ---- correctness first
    name = f"{N}x{n_cls}x{h}x{w} -> {H}x{W}"
    forms["stab_labels_hold_stats"]()
    torch.cuda.synchronize()
    same = (h, w) == (H, W)
    k = pred[0:1].long()
    _, held, differ, d, _ = torch_form(logits[0:1], ref, mv[0:1], beta[0:1], link[0:1], conf, H, W, align, torch.float32 if same else torch.float64, k)
    band = differ & ((d - 1.0).abs() <= BAND) if not same else torch.zeros_like(differ)
    got_held = plane[0:1] == 255
    c_ref = torch.where(got_held, lab[0:1].long(), k)
    check = {"band_share": float(band.double().mean()), "held": int(got_held.sum()), "differing_with_prior": int(differ.sum()),
             "decided_differently_outside_band": int(((got_held != held) & ~band).sum()),
             "decided_differently_inside_band": int(((got_held != held) & band).sum()),
             "labels_neither_kstar_nor_cref": int(((lab[0:1].long() != k) & ~got_held).sum())}
    want = torch.zeros((_lib.ST_NSTATS,), dtype=torch.int64, device=dev)
    want[4], want[5], want[6] = int((plane[0] == 0).sum()), int(got_held.sum()), int((plane[0] == 192).sum())
    want[8:8 + n_cls] = torch.bincount(c_ref[got_held], minlength=n_cls)
    want[40:40 + n_cls] = torch.bincount(k[got_held], minlength=n_cls)
    row = st_stats[0].clone()
    check["stats_equal_planes"] = bool(torch.equal(row[4:], want[4:]) and int(row[:4].sum()) == int((plane[0] == 128).sum()) and int(row[:7].sum()) == H * W)
    if check["decided_differently_outside_band"] or check["labels_neither_kstar_nor_cref"] or check["band_share"] > BAND_CAP or \
            not check["stats_equal_planes"] or not check["held"]:
        raise SystemExit(f"{name}: the kernel misses the comparison rule: {check}")
    labels32 = torch_form(logits[0:1], ref, mv[0:1], beta[0:1], link[0:1], conf, H, W, align)[0]
    check["torch_fp32_differing_labels"] = int((labels32 != lab[0:1]).sum())
    del held, differ, d, band, labels32
    st_stats.zero_()

    res = alternate(forms, repeats, window)
    lo, px = logits.numel() * 4, N * H * W
    needed = {"consistency": lo + (4 + 1 + 2) * px, "stab_labels_hold_stats": lo + (4 + 1 + 1 + 1 + 2) * px, "stab_labels": lo + (4 + 1 + 1 + 1 + 1) * px}
    base = res["consistency"]
    spread = (base["us_max"] - base["us_min"]) / base["us_median"]
    for key, r in res.items():
        r["time_over_consistency"] = r["us_median"] / base["us_median"]
        if key in needed:
            r["bytes_needed"] = needed[key]
            r["GBps"] = needed[key] / (r["us_median"] * 1e-6) / 1e9
    print(f"{name}: " + ", ".join(f"{key} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for key, r in res.items()) +
          f"; consistency spread {100 * spread:.1f}%", file=sys.stderr)
    return {"logits": [N, n_cls, h, w], "labels": [H, W], "align_corners": bool(align), "beta": 1.0, "ref_low": REF_LOW, "link_mask": LINK_MASK,
            "consistency_spread": spread, "check_frame0": check, "forms": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "stabilise.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stabilise.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    for N in (11, 1):
        res["shapes"].append(shape_cost(N, 12, 512, 1024, 512, 1024, True, a.repeats, a.window, dev))
        res["shapes"].append(shape_cost(N, 19, 128, 256, 1024, 2048, False, a.repeats, a.window, dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
