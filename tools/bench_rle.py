#!/usr/bin/env python3
"""What run-length coded masks cost and save: the encoder and decoder of csrc/rle.hip against the egress launch that writes the label plane
alone, against the same code composed in torch, and the device -> pinned-host copy of the runs against the copy of the plane.  One process,
forms alternated, --repeats windows of >= --window seconds each (HIP events on the launch stream), median and min-max; the protocol of
tools/bench_consistency.py.  The kernel forms are bare ABI calls on preallocated buffers.

Shapes: an N = 11 batch (the non-keyframes of a GOP) at 720x960 (12 classes, logits at label size: the same-size route) and at 1024x2048
(19 classes, 128x256 head logits: the x8 run route).  The logits are blob-like: low-resolution noise (one scene per batch plus a little
noise per frame, features of about 32 output pixels) resized up, as tests/consistency_oracle.py builds its scenes.
Forms:
  labels8          arseg_segment_egress_fwd, the uint8 label plane only: the yardstick
  labels8_encode   labels8, then arseg_labels_rle_fwd on that plane
  encode           arseg_labels_rle_fwd alone (count, scan, emit)
  decode           arseg_rle_decode_fwd
  torch            per-row diff -> nonzero -> gather, cumsum of the counts: what a caller would compose today (allocating; nonzero
                   synchronises with the host)
  copy_plane       the plane, device -> pinned host
  copy_runs        row_start[:, H] device -> pinned host, a synchronise, then runs[:, :max needed] device -> pinned host
  e2e_plane        labels8 + copy_plane          e2e_runs    labels8_encode + copy_runs
  stream_copy      arseg_peak_stream_copy over 256 MiB: the on-box bandwidth yardstick
Before anything is timed, for each shape: row_start and the runs of the encoder must equal the torch composition bit for bit, and the decoder
must give the plane back.  One JSON line on stdout, the same written to --out (default profiles/rle.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from arseg_amd import _lib


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
    return {k: {"us_median": 1e3 * statistics.median(v), "us_min": 1e3 * min(v), "us_max": 1e3 * max(v)} for k, v in ms.items()}


def blob_logits(g, N, n_cls, h, w, cell, dev):
    """fp32 logits [N,n_cls,h,w] with |x| <= 8 whose argmax forms regions of about ``cell`` logit pixels."""
    gh, gw = max(2, h // cell), max(2, w // cell)
    base = g.standard_normal((n_cls, gh, gw))
    noise = torch.from_numpy((base[None] + 0.3 * g.standard_normal((N, n_cls, gh, gw))).astype(np.float32)).to(dev)
    return torch.clamp(3.0 * F.interpolate(noise, size=(h, w), mode="bilinear", align_corners=True), -8.0, 8.0).contiguous()


def torch_form(plane):
    """(row_start int64 [N,H+1], the words of all frames in (n, y, x) order, int64) composed from torch ops."""
    N, H, W = plane.shape
    start = torch.ones((N, H, W), dtype=torch.bool, device=plane.device)
    start[:, :, 1:] = plane[:, :, 1:] != plane[:, :, :-1]
    row_start = torch.zeros((N, H + 1), dtype=torch.int64, device=plane.device)
    row_start[:, 1:] = start.sum(dim=2).cumsum(dim=1)
    idx = start.nonzero()
    words = (idx[:, 2] << 8) | plane[idx[:, 0], idx[:, 1], idx[:, 2]].long()
    return row_start, words


def shape_cost(N, n_cls, h, w, H, W, align, cell, repeats, window, copy_peak, dev):
    lib = _lib.load()
    g = np.random.Generator(np.random.PCG64(5))
    logits = blob_logits(g, N, n_cls, h, w, cell, dev)
    lab = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    back = torch.empty_like(lab)
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    al = 1 if align else 0
    name = f"{N}x{n_cls}x{h}x{w} -> {H}x{W}"

    def labels8():
        _lib.check(lib.arseg_segment_egress_fwd(P(logits), N, n_cls, h, w, H, W, al, None, P(lab), W, H * W, 0, null, null, null, 0, 0, 0, 0, 0, 0,
                                                null, null, null, 0, 0, 0, 0, 0, 0, None, None, st), "egress")

    # ---- sizing pass, then a buffer with a quarter of headroom
    labels8()
    _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), null, 0, st), "rle sizing")
    needed = row_start[:, H].cpu().numpy().astype(np.int64)
    cap = int(needed.max()) * 5 // 4 + 16
    runs = torch.full((N, cap), -1, dtype=torch.int32, device=dev)

    def encode():
        _lib.check(lib.arseg_labels_rle_fwd(P(lab), W, H * W, N, H, W, P(row_start), P(runs), cap, st), "rle encode")

    def decode():
        _lib.check(lib.arseg_rle_decode_fwd(P(row_start), P(runs), cap, N, H, W, P(back), W, H * W, st), "rle decode")

    # ---- correctness first: bit for bit against the composition
    encode()
    back.fill_(0xA5)
    decode()
    torch.cuda.synchronize()
    want_start, want_words = torch_form(lab)
    if not torch.equal(row_start.long(), want_start):
        raise SystemExit(f"{name}: row_start differs from the composition's")
    got = torch.cat([runs[n, :int(needed[n])] for n in range(N)]).long() & 0xFFFFFFFF
    if not torch.equal(got, want_words):
        raise SystemExit(f"{name}: the runs differ from the composition's in {int((got != want_words).sum())} words")
    if not bool((runs[0, int(needed[0]):] == -1).all()):
        raise SystemExit(f"{name}: words beyond the needed ones were written")
    if not torch.equal(back, lab):
        raise SystemExit(f"{name}: the decoder does not give the plane back ({int((back != lab).sum())} pixels differ)")
    del want_start, want_words, got

    pin_plane = torch.empty((N, H, W), dtype=torch.uint8).pin_memory()
    pin_need = torch.empty((N,), dtype=torch.int32).pin_memory()
    pin_runs = torch.empty((N, cap), dtype=torch.int32).pin_memory()

    def copy_plane():
        pin_plane.copy_(lab, non_blocking=True)

    def copy_runs():
        pin_need.copy_(row_start[:, H], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        m = int(pin_need.max())
        pin_runs[:, :m].copy_(runs[:, :m], non_blocking=True)

    def both(*fns):
        def run():
            for f in fns:
                f()
        return run

    forms = {"labels8": labels8, "labels8_encode": both(labels8, encode), "encode": encode, "decode": decode,
             "torch": lambda: torch_form(lab), "copy_plane": copy_plane, "copy_runs": copy_runs,
             "e2e_plane": both(labels8, copy_plane), "e2e_runs": both(labels8, encode, copy_runs)}
    res = alternate(forms, repeats, window)

    px, total_runs = N * H * W, int(needed.sum())
    enc_bytes = 2 * px + 4 * total_runs + 12 * N * (H + 1)          # the plane twice; the words; row_start written, scanned, read
    res["encode"]["bytes_needed"] = enc_bytes
    res["encode"]["GBps"] = enc_bytes / (res["encode"]["us_median"] * 1e-6) / 1e9
    res["encode"]["share_of_stream_copy"] = res["encode"]["GBps"] / copy_peak
    res["decode"]["bytes_needed"] = px + 4 * total_runs + 4 * N * (H + 1)
    res["decode"]["GBps"] = res["decode"]["bytes_needed"] / (res["decode"]["us_median"] * 1e-6) / 1e9
    base = res["labels8"]
    for r in res.values():
        r["time_over_labels8"] = r["us_median"] / base["us_median"]
    e, t = res["encode"], res["torch"]
    spreads = (e["us_max"] - e["us_min"]) + (t["us_max"] - t["us_min"])
    verdict = {"torch_over_encode": t["us_median"] / e["us_median"], "gap_us": t["us_median"] - e["us_median"], "spreads_us": spreads,
               "encode_beats_torch_beyond_spreads": bool(t["us_median"] - e["us_median"] > spreads),
               "e2e_runs_over_e2e_plane": res["e2e_runs"]["us_median"] / res["e2e_plane"]["us_median"]}
    code_bytes = 4 * (needed + H + 1)
    inputs = {"runs_per_frame": needed.tolist(), "runs_per_row_mean": float(needed.mean() / H), "plane_bytes_per_frame": H * W,
              "code_bytes_per_frame_mean": float(code_bytes.mean()), "code_over_plane": float(code_bytes.mean() / (H * W)), "capacity": cap}
    print(f"{name}: " + ", ".join(f"{k} {r['us_median']:.1f} us ({r['us_min']:.1f}-{r['us_max']:.1f})" for k, r in res.items()) +
          f"; runs/frame {int(needed.mean())}, code/plane {inputs['code_over_plane']:.4f}", file=sys.stderr)
    return {"logits": [N, n_cls, h, w], "labels": [H, W], "align_corners": bool(align), "inputs": inputs, "verdict": verdict, "forms": res}


def stream_copy_gbps(repeats, window, dev):
    lib = _lib.load()
    n = 256 << 20
    src, dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.check(lib.arseg_peak_stream_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n, st), "stream copy")

    r = alternate({"stream_copy": run}, repeats, window)["stream_copy"]
    r["bytes_needed"] = 2 * n
    r["GBps"] = 2 * n / (r["us_median"] * 1e-6) / 1e9
    return r


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "rle.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rle.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    _lib.load()
    res = {"repeats": a.repeats, "window_s": a.window, "device": torch.cuda.get_device_name(0), "shapes": []}
    res["stream_copy"] = stream_copy_gbps(a.repeats, a.window, dev)
    res["shapes"].append(shape_cost(11, 12, 720, 960, 720, 960, True, 32, a.repeats, a.window, res["stream_copy"]["GBps"], dev))
    res["shapes"].append(shape_cost(11, 19, 128, 256, 1024, 2048, False, 4, a.repeats, a.window, res["stream_copy"]["GBps"], dev))
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
