#!/usr/bin/env python3
"""What it costs to get 8-bit decoder frames into the conv engine's input format.  One process, variants alternated, --repeats windows of
>= --window seconds each (HIP events on the launch stream), median and min-max.

Shapes: the 11 non-keyframes of a GOP at 512x1024 -> 256x512 and at 1024x2048 -> 512x1024, and the keyframe at identity size (512x1024 and
1024x2048), each into fp32 NHWC4 / bf16 / fp16 NHWC8.  Routes:
  rgb8           ops.frame_ingest8 from uint8 RGB          (one kernel)
  nv12           ops.frame_ingest8 from NV12               (one kernel)
  torch_then_f32 what a caller had to do before for the same uint8 RGB frames: torch ops to a normalised fp32 NCHW tensor
                 (permute, float, /255, -mean, /std), then ops.frame_ingest
  f32            ops.frame_ingest alone from a ready fp32 NCHW tensor
--yuv: the planar 4:2:0 / 10-bit routes instead, same protocol, written to profiles/ingest_yuv.json:
  i420 / p010 / i010   ops.frame_ingest_yuv from I420 / P010 / I010 planes   (one kernel)
  nv12                 the NV12 route above, run again in the same process: the yardstick of that table
and the GOP step from I420 and P010 frames next to NV12.
GB/s = the bytes the route MUST move (its source once + its output once) over the time; beside the stream-copy figure of a bench.py --full
run if one is on file (--peaks).  Then one bise_bf16-shaped GOP step (keyframe 1024x2048 + 11 non-keyframes at 0.5x) end to end from
DecodedFrames (RGB8, NV12) and from fp32 frames.  One JSON line on stdout, the same written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from arseg_amd import _lib, ingest, ops, synth
from arseg_amd import evaluation as ev
from arseg_amd.model import BiSeNetV1, BiSeNetV1WithFuse

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MEAN, STD = synth.CITY_BISE_MEAN, synth.CITY_BISE_STD


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
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}


def shape_cost(N, H, W, h, w, repeats, window, dev, copy_gbps):
    g = np.random.Generator(np.random.PCG64(1))
    u8 = torch.from_numpy(g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(dev)
    y = torch.from_numpy(g.integers(0, 256, (N, H, W), dtype=np.uint8)).to(dev)
    uv = torch.from_numpy(g.integers(0, 256, (N, H // 2, W // 2, 2), dtype=np.uint8)).to(dev)
    rgb, nv = ingest.DecodedFrames.rgb8(u8, MEAN, STD), ingest.DecodedFrames.nv12(y, uv, MEAN, STD)
    m = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    s = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    to_f32 = lambda: (u8.permute(0, 3, 1, 2).float() / 255.0 - m) / s
    f32 = to_f32().contiguous()
    rows = []
    for name, dt in DT.items():
        out_b = N * h * w * (16 if dt == torch.float32 else 16)          # NHWC4 fp32 and NHWC8 16-bit are both 16 bytes per pixel
        need = {"rgb8": N * H * W * 3 + out_b, "nv12": N * H * W * 3 // 2 + out_b, "torch_then_f32": N * H * W * 3 + out_b, "f32": N * H * W * 12 + out_b}
        forms = {"rgb8": lambda: rgb.to_input(h, w, dt), "nv12": lambda: nv.to_input(h, w, dt),
                 "torch_then_f32": lambda: ops.frame_ingest(to_f32(), h, w, dt), "f32": lambda: ops.frame_ingest(f32, h, w, dt)}
        res = alternate(forms, repeats, window)
        for k, r in res.items():
            r["bytes_needed"] = need[k]
            r["GBps_of_needed_bytes"] = need[k] / (r["ms_median"] * 1e-3) / 1e9
            if copy_gbps:
                r["share_of_stream_copy"] = r["GBps_of_needed_bytes"] / copy_gbps
        rows.append({"frames": N, "source": [H, W], "output": [h, w], "dtype": name, "routes": res})
        print(f"{N} x {H}x{W} -> {h}x{w} {name}: " + ", ".join(f"{k} {r['ms_median'] * 1e3:.1f} us ({r['GBps_of_needed_bytes']:.0f} GB/s)" for k, r in res.items()), file=sys.stderr)
    return rows


def shape_cost_yuv(N, H, W, h, w, repeats, window, dev, copy_gbps):
    g = np.random.Generator(np.random.PCG64(1))
    u8 = lambda *s: torch.from_numpy(g.integers(0, 256, s, dtype=np.uint8)).to(dev)
    u16 = lambda shift, *s: torch.from_numpy(g.integers(0, 1024, s, dtype=np.uint16) << shift).to(dev)
    D = ingest.DecodedFrames
    src = {"nv12": D.nv12(u8(N, H, W), u8(N, H // 2, W // 2, 2), MEAN, STD),
           "i420": D.i420(u8(N, H, W), u8(N, H // 2, W // 2), u8(N, H // 2, W // 2), MEAN, STD),
           "p010": D.p010(u16(6, N, H, W), u16(6, N, H // 2, W // 2, 2), MEAN, STD),
           "i010": D.i010(u16(0, N, H, W), u16(0, N, H // 2, W // 2), u16(0, N, H // 2, W // 2), MEAN, STD)}
    rows = []
    for name, dt in DT.items():
        out_b = N * h * w * 16                                           # NHWC4 fp32 and NHWC8 16-bit are both 16 bytes per pixel
        need = {k: N * H * W * 3 // 2 * (2 if k in ("p010", "i010") else 1) + out_b for k in src}
        res = alternate({k: (lambda d=d: d.to_input(h, w, dt)) for k, d in src.items()}, repeats, window)
        for k, r in res.items():
            r["bytes_needed"] = need[k]
            r["GBps_of_needed_bytes"] = need[k] / (r["ms_median"] * 1e-3) / 1e9
            r["time_over_nv12"] = r["ms_median"] / res["nv12"]["ms_median"]
            if copy_gbps:
                r["share_of_stream_copy"] = r["GBps_of_needed_bytes"] / copy_gbps
        rows.append({"frames": N, "source": [H, W], "output": [h, w], "dtype": name, "routes": res})
        print(f"{N} x {H}x{W} -> {h}x{w} {name}: " + ", ".join(f"{k} {r['ms_median'] * 1e3:.1f} us ({r['ms_min'] * 1e3:.1f}-{r['ms_max'] * 1e3:.1f}; {r['GBps_of_needed_bytes']:.0f} GB/s)"
                                                                 for k, r in res.items()), file=sys.stderr)
    return rows


def gop_step(repeats, window, dev, H=1024, W=2048, gop=12, yuv=False):
    hr, lr = BiSeNetV1(n_classes=19, backend="resnet18"), BiSeNetV1WithFuse(n_classes=19, backend="resnet18")
    synth.load_synth_weights(hr, 0)
    synth.load_synth_weights(lr, 1)
    hr, lr = hr.to(dev).eval().set_storage(torch.bfloat16), lr.to(dev).eval().set_storage(torch.bfloat16)
    clip = synth.make_clip(40, H, W, gop=gop, mean=MEAN, std=STD)
    u8 = np.rint((clip["frames"].transpose(0, 2, 3, 1).astype(np.float64) * np.asarray(STD) + np.asarray(MEAN)) * 255.0).astype(np.uint8)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    y, uv = ingest.rgb_to_nv12(u8)
    src = {"fp32_frames": torch.from_numpy(clip["frames"]).to(dev), "rgb8": ingest.DecodedFrames.rgb8(torch.from_numpy(u8).to(dev), MEAN, STD),
           "nv12": ingest.DecodedFrames.nv12(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev), MEAN, STD)}
    if yuv:
        del src["rgb8"]
        src["i420"] = ingest.DecodedFrames.i420(*[torch.from_numpy(p).to(dev) for p in ingest.rgb_to_yuv420(u8, "i420")], MEAN, STD)
        src["p010"] = ingest.DecodedFrames.p010(*[torch.from_numpy(p).to(dev) for p in ingest.rgb_to_yuv420(u8, "p010")], MEAN, STD)

    def step(f):
        _, ref = hr.forward_keyframe(f[0:1])
        return ev.alter_res_batch_pred(lr, [ref[0]] * (gop - 1), f[1:], mvs[1:], 0.5)[0]

    preds = {k: step(f) for k, f in src.items()}
    res = alternate({k: (lambda f=f: step(f)) for k, f in src.items()}, repeats, window)
    for k, r in res.items():
        r["frames_per_s"] = gop / (r["ms_median"] * 1e-3)
        r["labels_equal_fp32_frames_run"] = float((preds[k] == preds["fp32_frames"]).float().mean())
    return {"workload": f"BiSeNet-18 bf16, keyframe {H}x{W} + {gop - 1} non-keyframes at 0.5x, eager, one stream", "repeats": repeats, "window_s": window, "sources": res}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--only", choices=["ingest", "gop"], default=None)
    ap.add_argument("--peaks", default=os.path.join(root, "profiles", "r06_bise_bf16_bench.json"), help="a bench.py --full result holding the on-box stream-copy rate")
    ap.add_argument("--yuv", action="store_true", help="the I420 / P010 / I010 routes beside NV12 -> profiles/ingest_yuv.json")
    ap.add_argument("--out", default=None, help="default: profiles/ingest_formats.json, or profiles/ingest_yuv.json with --yuv")
    a = ap.parse_args()
    a.out = a.out or os.path.join(root, "profiles", "ingest_yuv.json" if a.yuv else "ingest_formats.json")
    dev = torch.device("cuda:0")
    _lib.load()
    copy_gbps = None
    if os.path.exists(a.peaks):
        with open(a.peaks) as f:
            pk = json.load(f)

        def find(o):
            if isinstance(o, dict):
                if isinstance(o.get("hbm_stream_copy_GBps"), (int, float)):
                    return float(o["hbm_stream_copy_GBps"])
                o = list(o.values())
            return next((v for v in map(find, o) if v is not None), None) if isinstance(o, list) else None

        copy_gbps = find(pk)
    res = {"repeats": a.repeats, "window_s": a.window, "stream_copy_GBps_on_file": copy_gbps}
    with torch.no_grad():
        if a.only != "gop":
            res["ingest"] = []
            for (N, H, W, h, w) in ((11, 512, 1024, 256, 512), (11, 1024, 2048, 512, 1024), (1, 512, 1024, 512, 1024), (1, 1024, 2048, 1024, 2048)):
                res["ingest"] += (shape_cost_yuv if a.yuv else shape_cost)(N, H, W, h, w, a.repeats, a.window, dev, copy_gbps)
        if a.only != "ingest":
            res["gop_step"] = gop_step(a.repeats, a.window, dev, yuv=a.yuv)
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
