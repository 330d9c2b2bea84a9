#!/usr/bin/env python3
"""The CamVid PSPNet-18 GOP-12 step at 512x1024 (keyframe HR forward + 11 non-keyframes through alter_res_batch_fast) in fp32 (f16x3 convs),
bf16 and fp16 storage, in one process; plus the two measurements the 16-bit path's routing rests on:
  * the x2-upsample convs (up_1 / up_2 / up_3 of the keyframe and of the LR batch): the best fused patch plan against resize16 + conv2d16,
    and which of the two the plan cache keeps;
  * phase 2 on 16-bit features at the headline shape: the fused warp + CReFF kernel reading the 16-bit tensors directly, cast-once + its
    fp32 instantiation (PSPNetWithFuse.phase2_warp under creff_warp16 = direct / cast) and the two-kernel 16-bit route (warp_mvq16 to an
    fp32 C8 tensor + CReFF); the GOP step in bf16 / fp16 is timed under both knob values (variants "bf16" = default, "bf16_cast", ...).
Variants are alternated (repeats x variants), each timed over windows of >= 0.5 s after >= 2 warm-up steps; the spread over repeats is
printed with the median.  --profile-step DTYPE: warm up, then run a few steps of that variant only (for rocprofv3 --kernel-trace --stats).
One JSON line on stdout; the per-layer tables (ops.profile().layers()) with --layers."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from arseg_amd import _lib, ops, synth
from arseg_amd import evaluation as ev
from arseg_amd.model import PSPNet, PSPNetWithFuse

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def window_ms(fn, min_s=0.5):
    """ms per call, averaged over a window of at least min_s seconds (HIP events on the launch stream)."""
    fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < 1e3 * min_s:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(4):
            fn()
        e.record()
        e.synchronize()
        total += s.elapsed_time(e)
        n += 4
    return total / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--profile-step", choices=sorted(DT) + ["bf16_direct", "bf16_cast", "fp16_direct", "fp16_cast"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = 512, 1024
    kw = dict(sizes=(1, 2, 3, 6), n_classes=12, psp_size=512, deep_features_size=256, backend="resnet18")
    hr, lr = PSPNet(**kw), PSPNetWithFuse(atten_k=7, **kw)
    synth.load_synth_weights(hr, 0)
    synth.load_synth_weights(lr, 1)
    hr, lr = hr.to(dev).eval(), lr.to(dev).eval()
    clip = synth.make_clip(2, H, W, gop=12, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"]).to(dev)

    def step(name):
        # "bf16_direct" / "bf16_cast": the 16-bit step with the phase-2 route pinned (plain "bf16": the default route)
        name, _, route = name.partition("_")
        prev = ops.configure(creff_warp16=route)
        try:
            hr.set_storage(DT[name])
            lr.set_storage(DT[name])
            _, ref = hr.forward_keyframe(frames[0:1])
            return ev.alter_res_batch_fast(lr, [ref[0]] * 11, frames[1:12], mvs[1:12], 0.5)
        finally:
            ops.configure(**prev)

    variants = [a.profile_step] if a.profile_step else ["fp32", "bf16_direct", "bf16_cast", "fp16_direct", "fp16_cast"]
    with torch.no_grad():
        for v in variants:                      # warm-ups (the first also tunes every conv plan of the variant)
            for _ in range(max(2, a.warmup)):
                step(v)
        torch.cuda.synchronize()
        if a.profile_step:
            for _ in range(3):
                step(a.profile_step)
            torch.cuda.synchronize()
            print(json.dumps({"profile_step": a.profile_step, "steps": 3}))
            return
        ms = {v: [] for v in variants}
        for _ in range(a.repeats):
            for v in variants:
                ms[v].append(window_ms(lambda: step(v), a.window))
        res = {"workload": "PSPNet-18 GOP-12 step at 512x1024: keyframe HR forward + 11 non-keyframes (LR 0.5x) through alter_res_batch_fast",
               "repeats": a.repeats, "window_s": a.window, "variants": {}}
        for v in variants:
            fps = [12 * 1e3 / m for m in ms[v]]
            res["variants"][v] = {"ms_per_step_median": statistics.median(ms[v]), "frames_per_s_median": statistics.median(fps),
                                  "frames_per_s_min": min(fps), "frames_per_s_max": max(fps)}
        layers = {}
        for v in variants:
            with ops.profile() as prof:
                step(v)
            rows = prof.layers()
            layers[v] = rows
            summ = prof.summary()
            res["variants"][v]["ms_by_op_profiled_step"] = {k: round(r["ms"], 4) for k, r in sorted(summ.items())}
        if a.layers:
            res["layers"] = layers

        # x2-upsample convs: best fused patch plan against resize16 + conv2d16, per dtype, keyframe and LR-batch shapes
        up = {}
        for v in ("bf16", "fp16"):
            dt = DT[v]
            for who, N, h, w in (("key", 1, 64, 128), ("lr", 11, 32, 64)):
                for name, mod, sc in (("up_1", lr.up_1, 1), ("up_2", lr.up_2, 2), ("up_3", lr.up_3, 4)):
                    pc = mod.packed()
                    x = torch.randn(N, h * sc, w * sc, pc.cin, device=dev).to(dt)
                    fused = {}
                    for cfg in (5, 6, 7, 8, 10, 11, 12, 13):
                        try:
                            fused[cfg] = 1e3 * window_ms(lambda: ops.conv2d(x, pc, up2=True, tile_cfg=cfg), 0.1)
                        except _lib.ArsegError:
                            pass
                    mat = 1e3 * window_ms(lambda: ops.conv2d(ops.resize_nhwc(x, 2 * h * sc, 2 * w * sc, _lib.BILINEAR, False), pc), 0.1)
                    key = ("conv16", dev.index, _lib.DT_BF16 if dt == torch.bfloat16 else _lib.DT_F16, N, 2 * h * sc, 2 * w * sc, pc.cin,
                           pc.cout, 3, 3, 1, 1, 1, "up2")
                    best = min(fused, key=fused.get)
                    up[f"{v}_{who}_{name}"] = {"in": [N, h * sc, w * sc, pc.cin], "cout": pc.cout, "fused_best_plan": best,
                                               "fused_best_us": fused[best], "materialised_us": mat, "plan_cache": ops._conv_plans.get(key)}
        res["up2_convs"] = up

        # phase 2 at the headline shape on 16-bit features, three routes alternated (repeats x routes): the rolling kernel reading the 16-bit
        # tensors directly, cast-once + its fp32 instantiation (both through phase2_warp, pinned by the creff_warp16 knob), and the two-kernel
        # 16-bit route (warp_mvq16 to an fp32 C8 tensor + CReFF)
        from arseg_amd.ops.creff import _creff_warp16_two_kernel

        p2 = {}
        hd = lr.packed()["head"]
        pa = lr.fuse_attention.packed()
        for v in ("bf16", "fp16"):
            dt = DT[v]
            feat = torch.randn(11, H // 2, W // 2, 64, device=dev).to(dt)
            ref = torch.randn(H, W, 64, device=dev).to(dt)
            refs = [ref] * 11
            code = _lib.DT_BF16 if dt == torch.bfloat16 else _lib.DT_F16

            def knob(value):
                def run():
                    prev = ops.configure(creff_warp16=value)
                    try:
                        lr.phase2_warp(feat, refs, mvs[1:12])
                    finally:
                        ops.configure(**prev)
                return run

            routes = {"direct16_fused_ms": knob("direct"), "cast_once_fp32_fused_ms": knob("cast"),
                      "route16_warp_mvq16_creff_ms": lambda: _creff_warp16_two_kernel(code, refs, mvs[1:12], feat, pa, (hd.wf, hd.bf), True, 7, 7, _lib.C8)}
            t = {k: [] for k in routes}
            for _ in range(a.repeats):
                for k, fn in routes.items():
                    t[k].append(window_ms(fn, a.window))
            p2[v] = {k: statistics.median(x) for k, x in t.items()}
            p2[v].update({k.replace("_ms", "_min_max_ms"): [min(x), max(x)] for k, x in t.items()})
            p2[v]["winner"] = min(routes, key=lambda k: p2[v][k])[:-3]
        res["phase2_16bit"] = p2
    print(json.dumps(res))


if __name__ == "__main__":
    main()
