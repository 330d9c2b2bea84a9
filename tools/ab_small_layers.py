#!/usr/bin/env python3
"""A/B of the small NHWC layers (csrc/layers.hip, the 16-bit warp of csrc/warp.hip) between two builds of the library: output bits and speed.
ARSEG_HIP_LIB selects the build; one process per build, then --against compares two result files.  GPU only.

    ARSEG_HIP_LIB=<a.so> python tools/ab_small_layers.py --out a.json [--time]
    ARSEG_HIP_LIB=<b.so> python tools/ab_small_layers.py --out b.json [--time] --against a.json

Bits: every small-layer wrapper and the two arseg_warp_mvq16 entries on fixed seeded inputs in fp32, fp16 and bf16 -- C == V and 3 V (V = 4 / 8
channels per lane), 9x13 and an odd 33x47 map, N = 2; the inputs hold +-0, +-inf, a NaN inside a maxpool window / a global-max slice / a head
input, and products that overflow fp16 at the store of scale_add -- as the sha256 of each output's bytes.  --against: every digest must be equal.
--time: each wrapper at the shapes it takes in one GOP step of the headline config and of bise_bf16 (recorded from one step under
ops.profile()), tools/bench_regions.py's protocol (forms alternated, windows >= 0.5 s, median and min-max).  --against then prints this
run's median beside the other run's min-max; nothing is gated on a ratio."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

from arseg_amd import _lib, ops

SIZES = (1, 2, 3, 6)
TIMED = ("maxpool3x3s2", "psp_pool_matrix", "psp_prior_sum", "global_reduce", "resize_nhwc", "scale_add", "head", "frame_ingest", "cast")


def rnd(seed, *shape, dtype=torch.float32, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32)).to(dtype).cuda()


def digests():
    out = {}

    def put(name, t):
        torch.cuda.synchronize()
        out[name] = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        V = 4 if dtype == torch.float32 else 8
        for N, H, W, C in ((2, 5, 7, V), (2, 5, 7, 3 * V), (2, 9, 13, 16), (2, 33, 47, 16), (1, 9, 37, 64)):
            tag = f"{str(dtype)[6:]}/{H}x{W}x{C}/"
            x = rnd(1, N, H, W, C, dtype=dtype)
            x[0, 0, 0, 0], x[0, 0, 0, 1], x[0, 0, 1, 0], x[0, 0, 1, 1] = 0.0, -0.0, float("inf"), float("-inf")
            xn = x.clone()
            xn[-1, H // 2, W // 2, 2] = float("nan")          # inside a 3x3 window, inside a pixel slice, one head input
            for k, v in (("", x), ("nan/", xn)):
                put(tag + k + "maxpool", ops.maxpool3x3s2(v))
                put(tag + k + "global_max", ops.global_reduce(v, _lib.REDUCE_MAX))
                for n_cls, lsm in ((5, True), (19, False)):
                    put(tag + k + f"head{n_cls}", ops.head(v, rnd(2, n_cls, C, scale=0.2), rnd(3, n_cls, scale=0.1), lsm))
            put(tag + "global_mean", ops.global_reduce(x, _lib.REDUCE_MEAN))
            for mode, al in ((_lib.NEAREST, False), (_lib.BILINEAR, False), (_lib.BILINEAR, True)):
                put(tag + f"resize{mode}{int(al)}", ops.resize_nhwc(x, 2 * H + 1, 2 * W - 1, mode, al))
            sc, av, af = rnd(4, N, 1, 1, C, dtype=dtype), rnd(5, N, 1, 1, C, dtype=dtype), rnd(6, N, H, W, C, dtype=dtype)
            put(tag + "scale_add", ops.scale_add(x, sc, add_full=af, add_vec=av))
            put(tag + "scale_add_vec", ops.scale_add(x, sc, add_vec=av))
            put(tag + "scale_add_overflow", ops.scale_add(x * 200, sc * 400, add_full=af))          # |products| up to ~1e6 > 65504
            if C % 8 == 0:
                put(tag + "psp_pool_matrix", ops.psp_pool_matrix(x, SIZES))
                put(tag + "psp_prior_sum", ops.psp_prior_sum(rnd(7, N, 50, C, dtype=dtype), SIZES, H, W))
        for (Hs, Ws, h, w) in ((36, 48, 18, 24), (35, 47, 17, 23), (20, 32, 20, 32), (64, 1200, 32, 600)):
            put(f"{str(dtype)[6:]}/frame_ingest{Hs}x{Ws}", ops.frame_ingest(rnd(8, 2, 3, Hs, Ws), h, w, dtype))
        if dtype == torch.float32:
            continue
        y = rnd(9, 4, 40)
        put(f"{str(dtype)[6:]}/cast16", ops.cast(y, dtype))
        put(f"{str(dtype)[6:]}/cast32", ops.cast(ops.cast(y, dtype), torch.float32))
        H, W, Hp, Wp, C, B = 64, 96, 8, 12, 64, 3
        g = np.random.Generator(np.random.PCG64(10))
        mv = torch.from_numpy((g.integers(-12, 13, (B, H, W, 2)) * 4).astype(np.int16)).cuda()
        lib, feat = _lib.load(), rnd(11, B, Hp, Wp, C, dtype=dtype)
        for name, full in (("warp_mvq16", True), ("warp_mvq16_shared", False)):
            o = torch.empty((B, C // 8, Hp, Wp, 8), dtype=torch.float32, device="cuda")
            args = (ctypes.c_void_p(feat.data_ptr()),) + (() if full else (0,)) + (ops._DT16[dtype], ctypes.c_void_p(mv.data_ptr()),
                    ctypes.c_void_p(o.data_ptr()), B, C, Hp, Wp, H, W, st)
            assert getattr(lib, f"arseg_{name}_fwd")(*args) == 0
            put(f"{str(dtype)[6:]}/{name}", o)
    return out


def gop_step_calls(config):
    """The distinct calls of the TIMED wrappers in one GOP step (keyframe + 11 non-keyframes) of a bench.py config: (name, args with every
    tensor replaced by its (shape, dtype)), recorded while the step runs under ops.profile()."""
    import bench
    from arseg_amd import evaluation as ev

    cfg = bench.CONFIGS[config]
    hr, lr, _, _ = bench.build_nets(torch.device("cuda"), cfg)
    if "storage" in cfg:
        sdt = {"bf16": torch.bfloat16, "f16": torch.float16}[cfg["storage"]]
        hr.set_storage(sdt), lr.set_storage(sdt)
    calls, orig = {}, {n: getattr(ops.layers, n) for n in TIMED}
    spec = lambda a: ("T", tuple(a.shape), str(a.dtype)) if torch.is_tensor(a) else a

    def recorder(name):
        def f(*args, **kw):
            key = (name, tuple(spec(a) for a in args), tuple(sorted((k, spec(v)) for k, v in kw.items() if k != "out")))
            calls.setdefault(repr(key), key)
            return orig[name](*args, **kw)
        return f

    for n in TIMED:
        setattr(ops, n, recorder(n)), setattr(ops.layers, n, getattr(ops, n))
    try:
        H, W = cfg["H"], cfg["W"]
        with torch.no_grad(), ops.profile():
            ref = hr.forward_keyframe(rnd(20, 1, 3, H, W))[-1][0]
            step = ev.alter_res_batch_pred if cfg["kind"] == "bise" else ev.alter_res_batch_fast
            step(lr, [ref] * 11, rnd(21, 11, 3, H, W), torch.zeros((11, H, W, 2), dtype=torch.int16, device="cuda"), cfg.get("scale", 0.5))
    finally:
        for n in TIMED:
            setattr(ops, n, orig[n]), setattr(ops.layers, n, orig[n])
    return list(calls.values())


def timings(repeats, window):
    from bench_regions import alternate

    shapes, forms = {}, {}
    make = lambda a, i: rnd(30 + i, *a[1], dtype=getattr(torch, a[2][6:])) if isinstance(a, tuple) and a[:1] == ("T",) else a
    for config in ("psp", "bise_bf16"):
        for j, (name, args, kw) in enumerate(gop_step_calls(config)):
            a, k = [make(v, i) for i, v in enumerate(args)], {kk: make(v, 9) for kk, v in kw}
            label = f"{config}/{name}/{j}"
            shapes[label] = repr((args, kw))
            forms[label] = (lambda fn, a, k: lambda: fn(*a, **k))(getattr(ops, name), a, k)
    print(json.dumps({"shapes": shapes}, indent=1), file=sys.stderr)
    with torch.no_grad():
        return {"shapes": shapes, "us": alternate(forms, repeats, window)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--against", help="result file of the other build: digests must be equal; timings are printed side by side")
    args = ap.parse_args()
    res = {"lib": os.path.abspath(_lib.LIB_PATH), "digests": digests()}
    if args.time:
        res.update(timings(args.repeats, args.window))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    if not args.against:
        print(f"{len(res['digests'])} digests -> {args.out}")
        return 0
    other = json.load(open(args.against))
    bad = sorted(k for k in set(res["digests"]) | set(other["digests"]) if res["digests"].get(k) != other["digests"].get(k))
    for k, v in res.get("us", {}).items():
        o = other.get("us", {}).get(k)
        if o:
            print(f"{k:40s} {v['us_median']:9.1f} us   other {o['us_median']:9.1f} [{o['us_min']:.1f}, {o['us_max']:.1f}]")
    print(f"{len(res['digests'])} digests, {len(bad)} differ from {args.against}" + "".join(f"\n  {k}" for k in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
