#!/usr/bin/env python
"""Which kernels the conv launch plans launch, for comparing two builds of the library (a host-side change must leave the list as it was).

    rocprofv3 --kernel-trace -d DIR -o t --output-format json -- python tools/ab_conv_launches.py
    python tools/ab_conv_launches.py --list DIR/.../t_results.json profiles/conv_launches.json

The first form pins every (engine, tile_cfg, split_k) once on a few small shapes -- both engines, every id, f32 and f16x3, fp16 and bf16, with
and without a fused x2 upsample -- through arseg_conv2d_fwd / arseg_conv2d16_fwd with the workspace their *_workspace_bytes queries ask for;
a refused plan launches nothing.  It uses no entry point younger than those, so it runs on older builds.  The second form reduces the trace to
the sequence of (kernel with template arguments, grid, workgroup, LDS bytes) of the conv kernels, runs of equal launches counted."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#         H,  W,  Cin, Cout, k, stride, pad, dil      (N = 1)
SHAPES = {"w50": (12, 50, 64, 64, 3, 1, 1, 1), "w24": (12, 24, 64, 64, 3, 1, 1, 1), "w16": (12, 16, 64, 64, 3, 1, 1, 1), "dil2": (12, 50, 64, 64, 3, 1, 2, 2),
          "stem": (20, 40, 8, 64, 7, 2, 3, 1), "1x1": (12, 50, 96, 19, 1, 1, 0, 1), "deep": (8, 8, 512, 128, 3, 1, 1, 1)}
SPLITS = (0, 1, 2, 4)


def launches():
    import torch

    from arseg_amd import _lib

    lib, dev = _lib.load(), torch.device("cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    accepted = {}
    for shape, (H, W, Cin, Cout, k, stride, pad, dil) in SHAPES.items():
        kpad = (k * k * Cin + 63) // 64 * 64
        Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        ld = (Cout + 7) // 8 * 8
        x = torch.zeros(H * W * Cin, dtype=torch.float32, device=dev)
        w = torch.zeros(Cout * kpad, dtype=torch.float32, device=dev)
        out = torch.zeros(Ho * Wo * ld, dtype=torch.float32, device=dev)
        for engine, n_ids, code in (("f32", 24, _lib.MATH_F32), ("f16x3", 24, _lib.MATH_F16X3), ("fp16", 14, _lib.DT_F16), ("bf16", 14, _lib.DT_BF16)):
            is16 = engine in ("fp16", "bf16")
            for up2 in (0, 1):
                for cfg in range(n_ids):
                    for sk in SPLITS:
                        d = _lib.ConvDesc()
                        d.N, d.H, d.W, d.Cin, d.in_ld, d.Cout, d.out_ld, d.res_ld = 1, H, W, Cin, Cin, Cout, ld, ld
                        d.R, d.S, d.stride, d.pad, d.dil = k, k, stride, pad, dil
                        d.tile_cfg, d.split_k, d.upsample2x, d.math = cfg, sk, up2, _lib.MATH_F32 if is16 else code
                        nbytes = (lib.arseg_conv2d16_workspace_bytes if is16 else lib.arseg_conv2d_workspace_bytes)(ctypes.byref(d))
                        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
                        wp = ws.data_ptr() if nbytes else None
                        if is16:
                            st = lib.arseg_conv2d16_fwd(ctypes.byref(d), code, x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), wp, nbytes, stream)
                        else:
                            st = lib.arseg_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), wp, nbytes, stream)
                        if st > 0:
                            raise SystemExit(f"HIP error {st} at {(shape, engine, up2, cfg, sk)}")
                        accepted[engine] = accepted.get(engine, 0) + (st == 0)
        torch.cuda.synchronize()
    print(json.dumps({"accepted_launches": accepted}))


def walk(node):
    if isinstance(node, dict):
        yield node
        node = list(node.values())
    if isinstance(node, list):
        for v in node:
            yield from walk(v)


def listing(trace, dest):
    """``trace``: rocprofv3's JSON output (…_results.json).  Its dispatch records carry the group segment size of the dispatch -- static plus
    dynamic LDS; the LDS_Block_Size column of the CSV output is 0 for kernels whose LDS is dynamic, as all of these are."""
    with open(trace) as f:
        nodes = list(walk(json.load(f)))
    names = {}
    for n in nodes:
        if "kernel_id" in n and any(k in n for k in ("formatted_kernel_name", "demangled_kernel_name", "kernel_name")):
            names[n["kernel_id"]] = n.get("formatted_kernel_name") or n.get("demangled_kernel_name") or n["kernel_name"]
    disp = {n["dispatch_info"]["dispatch_id"]: n["dispatch_info"] for n in nodes if isinstance(n.get("dispatch_info"), dict)}
    rows = [{"name": names[i["kernel_id"]], "grid": [i["grid_size"][a] for a in "xyz"], "wg": [i["workgroup_size"][a] for a in "xyz"],
             "lds": i["group_segment_size"]} for _, i in sorted(disp.items())]
    kernels, seq = [], []
    for r in rows:
        if "conv" not in r["name"]:
            continue
        k = r["name"].replace("(anonymous namespace)::", "")
        if k not in kernels:
            kernels.append(k)
        item = [kernels.index(k), r["grid"], r["wg"], r["lds"]]
        if seq and seq[-1][1:] == item:
            seq[-1][0] += 1
        else:
            seq.append([1] + item)
    with open(dest, "w") as f:
        f.write('{"note": "tools/ab_conv_launches.py under rocprofv3 --kernel-trace: [times, index into kernels, grid, workgroup, LDS bytes] in launch order",\n"kernels": [\n')
        f.write(",\n".join(json.dumps(k) for k in kernels))
        f.write('\n],\n"launches": [\n')
        f.write(",\n".join(json.dumps(x, separators=(",", ":")) for x in seq))
        f.write("\n]}\n")
    print(f"{sum(x[0] for x in seq)} conv launches of {len(kernels)} kernels, {len(seq)} runs -> {dest}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--list":
        listing(sys.argv[2], sys.argv[3])
    else:
        launches()
