"""Edge geometries for the conv engines, plain helper: no pytest, no GPU.

The conv tests elsewhere hold every plan to its precision on a few model-like shapes.  This module holds what a test needs to hold every
plan to its *geometry*: ragged last tiles, halos wider than the map, the pixel -> (n, y, x) split across many images, parity under
stride 2, padding other than "same", kernels with R != S, input widths below one K step.

* the table of cases (CASES), each in one hazard class (CLASSES), and their seeded inputs (unit-normal activations, He-scaled weights);
* ``reference(case, ...)``: the whole operation (optional x2 bilinear upsample, conv, folded BN and bias, residual, activation) in float64
  on the CPU with torch's own conv, NHWC; with ``defect=`` one of five value-only models of the indexing bugs the table is there to catch,
  computed by an explicit tap loop (which, without a defect, is a second statement of the reference);
* ``plans(case, engine, math)``: the pinned plans of an engine -- every id of the library's plan table, found by walking it, and the
  split-K pairs of the older tests -- and ``verdict(...)``: what arseg_conv_plan_query says about the descriptor ops.conv2d launches for one;
* ``routes(case, engine, math)``: the routes above the engines (Winograd, the LDS-DMA GEMMs, the tap decomposition, up_3's kernel), which have
  no query: their eligibility is the host condition of ops/conv.py, restated here;
* ``applies(row, engine, cls)``: in which classes a plan of the table can be accepted at all.

tests/test_conv_geometry.py proves on the CPU that the table has teeth and that the sweep cannot pass vacuously;
tests/test_gpu_conv_geometry.py runs it on the device."""
import collections
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.2
BN_EPS = 1e-5
TOL, TOL_TAPS = 2e-4, 5e-5          # tests/test_gpu_ops.py: test_conv2d / test_conv2d_winograd* and the tap route (absolute)
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}          # tests/test_gpu_16bit.py
EXTRA16 = 2e-5                      # close16(..., extra=2e-5 * max|want|)
SPLIT_K_PAIRS = ((3, 3), (7, 3), (1, 2), (5, 2), (11, 2), (9, 3), (19, 2))          # test_conv2d's pairs (split_accuracy.SPLIT_K_PAIRS)
SPLIT_K16 = ((1, 2), (3, 3), (4, 8))                                                # test_conv2d16's pairs
CLASSES = ("tiny", "dil_gt_map", "thresholds", "m_edges", "many_images", "parity", "padding", "nonsquare", "narrow_k")
DEFECTS = ("clamp_pad", "batch_wrap", "floor_out", "rs_swap", "phase_drop")
ENGINES = ("f32", "f16x3", "fp16", "bf16")          # the fp32 engine under its two maths, the 16-bit engine on its two storage types
DTYPE16 = {"fp16": torch.float16, "bf16": torch.bfloat16}

Case = collections.namedtuple("Case", "id cls N H W Cin Cout R S stride pad dil act bn bias res up2")


def _c(id_, cls, N, H, W, Cin, Cout, R, S, stride, pad, dil, ep="r", up2=False):
    """ep: the epilogue -- "full" = BN + bias + residual + PReLU (one per class at least), "r" BN + ReLU, "n" bias only, "p" BN + bias + PReLU,
    "rr" BN + ReLU + residual"""
    act, bn, bias, res = {"full": ("prelu", True, True, True), "r": ("relu", True, False, False), "n": ("none", False, True, False),
                          "p": ("prelu", True, True, False), "rr": ("relu", True, False, True)}[ep]
    return Case(id_, cls, N, H, W, Cin, Cout, R, S, stride, pad, dil, act, bn, bias, res, up2)


def _table():
    t = []
    # tiny: maps smaller than the kernel's reach; one tile is many times the map.  up2: H x W is the LOW resolution, the conv runs at 2H x 2W
    t += [_c("t11", "tiny", 1, 1, 1, 64, 64, 3, 3, 1, 1, 1, "full"), _c("t17", "tiny", 1, 1, 7, 64, 72, 3, 3, 1, 1, 1, "r"),
          _c("t61", "tiny", 2, 6, 1, 64, 64, 3, 3, 1, 1, 1, "n"), _c("t23", "tiny", 1, 2, 3, 64, 36, 3, 3, 1, 1, 1, "p"),
          _c("t33", "tiny", 1, 3, 3, 32, 64, 3, 3, 1, 1, 1, "rr"),
          _c("ts19", "tiny", 1, 1, 9, 3, 64, 7, 7, 2, 3, 1, "r"), _c("ts46", "tiny", 1, 4, 6, 3, 64, 7, 7, 2, 3, 1, "p"),
          _c("ts77", "tiny", 2, 7, 7, 3, 64, 7, 7, 2, 3, 1, "n"),
          _c("tu11", "tiny", 1, 1, 1, 64, 64, 3, 3, 1, 1, 1, "p", True), _c("tu15", "tiny", 1, 1, 5, 64, 72, 3, 3, 1, 1, 1, "r", True),
          _c("tu41", "tiny", 2, 4, 1, 64, 64, 3, 3, 1, 1, 1, "n", True), _c("tu33", "tiny", 1, 3, 3, 64, 96, 3, 3, 1, 1, 1, "full", True)]
    # dil_gt_map: a dilation larger than the map: Winograd's polyphase sub-images without rows or columns, patch halos beyond the LDS budget
    t += [_c("d35", "dil_gt_map", 2, 3, 5, 64, 64, 3, 3, 1, 4, 4, "full"), _c("d44", "dil_gt_map", 1, 4, 4, 64, 72, 3, 3, 1, 4, 4, "r"),
          _c("d29", "dil_gt_map", 1, 2, 9, 64, 64, 3, 3, 1, 4, 4, "n"), _c("d13", "dil_gt_map", 2, 1, 3, 64, 64, 3, 3, 1, 2, 2, "p"),
          _c("d52", "dil_gt_map", 2, 5, 2, 64, 36, 3, 3, 1, 2, 2, "rr")]
    # thresholds: conv_patch_tile changes the tile width at Wo = 24 and 48, the patch heights are 2 / 4 / 8 / 16, Winograd's tiles 4 x 4
    for i, (h, w) in enumerate(((3, 23), (5, 24), (9, 24), (17, 25), (3, 47), (5, 48), (9, 48), (17, 49), (3, 65), (5, 65), (9, 47), (17, 23))):
        t.append(_c(f"h{h}x{w}", "thresholds", 1, h, w, 64, 136 if i in (2, 7) else 64, 3, 3, 1, 1, 1, ("full", "r", "n", "p")[i % 4]))
    # ... and the stem kernel's 8 x 32 output tiles: outputs (8, 32), (9, 33), (1, 1)
    t += [_c("hs16x64", "thresholds", 1, 16, 64, 3, 64, 7, 7, 2, 3, 1, "r"), _c("hs17x65", "thresholds", 1, 17, 65, 3, 64, 7, 7, 2, 3, 1, "p"),
          _c("hs1x1", "thresholds", 1, 1, 1, 3, 64, 7, 7, 2, 3, 1, "n")]
    # m_edges: M = N Ho Wo one below, at and one above every pixel tile; the channel counts are the tails against every channel tile
    maps = ((63, 1, 7, 9), (64, 1, 8, 8), (65, 1, 5, 13), (127, 1, 1, 127), (128, 2, 8, 8), (129, 3, 1, 43), (255, 1, 15, 17), (256, 1, 16, 16),
            (257, 1, 1, 257))
    for i, (m, n, h, w) in enumerate(maps):
        t.append(_c(f"m{m}k1", "m_edges", n, h, w, 64, (4, 10, 60, 68, 132, 260, 68, 260, 132)[i], 1, 1, 1, 0, 1, ("n", "rr", "p", "full", "r")[i % 5]))
        t.append(_c(f"m{m}k3", "m_edges", n, h, w, 64, (60, 68, 4, 10, 260, 132, 10, 60, 4)[i], 3, 3, 1, 1, 1, ("full", "r", "n", "p", "rr")[i % 5]))
    # many_images: one 128- / 256-pixel tile spans 4 to 8 images of 35 pixels
    t += [_c("n9s1", "many_images", 9, 5, 7, 64, 64, 3, 3, 1, 1, 1, "full"), _c("n9s2", "many_images", 9, 5, 7, 64, 72, 3, 3, 2, 1, 1, "p"),
          _c("n9d2", "many_images", 9, 5, 7, 64, 64, 3, 3, 1, 2, 2, "rr"), _c("n9k1", "many_images", 9, 5, 7, 64, 68, 1, 1, 1, 0, 1, "n"),
          _c("n5u", "many_images", 5, 2, 3, 64, 64, 3, 3, 1, 1, 1, "r", True)]
    # parity: stride 2 on every parity of H and W, down to one pixel
    t += [_c("p8x10", "parity", 2, 8, 10, 64, 64, 3, 3, 2, 1, 1, "full"), _c("p9x10", "parity", 1, 9, 10, 64, 72, 3, 3, 2, 1, 1, "r"),
          _c("p8x11", "parity", 1, 8, 11, 64, 64, 3, 3, 2, 1, 1, "n"), _c("p2x2", "parity", 1, 2, 2, 64, 64, 3, 3, 2, 1, 1, "p"),
          _c("p1x1", "parity", 2, 1, 1, 64, 64, 3, 3, 2, 1, 1, "rr"),
          _c("pk1x1", "parity", 1, 1, 1, 64, 68, 1, 1, 2, 0, 1, "n"), _c("pk2x3", "parity", 2, 2, 3, 64, 68, 1, 1, 2, 0, 1, "rr"),
          _c("pk7x8", "parity", 1, 7, 8, 64, 68, 1, 1, 2, 0, 1, "p"),
          _c("ps8x11", "parity", 1, 8, 11, 3, 64, 7, 7, 2, 3, 1, "r"), _c("ps9x10", "parity", 2, 9, 10, 3, 64, 7, 7, 2, 3, 1, "p")]
    # padding: none, more than "same" (the output is larger than the input), and on a 1x1 (the border is pure epilogue)
    t += [_c("z3x3", "padding", 1, 3, 3, 64, 64, 3, 3, 1, 0, 1, "r"), _c("z5x9", "padding", 2, 5, 9, 64, 72, 3, 3, 1, 0, 1, "full"),
          _c("z2big", "padding", 1, 4, 6, 64, 64, 3, 3, 1, 2, 1, "p"), _c("zk1", "padding", 2, 3, 5, 64, 68, 1, 1, 1, 1, 1, "full")]
    # nonsquare: R != S (the K order is (r * S + s) * Cin + ci)
    t += [_c("q1x3", "nonsquare", 2, 5, 7, 64, 64, 1, 3, 1, 1, 1, "full"), _c("q3x1", "nonsquare", 1, 5, 7, 64, 72, 3, 1, 1, 1, 1, "r"),
          _c("q1x7", "nonsquare", 1, 4, 9, 64, 64, 1, 7, 1, 1, 1, "n"), _c("q1x3s2", "nonsquare", 2, 6, 9, 64, 68, 1, 3, 2, 1, 1, "p")]
    # narrow_k: input widths below one K step (3 is padded), and 1x1 convs whose K is no multiple of it
    t += [_c(f"k3c{ci}", "narrow_k", 2, 6, 10, ci, (64, 72, 64, 36)[i], 3, 3, 1, 1, 1, ("r", "full", "n", "p")[i]) for i, ci in enumerate((3, 4, 8, 16))]
    t += [_c(f"k1c{ci}", "narrow_k", 1, 5, 7, ci, (10, 68, 64)[i], 1, 1, 1, 0, 1, ("n", "full", "rr")[i]) for i, ci in enumerate((4, 36, 100))]
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def of_class(cls):
    return [c for c in CASES if c.cls == cls]


def conv_hw(c):
    """the size of the conv's input"""
    return (2 * c.H, 2 * c.W) if c.up2 else (c.H, c.W)


def out_hw(c, ceil=False):
    H, W = conv_hw(c)
    f = lambda v, k: (v + 2 * c.pad - c.dil * (k - 1) - 1 + (c.stride - 1 if ceil else 0)) // c.stride + 1      # noqa: E731
    return f(H, c.R), f(W, c.S)


def is_stem(c):
    return (c.R, c.S, c.stride, c.pad, c.dil, c.Cin, c.Cout) == (7, 7, 2, 3, 1, 3, 64)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rnd(c, item, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64([ord(ch) for ch in c.id] + [item]))
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """x NHWC [N, H, W, Cin], w OIHW (He-scaled), bn (gamma, beta, mean, var) or None, b or None, res NHWC or None: float32 CPU tensors, shared,
    never written."""
    c = BY_ID[case_id]
    g = np.random.Generator(np.random.PCG64([ord(ch) for ch in c.id] + [9]))
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))      # noqa: E731
    Ho, Wo = out_hw(c)
    return {"x": _rnd(c, 0, c.N, c.H, c.W, c.Cin),
            "w": _rnd(c, 1, c.Cout, c.Cin, c.R, c.S, scale=float(np.sqrt(2.0 / (c.Cin * c.R * c.S)))),
            "bn": (f32(g.uniform(0.5, 1.5, c.Cout)), _rnd(c, 2, c.Cout, scale=0.1), _rnd(c, 3, c.Cout, scale=0.1), f32(g.uniform(0.5, 1.5, c.Cout))) if c.bn else None,
            "b": _rnd(c, 4, c.Cout, scale=0.1) if c.bias else None,
            "res": _rnd(c, 5, c.N, Ho, Wo, c.Cout) if c.res else None}


def operands(case_id, dtype=None):
    """The operands as the engine sees them, float64: dtype None = fp32 storage; a 16-bit dtype = x, w and the residual rounded to it (BN and
    bias stay fp32 in the epilogue) -> (x NHWC, w OIHW, res NHWC or None)"""
    ins = inputs(case_id)
    r = (lambda v: v.double()) if dtype is None else (lambda v: v.to(dtype).double())
    return r(ins["x"]), r(ins["w"]), None if ins["res"] is None else r(ins["res"])


# ---------------------------------------------------------------------------------------------------------------- reference
def _finish(y, c, res):
    """conv result NCHW float64 -> folded BN and bias, residual (NHWC), activation -> NHWC"""
    ins = inputs(c.id)
    scale, shift = torch.ones(c.Cout, dtype=torch.float64), torch.zeros(c.Cout, dtype=torch.float64)
    if ins["b"] is not None:
        shift = ins["b"].double()
    if ins["bn"] is not None:
        gamma, beta, mean, var = (v.double() for v in ins["bn"])
        scale = gamma / torch.sqrt(var + BN_EPS)
        shift = beta + (shift - mean) * scale
    y = (y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res
    if c.act == "relu":
        y = F.relu(y)
    elif c.act == "prelu":
        y = torch.where(y >= 0, y, SLOPE * y)
    return y.contiguous()


def _tap_conv(x, w, c, defect=None, guard=float("nan")):
    """The conv as an explicit loop over its taps, x NCHW / w OIHW float64 -> NCHW: out[oy, ox] += w[r, s] . x[oy * stride - pad + r * dil, ...].
    defect None: the conv itself.  The defects change which input value, weight or output position a tap uses, never the arithmetic:

    clamp_pad   a tap outside the image reads the clamped border pixel instead of zero;
    batch_wrap  a tap one row above (below) image n reads the last (first) row of image n - 1 (n + 1) -- the flat index (n * H + y) * W + x with
                y = -1 or H; before image 0 and after image N - 1 lies ``guard`` (NaN: the guard images of the GPU test; 0.0: what a caching
                allocator usually leaves there);
    floor_out   Ho, Wo are rounded up instead of down under stride 2 and the output is written at the flat index of that larger grid: returned
                is what lands in the [N, Ho, Wo] tensor (what falls behind it is a write outside the tensor, which values cannot show);
    rs_swap     the weight of tap (r, s) is taken from K position s * R + r instead of r * S + s;
    phase_drop  (stride 1, pad == dil) a polyphase sub-image sy >= H or sx >= W, which has no rows or columns, is treated as having one: its phantom
                row y = sy lands at the flat row n * H + y, i.e. in the next image (and a phantom column in the next row); every tap of a
                phantom pixel is out of bounds, so it stores a zero sum."""
    N, C, H, W = x.shape
    Ho, Wo = out_hw(c, ceil=defect == "floor_out")
    if defect == "rs_swap":
        flat = w.reshape(c.Cout, C, c.R * c.S)
        w = torch.stack([torch.stack([flat[:, :, (s * c.R + r) % (c.R * c.S)] for s in range(c.S)], dim=-1) for r in range(c.R)], dim=-2)
    out = torch.zeros(N, c.Cout, Ho, Wo, dtype=torch.float64)
    oy, ox = torch.arange(Ho) * c.stride - c.pad, torch.arange(Wo) * c.stride - c.pad
    if defect == "batch_wrap":
        outer = torch.full((1, C, H, W), guard, dtype=torch.float64)
        rows = torch.cat([outer, x, outer]).permute(1, 0, 2, 3).reshape(C, (N + 2) * H, W)          # every image row of the buffer, guards included
    for r in range(c.R):
        iy = oy + r * c.dil
        for s in range(c.S):
            ix = ox + s * c.dil
            vy, vx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            xs = x[:, :, iy.clamp(0, H - 1)][:, :, :, ix.clamp(0, W - 1)]
            if defect == "batch_wrap":
                wrap = (iy == -1) | (iy == H)
                flat_row = (torch.arange(N).view(N, 1) + 1) * H + iy.clamp(-1, H).view(1, Ho)                      # [N, Ho] rows of the guarded buffer
                xs = torch.where((vy | wrap).view(1, 1, Ho, 1), rows[:, flat_row][:, :, :, ix.clamp(0, W - 1)].permute(1, 0, 2, 3), xs)
                vy = vy | wrap
            if defect != "clamp_pad":
                xs = torch.where((vy.view(Ho, 1) & vx.view(1, Wo)).view(1, 1, Ho, Wo), xs, torch.zeros((), dtype=torch.float64))
            out = out + torch.einsum("nchw,oc->nohw", xs, w[:, :, r, s])
    if defect == "floor_out":
        Hf, Wf = out_hw(c)
        out = out.permute(0, 2, 3, 1).reshape(-1, c.Cout)[:N * Hf * Wf].reshape(N, Hf, Wf, c.Cout).permute(0, 3, 1, 2)
    if defect == "phase_drop" and c.stride == 1 and c.pad == c.dil and c.R == 3 and c.S == 3:
        flat = out.permute(0, 2, 3, 1).reshape(N * H * W, c.Cout).clone()
        for n in range(N):
            for y in range(max(H, 1), c.dil):                     # phantom rows of the sub-images sy >= H
                for xx in range(W):
                    if (n * H + y) * W + xx < flat.shape[0]:
                        flat[(n * H + y) * W + xx] = 0.0
            for y in range(H):
                for xx in range(W, c.dil):                        # phantom columns of the sub-images sx >= W
                    if (n * H + y) * W + xx < flat.shape[0]:
                        flat[(n * H + y) * W + xx] = 0.0
        out = flat.reshape(N, H, W, c.Cout).permute(0, 3, 1, 2)
    return out


def reference(case_id, dtype=None, conv_input=None, defect=None, guard=float("nan")):
    """The whole operation in float64 on the CPU -> NHWC.  dtype: the storage type whose rounded operands it runs on (None: fp32).
    conv_input: the conv's NHWC input where it is not the (upsampled) ``x`` -- the 16-bit path rounds the materialised upsample to 16 bits, so
    its reference runs on that tensor, as tests/test_gpu_conv_views.py does.  defect: see _tap_conv."""
    c = BY_ID[case_id]
    x, w, res = operands(case_id, dtype)
    xin = (x if conv_input is None else conv_input.detach().cpu().double()).permute(0, 3, 1, 2)
    if c.up2 and conv_input is None:
        xin = F.interpolate(xin, scale_factor=2.0, mode="bilinear", align_corners=False)
    y = F.conv2d(xin, w, None, c.stride, c.pad, c.dil) if defect is None else _tap_conv(xin, w, c, defect, guard)
    return _finish(y, c, res)


@functools.lru_cache(maxsize=None)
def want(case_id, dtype=None):
    """reference(case, dtype): computed once, shared, never written"""
    return reference(case_id, dtype)


def tol16(w64, dtype):
    """the elementwise bound of close16(got, want, dtype, extra=2e-5 * max|want|)"""
    return ULP[dtype] * 0.51 * w64.abs() + EXTRA16 * float(w64.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------------------------- plans and verdicts
def engine_of(name):
    from arseg_amd import _lib

    return _lib.CONV_ENGINE_16 if name in DTYPE16 else _lib.CONV_ENGINE_F32


def math_of(name):
    from arseg_amd import _lib

    return _lib.MATH_F16X3 if name == "f16x3" else _lib.MATH_F32


@functools.lru_cache(maxsize=None)
def table_ids(engine):
    """every id of an engine's plan table: walked until the first number that is no id"""
    from arseg_amd import _lib

    ids = []
    while _lib.conv_plan_row(engine, len(ids)).kind != _lib.PLAN_NONE:
        ids.append(len(ids))
    return tuple(ids)


def plans(name):
    """The pinned (tile_cfg, split_k) of engine ``name``.  fp32 engine: id 0 as (0, 0) (the library's heuristic: launched with the tuner off),
    every other id with split_k 1, then test_conv2d's split-K pairs.  16-bit engine: every id with split_k 0 (a set split_k keeps
    ops.conv2d off the fused upsample), then test_conv2d16's pairs."""
    if name in DTYPE16:
        return [(cfg, 0) for cfg in table_ids(engine_of(name))] + list(SPLIT_K16)
    return [(0, 0)] + [(cfg, 1) for cfg in table_ids(engine_of(name))[1:]] + list(SPLIT_K_PAIRS)


def cin_pad(c, name):
    g = 8 if name in DTYPE16 else 4
    return (c.Cin + g - 1) // g * g


def fused_up2(c, name, cfg, sk, in_ld):
    """Does ops.conv2d hand plan (cfg, sk) the half-resolution input with upsample2x set?  (Any other plan runs on the materialised upsample.)"""
    from arseg_amd import _lib

    if not c.up2:
        return False
    fuses = bool(_lib.conv_plan_row(engine_of(name), cfg).fuses_upsample)
    if name not in DTYPE16:
        return fuses
    fusable = (c.R, c.S, c.stride, c.pad, c.dil) == (3, 3, 1, 1, 1) and cin_pad(c, name) % 64 == 0 and in_ld % 8 == 0      # ops.conv._up2_fusable
    return not sk and (cfg == 0 or fuses) and fusable


def launch_desc(c, name, cfg, sk, in_ld=None, out_ld=None, res_ld=None):
    """The descriptor ops.conv2d launches for a pinned plan of engine ``name``; in_ld / out_ld / res_ld: the row pitches of the call's views
    (default: dense fp32 rows, 16-bit output rows padded to 8 channels)."""
    from arseg_amd import _lib

    cp = cin_pad(c, name)
    dense_out = c.Cout if name not in DTYPE16 else (c.Cout + 7) // 8 * 8
    in_ld = cp if in_ld is None else in_ld
    up = fused_up2(c, name, cfg, sk, in_ld)
    d = _lib.ConvDesc()
    d.N = c.N
    d.H, d.W = conv_hw(c)
    d.Cin, d.in_ld = cp, (in_ld if up or not c.up2 else cp)          # (a materialised upsample has dense rows)
    d.Cout, d.out_ld, d.res_ld = c.Cout, out_ld or dense_out, res_ld or out_ld or dense_out
    d.R, d.S, d.stride, d.pad, d.dil = c.R, c.S, c.stride, c.pad, c.dil
    d.tile_cfg, d.split_k, d.math, d.upsample2x = cfg, sk, math_of(name), 1 if up else 0
    return d


def verdict(c, name, cfg, sk, **ld):
    """(accepted?, arseg_conv_plan_info) of the library's device-free query on that descriptor"""
    from arseg_amd import _lib

    info = _lib.ConvPlanInfo()
    st = _lib.load().arseg_conv_plan_query(engine_of(name), ctypes.byref(launch_desc(c, name, cfg, sk, **ld)), ctypes.byref(info))
    assert st in (_lib.ARSEG_OK, _lib.ARSEG_EUNSUPPORTED, _lib.ARSEG_EINVAL), (c.id, name, cfg, sk, st)
    return st == _lib.ARSEG_OK, info


# The one statement of where a plan of the table can be accepted at all, by its kind and the class's cases:
PATCH_CLASSES = ("tiny", "dil_gt_map", "thresholds", "m_edges", "many_images")     # hold a 3x3 stride-1 pad == dil conv on 64 input channels
FORCED_TW_CLASSES = ("thresholds", "m_edges")     # ... on a map of 24 (48) columns or more, below which a forced 16 (32) wide tile is the default one
STEM_CLASSES = ("tiny", "thresholds", "parity")   # hold a 7x7 stride-2 pad-3 conv of padded RGB to 64 channels
UP2_C64_CLASSES = ("tiny", "many_images")         # hold a 64 -> 64 conv after a x2 upsample without a residual


def applies(name, cfg, sk, cls):
    """Can plan (cfg, sk) of engine ``name`` be accepted by some case of class ``cls``?"""
    from arseg_amd import _lib

    row = _lib.conv_plan_row(engine_of(name), cfg)
    if sk > 1 and not row.split_k_allowed:
        return False
    if name == "f32" and row.kind in (_lib.PLAN_TILE_WIDE, _lib.PLAN_PATCH, _lib.PLAN_UP2_C64):          # the f16x3-only ids of the fp32 engine
        return False
    if row.kind == _lib.PLAN_PATCH:
        forced = not verdict(BY_ID["h3x23"], name, cfg, sk)[0]          # (on 23 columns, the narrowest default tile, exactly the forced widths refuse)
        return cls in (FORCED_TW_CLASSES if forced else PATCH_CLASSES)
    if row.kind == _lib.PLAN_STEM:
        return cls in STEM_CLASSES
    if row.kind == _lib.PLAN_UP2_C64:
        return cls in UP2_C64_CLASSES
    return True


# ---------------------------------------------------------------------------------------------------------------- routes above the engines
WINO_GEMMS = (7, 100)          # the batched GEMM of the Winograd route: implicit-GEMM tile 7, gemm_x3 tile 0
X3_CFGS = tuple(range(7))
ROWS16_CFGS = tuple(range(12))
UP2_C64_WGS = (0, 3)


def has_wino(c):
    """packing.PackedConv builds Winograd weights (pc.wino_u is not None)"""
    return c.R == 3 and c.S == 3 and c.stride == 1 and c.pad == c.dil and c.Cin % 32 == 0 and c.Cin >= 64 and c.Cout % 4 == 0


def routes(c, name):
    """The labels of the routes eligible for case ``c`` under engine ``name`` (the host conditions of ops/conv.py); within them a refusal is a
    failure.  "wino:G", "x3:C", "taps", "up2_c64:W" (fp32 storage), "rows16:C" (16-bit storage)."""
    out = []
    if name in DTYPE16:
        if (c.R, c.S, c.stride, c.pad) == (1, 1, 1, 0) and c.Cin % 64 == 0 and c.Cout % 4 == 0:
            out += [f"rows16:{cfg}" for cfg in ROWS16_CFGS]
        return out
    if has_wino(c):
        out += [f"wino:{g}" for g in WINO_GEMMS if g < 100 or name == "f16x3"]
    if name == "f16x3" and (c.R, c.S, c.stride, c.pad) == (1, 1, 1, 0) and c.Cin % 32 == 0 and c.Cout % 4 == 0:
        out += [f"x3:{cfg}" for cfg in X3_CFGS]
    if c.up2 and not c.res and c.Cout % 4 == 0:
        out.append("taps")
    if name == "f16x3" and c.up2 and not c.res and c.Cin == 64 and c.Cout == 64:
        out += [f"up2_c64:{w}" for w in UP2_C64_WGS]
    return out


def route_tol(label):
    return TOL_TAPS if label == "taps" else TOL
