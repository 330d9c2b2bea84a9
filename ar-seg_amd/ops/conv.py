"""The conv engine's host side: route and plan selection per layer shape (implicit GEMM / patch-resident 3x3 / Winograd / tap
decomposition / LDS-DMA GEMM on split rows), the split-row activation carrier, the 16-bit storage path, the folded PSP bottleneck."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _lib
from .._lib import ConvDesc, check
from ._base import RANGE_LIMIT, _arm_range_watch, _need_gpu, _need_gpu16, _nhwc_ld, _ptr, _range_word, _stream, is16, workspace
from ._config import config, set_conv_math, sw
from ._plans import _tune_conv, fuses_up2, tuned
from ._profile import launch, tagged
from .layers import psp_prior_sum, resize_nhwc


class SplitRows:
    """An NHWC activation tensor stored as split rows -- per 32 channels 32 hi fp16 halves then 32 lo halves, the operand format of
    arseg_gemm_x3_fwd (include/arseg_hip.h) -- in a float32-typed buffer ``t`` of the logical shape (the same 4 bytes per value).
    Produced by ``conv2d(..., out_split=True)`` / ``split_rows``; consumed by ``conv2d`` (1x1 convs and the tap-decomposed conv after a
    x2 upsample).  ``float()`` gives the fp32 tensor back (torch ops on the device; only fallback paths need it)."""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    shape = property(lambda self: self.t.shape)
    device = property(lambda self: self.t.device)

    def float(self):
        n, h, w, c = self.t.shape
        hl = self.t.view(torch.float16).view(n, h, w, c // 32, 2, 32).float()
        return (hl[..., 0, :] + hl[..., 1, :]).reshape(n, h, w, c)


_ROWS_CFGS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)


def gemm_rows16(x: torch.Tensor, pc, residual=None, out: Optional[torch.Tensor] = None, cfg: Optional[int] = None, record: bool = True):
    """1x1 stride-1 conv of the 16-bit storage path as a plain GEMM of the LDS-DMA kernel (arseg_gemm_rows16_fwd): x NHWC fp16 / bf16 with dense
    rows (Cin % 64 == 0), 16-bit output (may be a channel slice).  cfg None: the tile shape is timed on first use per (M, K, N)."""
    lib = _lib.load()
    dt = _need_gpu16(x, residual, out)
    n, h, w, cin = x.shape
    w16, cin16 = pc.weights16(x.dtype)
    if cin != cin16 or cin % 64 or _nhwc_ld(x) != cin or pc.R != 1 or pc.S != 1 or pc.stride != 1 or pc.pad != 0 or pc.cout % 4:
        raise _lib.ArsegError("gemm_rows16: a 1x1 stride-1 conv on dense 16-bit rows with Cin % 64 == 0 and Cout % 4 == 0 is required")
    M, cout = n * h * w, pc.cout
    if out is None:
        out = torch.empty((n, h, w, (cout + 7) // 8 * 8), dtype=x.dtype, device=x.device)[..., :cout]
    elif tuple(out.shape) != (n, h, w, cout):
        raise _lib.ArsegError(f"conv out has shape {tuple(out.shape)}, expected {(n, h, w, cout)}")
    if residual is not None and tuple(residual.shape) != (n, h, w, cout):
        raise _lib.ArsegError("residual shape mismatch")
    flops = 2 * M * cin * cout

    def run(c, record=True):
        launch("conv2d", lib.arseg_gemm_rows16_fwd, _ptr(x), _ptr(w16), _ptr(out), dt, M, cin, cout, _nhwc_ld(out), _ptr(pc.scale), _ptr(pc.bias),
               _ptr(residual), _nhwc_ld(residual) if residual is not None else 0, pc.act, pc.slope, c, _stream(), flops=flops, record=record)

    if cfg is None:
        key = ("gemm16", x.device.index, dt, M, cin, cout, residual is not None)
        cfg = tuned(key, _ROWS_CFGS, lambda c: run(c, False), untuned=9 if cout <= 64 else 3)
        if cfg is None:          #  every tile refused the shape: the caller keeps its other plan
            raise _lib.ArsegError(f"gemm_rows16: no tile configuration accepts M={M} K={cin} N={cout}")
    with tagged(lambda: (n, h, w, pc.cin, cout, 1, 1, 1, False, f"gemm16({cfg})", flops)):
        run(cfg, record)
    return out


def gemm_x3_enabled() -> bool:
    return sw.GEMM_X3 is True and sw.math == _lib.MATH_F16X3 and not sw.RANGE_GUARD


def split_rows(x: torch.Tensor) -> SplitRows:
    """fp32 NHWC [N,H,W,C] (C % 32 == 0; may be a channel slice) -> SplitRows: one memory-bound pass (arseg_split_rows_fwd) that also
    carries the operand range watch of the GEMM that will consume it."""
    _need_gpu(x)
    n, h, w, c = x.shape
    t = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    rw = _range_word(x.device) if sw.RANGE_MODE == "device" else None
    launch("split_rows", _lib.load().arseg_split_rows_fwd, _ptr(x), _nhwc_ld(x), _ptr(t), n * h * w, c, 1.0, _ptr(rw), 65504.0, _stream())
    return SplitRows(t)


def _x3_eligible(pc, cin, residual, up2) -> bool:
    return (gemm_x3_enabled() and not up2 and pc.R == 1 and pc.S == 1 and pc.stride == 1 and pc.pad == 0 and cin % 32 == 0 and cin == pc.cin_pad
            and pc.cout % 4 == 0)


def _conv1x1_x3(x, pc, residual=None, out=None, out_split=False, cfg=None, record=True):
    """1x1 stride-1 conv on the LDS-DMA GEMM (csrc/gemm_x3.hip).  x: SplitRows, or fp32 NHWC (split by a pre-pass first).  cfg None: the
    tile shape is timed on first use per (M, K, N)."""
    lib = _lib.load()
    xs = x if isinstance(x, SplitRows) else split_rows(x)
    N, H, W, Cin = xs.shape
    M, Cout, dev = N * H * W, pc.cout, xs.device
    if out_split and Cout % 32:
        out_split = False                    # split rows come in groups of 32 channels: such a layer writes plain fp32
    if out_split:
        out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=dev)
    elif out is None:
        out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=dev)
    rw = _range_word(dev) if (out_split and sw.RANGE_MODE == "device") else None

    def run(c, record=True):
        launch("conv2d", lib.arseg_gemm_x3_fwd, _ptr(xs.t), _ptr(pc.w_h3), _ptr(out), M, Cout, Cin, Cout if out_split else _nhwc_ld(out), 1, 0, 0, 0,
               _ptr(pc.scale_h3), _ptr(pc.bias), _ptr(residual), _nhwc_ld(residual) if residual is not None else 0, pc.act, pc.slope,
               1 if out_split else 0, c, _ptr(rw), 65504.0, _stream(), flops=2 * M * Cin * Cout, record=record)

    if cfg is None:
        key = ("x3", dev.index, M, Cin, Cout, bool(out_split), residual is not None)
        cfg = tuned(key, range(7), lambda c: run(c, False), untuned=-1)
        if cfg is None:
            raise _lib.ArsegError(f"gemm_x3: no tile configuration accepts M={M} K={Cin} N={Cout}")
    if cfg == -1:
        # un-timed (tuner off / graph capture): the first tile shape the problem admits; the last one raises its own error (cfg 0
        # alone raised for a shape it rejects although another tile takes it)
        for c in range(6):
            try:
                run(c, record)
                return SplitRows(out) if out_split else out
            except _lib.ArsegError:
                pass
        cfg = 6
    run(cfg, record)
    return SplitRows(out) if out_split else out


def conv2d(x: torch.Tensor, pc, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           tile_cfg: int = 0, split_k: int = 0, up2: bool = False, out_split: bool = False):
    """x NHWC [N,H,W,Cin_pad] (may be a channel slice); pc: packing.PackedConv; out: optional NHWC (slice) view.
    tile_cfg / split_k: 0 = use the cached per-shape plan (autotuned on first use).
    up2: the conv input is the x2 bilinear (align_corners=False) upsample of ``x`` (PSPUpsample, model/pspnet.py:43-46);
    the Winograd route applies it inside its input transform, the patch-resident direct plans while they stage their input patch;
    the GEMM-tile plans materialise it first."""
    if isinstance(x, SplitRows):
        # an activation the producer already wrote as split rows: 1x1 convs go straight to the LDS-DMA GEMM, a 3x3 conv after a x2 upsample
        # to its tap decomposition (whose low-resolution 1x1 conv is such a GEMM); anything else reads the fp32 form
        n_, h_, w_, c_ = x.shape
        if not up2 and _x3_eligible(pc, c_, residual, False):
            return _conv1x1_x3(x, pc, residual, out, out_split)
        if (up2 and gemm_x3_enabled() and sw.UP2_TAPS and residual is None and pc.R == 3 and pc.S == 3 and pc.stride == 1 and pc.pad == 1 and pc.dil == 1
                and pc.cout % 4 == 0 and c_ % 32 == 0):
            split_out = out_split and out is None and pc.cout % 32 == 0      # (the next layer is again a tap-decomposed upsample conv)
            if out is None:
                out = torch.empty((n_, 2 * h_, 2 * w_, pc.cout), dtype=torch.float32, device=x.device)
            with tagged((n_, 2 * h_, 2 * w_, pc.cin, pc.cout, pc.R, pc.stride, pc.dil, True, "taps(x3)", 2 * n_ * 4 * h_ * w_ * pc.cout * 9 * pc.cin)):
                _conv_up2_taps(x, pc, out, True, split_out)
            return SplitRows(out) if split_out else out
        return conv2d(x.float(), pc, residual, out, tile_cfg, split_k, up2, out_split)
    if is16(x):
        return _conv2d16(x, pc, residual, out, up2, tile_cfg, split_k)
    _need_gpu(x, residual, out)
    if out_split and tile_cfg == 0 and split_k == 0 and out is None and _x3_eligible(pc, x.shape[3], residual, up2) and pc.cout % 32 == 0:
        # the consumer takes split rows (e.g. the PSP bottleneck feeding up_1): this conv runs on the LDS-DMA GEMM and writes them
        n_, h_, w_, c_ = x.shape
        with tagged((n_, h_, w_, pc.cin, pc.cout, 1, 1, 1, False, "x3(split out)", 2 * n_ * h_ * w_ * pc.cout * pc.cin)):
            return _conv1x1_x3(x, pc, residual, None, True)
    if sw.RANGE_GUARD and sw.math == _lib.MATH_F16X3 and not (float(x.abs().max()) <= RANGE_LIMIT):      # (NaN compares false)
        prev = set_conv_math("f32")
        try:
            return conv2d(x, pc, residual, out, 0, 0, up2)
        finally:
            set_conv_math(prev)
    x_low = None
    if up2:
        x_low = x
        n_, h_, w_, c_ = x.shape
        if (tile_cfg and not fuses_up2(tile_cfg)) or (not tile_cfg and (split_k or not sw.AUTOTUNE)):
            x, x_low = resize_nhwc(x, 2 * h_, 2 * w_, _lib.BILINEAR, False), None          # explicit GEMM tile / heuristic plan: materialise
        else:
            # shape carrier; filled only if a plan without a fused upsample is chosen (the patch-resident plans and the Winograd
            # route interpolate while they stage their input)
            x = torch.empty((n_, 2 * h_, 2 * w_, c_), dtype=x.dtype, device="meta")
    dev = x_low.device if x_low is not None else x.device
    N, H, W, Cin = x.shape
    if Cin != pc.cin_pad:
        raise _lib.ArsegError(f"conv expects {pc.cin_pad} input channels (padded), got {Cin}")
    in_ld_hi = Cin if x_low is not None else _nhwc_ld(x)
    math = sw.math
    d, out, Ho, Wo = _conv_desc(pc, N, H, W, Cin, in_ld_hi, tile_cfg, split_k, residual, out, torch.float32, dev, math,
                                up2=x_low is not None and fuses_up2(tile_cfg))
    w_dev, scale_dev = (pc.w_h3, pc.scale_h3) if math != _lib.MATH_F32 else (pc.w, pc.scale)
    lib = _lib.load()
    flops = 2 * N * Ho * Wo * pc.cout * pc.R * pc.S * pc.cin

    up_buf = []

    def run(plan, record=True):
        """Launch any plan: a (tile_cfg, split_k) pair of arseg_conv2d_fwd, or the route "wino", "x3" or "taps"."""
        if plan == "wino":
            return _conv_wino(x if x_low is None else x_low, pc, residual, out, N, H, W, record, up2=x_low is not None)
        if plan == "x3":
            return _conv1x1_x3(x, pc, residual, out, False, None, record)
        if plan == "taps":
            return _conv_up2_taps(x_low, pc, out, record)
        cfg, sk = plan
        xin = x
        d.upsample2x, d.in_ld = 0, in_ld_hi
        if x_low is not None:
            if fuses_up2(cfg):                                  # the patch-resident kernel upsamples while it stages its patch
                xin, d.upsample2x, d.in_ld = x_low, 1, _nhwc_ld(x_low)
            else:                                               # GEMM kernel on an upsampled input: materialise it
                if not up_buf:
                    up_buf.append(torch.empty((N, H, W, Cin), dtype=torch.float32, device=x_low.device))
                xin = resize_nhwc(x_low, H, W, _lib.BILINEAR, False, out=up_buf[0])
        d.tile_cfg, d.split_k = cfg, sk
        nbytes = lib.arseg_conv2d_workspace_bytes(ctypes.byref(d))
        ws = workspace(nbytes, out.device) if nbytes else None
        launch("conv2d", lib.arseg_conv2d_fwd, ctypes.byref(d), _ptr(xin), _ptr(w_dev), _ptr(scale_dev), _ptr(pc.bias), _ptr(residual), _ptr(out),
               _ptr(ws), nbytes, _stream(), flops=flops, record=record)

    def quiet(plan):
        run(plan, record=False)

    def find_native():
        """Plan selection inside the library (arseg_conv2d_find: every candidate timed with HIP events, no Python in the loop).  With a
        fused upsample only the patch-resident plans qualify; None = nothing launched."""
        xin = x
        d.upsample2x, d.in_ld = 0, in_ld_hi
        if x_low is not None:
            xin, d.upsample2x, d.in_ld = x_low, 1, _nhwc_ld(x_low)
        nbytes = lib.arseg_conv2d_find_workspace_bytes(ctypes.byref(d))
        ws = workspace(nbytes, out.device) if nbytes else None
        cfg, sk, us = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
        st = lib.arseg_conv2d_find(ctypes.byref(d), _ptr(xin), _ptr(w_dev), _ptr(scale_dev), _ptr(pc.bias), _ptr(residual), _ptr(out), _ptr(ws),
                                   nbytes, 3, ctypes.byref(cfg), ctypes.byref(sk), ctypes.byref(us), _stream())
        d.upsample2x, d.in_ld = 0, in_ld_hi
        if st > 0:
            check(st, "conv2d_find")                                # a HIP error is not "no plan": raise it
        return (cfg.value, sk.value) if st == _lib.ARSEG_OK else None

    if tile_cfg or split_k or not sw.AUTOTUNE:
        run((tile_cfg, split_k))
        return out
    wino_ok = getattr(pc, "wino_u", None) is not None and sw.WINOGRAD
    routes = {"wino": wino_ok, "x3": _x3_eligible(pc, Cin, residual, x_low is not None) and not wino_ok,
              "taps": (x_low is not None and sw.UP2_TAPS and residual is None and pc.R == 3 and pc.S == 3 and pc.stride == 1 and pc.pad == 1
                       and pc.dil == 1 and pc.cout % 4 == 0)}

    def candidates():
        """The library's own pick; the host loop where that launched nothing and, with a fused upsample (the library then times only the
        patch-resident plans), for the GEMM-tile plans on the materialised upsample.  Then each route outside arseg_conv_desc
        that applies, launched once first (which tunes its own GEMM)."""
        base = find_native()
        alt = _tune_conv(quiet, pc, N * Ho * Wo, allow_patch=base is None) if base is None or x_low is not None else None
        direct = [p for p in (base, alt) if p is not None]
        if not direct:
            return
        yield from direct
        for name, ok in routes.items():
            if ok:
                try:
                    quiet(name)
                except _lib.ArsegError:
                    continue                                    # the route does not cover this shape
                yield name

    key = (dev.index, N, H, W, Cin, pc.cout, pc.R, pc.S, pc.stride, pc.pad, pc.dil, x_low is not None, math)
    plan = tuned(key, candidates(), quiet, valid=lambda p: isinstance(p, tuple) or routes.get(p, False), untuned=(0, 0),
                 margin={"wino": float(config.conv_wino_margin)})
    if plan is None:
        # nothing could be launched.  The one shape-independent cause is the 2 GiB limit of the kernels' 32-bit buffer
        # offsets on a large batch: split the batch (as creff does) instead of caching a plan that never ran.
        if N > 1 and x_low is None and max(x.numel(), out.numel()) * 4 >= (1 << 31):
            hN = N // 2
            conv2d(x[:hN], pc, None if residual is None else residual[:hN], out[:hN])
            conv2d(x[hN:], pc, None if residual is None else residual[hN:], out[hN:])
            return out
        plan = (0, 0)                                           # raises the library's own error
    def go(p):
        with tagged((N, H, W, pc.cin, pc.cout, pc.R, pc.stride, pc.dil, x_low is not None, str(p), flops)):
            run(p)

    try:
        go(plan)
    except _lib.ArsegError:
        # the plan key holds the shape, not the alignment / row pitch of `out` and `residual`: a cached route or patch-resident plan that
        # refuses this call's channel-slice view (16-byte stores) gives way to the library's heuristic for this call; the cached plan stays
        if not (isinstance(plan, str) or fuses_up2(plan[0])):
            raise
        go((0, 0))
    return out


def conv_up2_c64(x_low: torch.Tensor, pc, out: Optional[torch.Tensor] = None, max_wgs: int = 0):
    """up_3's persistent kernel by itself (arseg_conv_up2_c64_fwd = tile_cfg 23 of ``conv2d(..., up2=True)``): 3x3 stride-1 pad-1, 64 -> 64
    channels, on the x2 bilinear upsample of ``x_low`` [N,h,w,64], split-fp16 arithmetic whatever the configured conv math.  max_wgs > 0 caps
    the persistent grid (0: one workgroup per compute unit)."""
    _need_gpu(x_low, out)
    n, h, w, c = x_low.shape
    d, out, Ho, Wo = _conv_desc(pc, n, 2 * h, 2 * w, c, _nhwc_ld(x_low), 23, 1, None, out, torch.float32, x_low.device, _lib.MATH_F16X3, up2=True)
    flops = 2 * n * Ho * Wo * pc.cout * 9 * pc.cin
    with tagged((n, Ho, Wo, pc.cin, pc.cout, 3, 1, 1, True, "up2_c64", flops)):
        launch("conv2d", _lib.load().arseg_conv_up2_c64_fwd, ctypes.byref(d), _ptr(x_low), _ptr(pc.w_h3), _ptr(pc.scale_h3), _ptr(pc.bias), _ptr(out),
               max_wgs, _stream(), flops=flops)
    return out


def _conv_desc(pc, N, H, W, Cin, in_ld, tile_cfg, split_k, residual, out, dtype, device, math=_lib.MATH_F32, up2=False):
    """arseg_conv_desc of ``pc`` on an [N, H, W, Cin] input of row pitch ``in_ld``, and its output tensor: ``out`` (shape checked) or a new one
    of ``dtype`` (16-bit: row pitch padded to 8 channels) -> (desc, out, Ho, Wo).  up2: ``tile_cfg`` is a plan that upsamples its
    half-resolution input itself (upsample2x; H, W are the upsampled size).  The engine that stores ``dtype`` gives the size (or its refusal)."""
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.in_ld = N, H, W, Cin, in_ld
    d.Cout = pc.cout
    d.R, d.S, d.stride, d.pad, d.dil = pc.R, pc.S, pc.stride, pc.pad, pc.dil
    d.act, d.prelu_slope = pc.act, pc.slope
    d.tile_cfg, d.split_k = tile_cfg, split_k
    d.math = math
    _arm_range_watch(d, device)
    ld = pc.cout if dtype == torch.float32 else (pc.cout + 7) // 8 * 8
    d.out_ld, d.res_ld = ld, ld               # provisional, for the shape query
    d.upsample2x = 1 if up2 else 0
    info = _lib.conv_plan(_lib.CONV_ENGINE_F32 if dtype == torch.float32 else _lib.CONV_ENGINE_16, d)
    Ho, Wo = info.Ho, info.Wo
    if out is None:
        out = torch.empty((N, Ho, Wo, ld), dtype=dtype, device=device)[..., :pc.cout]
    elif tuple(out.shape) != (N, Ho, Wo, pc.cout):
        raise _lib.ArsegError(f"conv out has shape {tuple(out.shape)}, expected {(N, Ho, Wo, pc.cout)}")
    d.out_ld = _nhwc_ld(out)
    if residual is not None:
        if tuple(residual.shape) != (N, Ho, Wo, pc.cout):
            raise _lib.ArsegError("residual shape mismatch")
        d.res_ld = _nhwc_ld(residual)
    return d, out, Ho, Wo


def _desc16(x, pc, residual, out, tile_cfg, split_k, up2=False):
    """arseg_conv_desc of a 16-bit conv (up2: ``x`` is the half-resolution input) and its output tensor -> (desc, out, N, H, W, Ho, Wo)."""
    N, H, W, Cin = x.shape
    if up2:
        H, W = 2 * H, 2 * W
    w16, cin_pad = pc.weights16(x.dtype)
    if Cin != cin_pad:
        raise _lib.ArsegError(f"conv (16-bit) expects {cin_pad} input channels (padded to 8), got {Cin}")
    d, out, Ho, Wo = _conv_desc(pc, N, H, W, Cin, _nhwc_ld(x), tile_cfg, split_k, residual, out, x.dtype, x.device, up2=up2)
    return d, out, N, H, W, Ho, Wo


def _conv16_candidates(ktiles: int, cout: int):
    """The (tile_cfg, split_k) the 16-bit tuner times, in its order: every plan x split-K where the plan takes it and K (``ktiles`` steps of 64) is long enough."""
    for cfg in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13):
        row = _lib.conv_plan_row(_lib.CONV_ENGINE_16, cfg)
        # (a plan without split-K -- patch-resident, stem -- enters once, its 128-channel tiles only for more than 64 channels)
        yield from ((cfg, sk) for sk in (0, 1, 2, 4, 8) if not ((sk > 1 and (ktiles // sk < 3 or cout % 8 or not row.split_k_allowed))
                                                                or (not row.split_k_allowed and (sk == 1 or (row.bn == 128 and cout <= 64)))))


def _conv16_up2_candidates(cout: int):
    """The fused-upsample plans the 16-bit tuner times, in its order (128-channel tiles only where there are more than 64 channels)."""
    return [(cfg, 0) for cfg in range(14) if fuses_up2(cfg, _lib.CONV_ENGINE_16) and not (_lib.conv_plan_row(_lib.CONV_ENGINE_16, cfg).bn == 128 and cout <= 64)]


def _wino_gemm_candidates(math: int, cout: int):
    """The tile_cfg of the batched GEMM the Winograd route times, in its order: tiles of 128 or more channels only where they are more than half used."""
    return [cfg for cfg in (0, 5, 6, 7, 8, 9, 10, 11, 12) + ((17, 18, 19) if math == _lib.MATH_F16X3 else ())
            for bn in [_lib.conv_plan_row(_lib.CONV_ENGINE_F32, cfg).bn] if not (bn >= 128 and cout <= bn // 2)]


def _up2_fusable(x_low, pc) -> bool:
    return pc.R == 3 and pc.S == 3 and pc.stride == 1 and pc.pad == 1 and pc.dil == 1 and x_low.shape[3] % 64 == 0 and _nhwc_ld(x_low) % 8 == 0


def _conv2d16_up2(x_low, pc, residual, out, tile_cfg, split_k):
    """conv2d16 on the x2 bilinear (align_corners=False) upsample of ``x_low`` (PSPUpsample).  The fused form -- a patch plan that interpolates
    while it stages (upsample2x) -- is timed against resize16 + conv2d16 once per shape and the winner kept.  tile_cfg 5..8 / 10..13 pins a
    fused plan (ARSEG_EUNSUPPORTED raises if the map is too narrow for it); any other pinned plan, an explicit split_k and the shapes the fused
    plans refuse take resize16 + conv2d16 with that plan, as before the fused form existed."""
    dt = _need_gpu16(x_low, residual, out)
    n_, h_, w_, _ = x_low.shape

    def materialised(o=out, cfg=tile_cfg, sk=split_k):
        return _conv2d16(resize_nhwc(x_low, 2 * h_, 2 * w_, _lib.BILINEAR, False), pc, residual, o, False, cfg, sk)

    if split_k or (tile_cfg and not fuses_up2(tile_cfg, _lib.CONV_ENGINE_16)) or not _up2_fusable(x_low, pc):
        return materialised()
    lib = _lib.load()
    d, out, N, H, W, Ho, Wo = _desc16(x_low, pc, residual, out, tile_cfg, 0, up2=True)
    w16, _ = pc.weights16(x_low.dtype)

    def args():
        return (ctypes.byref(d), dt, _ptr(x_low), _ptr(w16), _ptr(pc.scale), _ptr(pc.bias), _ptr(residual), _ptr(out), None, 0, _stream())

    if tile_cfg == 0 and sw.AUTOTUNE:
        def quiet(plan):
            if plan == "resize":
                return materialised(out)
            d.tile_cfg = plan[0]
            check(lib.arseg_conv2d16_fwd(*args()), "conv2d16")

        def candidates():
            yield from _conv16_up2_candidates(pc.cout)
            materialised(out)                                                  # (tunes the materialised conv's own plan first)
            yield "resize"

        # the plan key of the materialised conv of the same shape plus an "up2" marker: keys without it keep their meaning
        key = ("conv16", x_low.device.index, dt, N, H, W, x_low.shape[3], pc.cout, pc.R, pc.S, pc.stride, pc.pad, pc.dil, "up2")
        plan = tuned(key, candidates(), quiet, valid=lambda p: p == "resize" or isinstance(p, tuple))
        if plan in (None, "resize"):
            return materialised(out)
        d.tile_cfg = plan[0]
    flops16 = 2 * N * Ho * Wo * pc.cout * pc.R * pc.S * pc.cin
    with tagged((N, H, W, pc.cin, pc.cout, pc.R, pc.stride, pc.dil, True, "16-bit up2 " + str((d.tile_cfg, 0)), flops16)):
        launch("conv2d", lib.arseg_conv2d16_fwd, *args(), flops=flops16)
    return out


def _conv2d16(x, pc, residual, out, up2, tile_cfg=0, split_k=0):
    """conv2d on the 16-bit storage path: one MFMA per product (arseg_conv2d16_fwd), fp32 epilogue (pc.scale / pc.bias)."""
    if up2:
        return _conv2d16_up2(x, pc, residual, out, tile_cfg, split_k)
    dt = _need_gpu16(x, residual, out)
    d, out, N, H, W, Ho, Wo = _desc16(x, pc, residual, out, tile_cfg, split_k)
    Cin = x.shape[3]
    w16, cin_pad = pc.weights16(x.dtype)
    lib = _lib.load()

    def args():
        nbytes = lib.arseg_conv2d16_workspace_bytes(ctypes.byref(d))
        ws = workspace(nbytes, x.device) if nbytes else None
        return (ctypes.byref(d), dt, _ptr(x), _ptr(w16), _ptr(pc.scale), _ptr(pc.bias), _ptr(residual), _ptr(out), _ptr(ws), nbytes, _stream())

    if tile_cfg == 0 and split_k == 0 and sw.AUTOTUNE:      # per-shape plan: tile / K-step variants x split-K timed once on the device
        def quiet(plan):
            if plan == "gemm16":
                return gemm_rows16(x, pc, residual, out, record=False)
            d.tile_cfg, d.split_k = plan
            check(lib.arseg_conv2d16_fwd(*args()), "conv2d16")

        def candidates():
            yield from _conv16_candidates((pc.R * pc.S * Cin + 63) // 64, pc.cout)
            if sw.IGEMM3 and pc.R == 1 and pc.S == 1 and pc.stride == 1 and pc.pad == 0 and Cin % 64 == 0 and pc.cout % 4 == 0 and d.in_ld == Cin:
                try:                                                                       # 1x1: the plain GEMM of the LDS-DMA kernel
                    gemm_rows16(x, pc, residual, out, record=False)                         # (tunes its tile shape first)
                except _lib.ArsegError:
                    return
                yield "gemm16"

        key = ("conv16", x.device.index, dt, N, H, W, Cin, pc.cout, pc.R, pc.S, pc.stride, pc.pad, pc.dil)
        plan = tuned(key, candidates(), quiet, valid=lambda p: isinstance(p, tuple) or p == "gemm16", untuned=(0, 0)) or (0, 0)
        #  the plan key holds the shape, not the alignment / row pitch of `out` and `residual`: a later call with a channel-slice
        # view the LDS-DMA kernel refuses (EINVAL) falls back to the library's heuristic instead of raising
        if plan == "gemm16":
            if sw.IGEMM3 and d.in_ld == Cin:
                try:
                    return gemm_rows16(x, pc, residual, out)
                except _lib.ArsegError:
                    pass
            plan = (0, 0)
        d.tile_cfg, d.split_k = plan
    flops16 = 2 * N * Ho * Wo * pc.cout * pc.R * pc.S * pc.cin
    with tagged((N, H, W, pc.cin, pc.cout, pc.R, pc.stride, pc.dil, bool(up2), "16-bit " + str((d.tile_cfg, d.split_k)), flops16)):      # per-layer table (profile.layers())
        launch("conv2d", lib.arseg_conv2d16_fwd, *args(), flops=flops16)
    return out


def _conv_wino(x, pc, residual, out, N, H, W, record=True, up2=False):
    """3x3 stride-1 conv as Winograd F(4x4,3x3): input transform -> 36 batched GEMMs -> output transform.  The GEMMs run either on the
    implicit-GEMM kernel in batched 1x1 mode (plan = its tile_cfg) or, with the transformed activations written as split rows, on the
    LDS-DMA kernel of csrc/gemm_x3.hip (plan = 100 + its tile_cfg); whichever was faster when the shape was first seen.
    N,H,W: conv input size; with up2 ``x`` is the half-resolution tensor the input transform upsamples on the fly."""
    lib = _lib.load()
    Cin, Cout, dil = pc.cin_pad, pc.cout, pc.dil
    T = lib.arseg_wino43_tiles(N, H, W, dil)
    V = torch.empty((36, T, Cin), dtype=torch.float32, device=x.device)
    M = torch.empty((36, T, Cout), dtype=torch.float32, device=x.device)
    # under f16x3 the transformed activations are stored scaled by 2^-4 (exact; undone in the output transform): B^T d B amplifies by up to
    # 100, and unscaled the split-fp16 operand range would be left for |x| >~ 1.3e3
    vs = 2.0 ** -4 if sw.math == _lib.MATH_F16X3 else 1.0
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.in_ld = 1, T, 1, Cin, Cin
    d.Cout, d.out_ld, d.res_ld = Cout, Cout, Cout
    d.R, d.S, d.stride, d.pad, d.dil = 1, 1, 1, 0, 1
    d.act, d.prelu_slope = _lib.ACT_NONE, 0.0
    d.batch, d.in_batch_stride, d.w_batch_stride, d.out_batch_stride = 36, T * Cin, Cout * Cin, T * Cout
    d.math = math = sw.math
    _arm_range_watch(d, x.device)          # the batched GEMM watches the transformed activations it multiplies
    u_dev, scale_dev = (pc.wino_u_h3, pc.wino_scale_h3) if math != _lib.MATH_F32 else (pc.wino_u, pc.scale)
    x3_ok = bool(sw.GEMM_X3) and math == _lib.MATH_F16X3 and Cin % 32 == 0 and Cout % 4 == 0

    def transform(split, record=True):
        if split:      # the transform is the last place that sees the GEMM's fp32 operands: it carries the range watch
            launch("wino_input", lib.arseg_wino43_input_split_fwd, _ptr(x), _nhwc_ld(x), _ptr(V), N, H, W, Cin, dil, 1 if up2 else 0, vs,
                   ctypes.c_void_p(d.range_flag), 65504.0, _stream(), record=record)
        else:
            launch("wino_input", lib.arseg_wino43_input_fwd, _ptr(x), _nhwc_ld(x), _ptr(V), N, H, W, Cin, dil, 1 if up2 else 0, vs, _stream(),
                   record=record)

    def gemm(cfg, record=True):
        if cfg >= 100:
            fn, args = lib.arseg_gemm_x3_fwd, (_ptr(V), _ptr(u_dev), _ptr(M), T, Cout, Cin, Cout, 36, T * Cin * 4, Cout * Cin * 4, T * Cout,
                                               _ptr(None), _ptr(None), _ptr(None), 0, _lib.ACT_NONE, 0.0, 0, cfg - 100, _ptr(None), 0.0, _stream())
        else:
            d.tile_cfg, d.split_k = cfg, 1
            fn, args = lib.arseg_conv2d_fwd, (ctypes.byref(d), _ptr(V), _ptr(u_dev), _ptr(None), _ptr(None), _ptr(None), _ptr(M), _ptr(None), 0, _stream())
        launch("conv2d", fn, *args, flops=2 * 36 * T * Cin * Cout, record=record)

    def candidates():
        transform(False, record=False)
        yield from _wino_gemm_candidates(math, Cout)
        if x3_ok:
            transform(True, record=False)
            yield from range(100, 107)

    plan = tuned(("wino_gemm", x.device.index, T, Cin, Cout, math), candidates(), lambda c: gemm(c, False), valid=lambda p: p < 100 or x3_ok)
    if plan is None:
        raise _lib.ArsegError(f"wino: no batched GEMM configuration accepts T={T} K={Cin} N={Cout}")
    transform(plan >= 100, record)
    gemm(plan, record)
    launch("wino_output", lib.arseg_wino43_output_fwd, _ptr(M), _ptr(scale_dev), _ptr(pc.bias), _ptr(residual),
           _nhwc_ld(residual) if residual is not None else 0, _ptr(out), _nhwc_ld(out), N, H, W, Cout, dil, pc.act, pc.slope, 1.0 / vs, _stream(),
           record=record)


def _conv_up2_taps(x_low, pc, out, record=True, out_split=False):
    """conv3x3(pad 1) of the x2 bilinear upsample of ``x_low`` by tap decomposition (csrc/upconv.hip): one 1x1 conv at low resolution
    with the nine taps stacked along the output channels, then the gather that samples the nine planes at the shifted positions of the
    upsampled image and applies the epilogue of ``pc``.  out_split: the gather writes ``out`` (contiguous, Cout % 32 == 0) as split rows."""
    lib = _lib.load()
    n, h, w, _ = x_low.shape
    z = conv2d(x_low, pc.taps())
    if out_split:
        rw = _range_word(out.device) if sw.RANGE_MODE == "device" else None
        launch("up2_tap_gather", lib.arseg_upconv3x3_tap_gather_split_fwd, _ptr(z), 9 * pc.cout, _ptr(pc.scale), _ptr(pc.bias), _ptr(out), n, h, w,
               pc.cout, pc.act, pc.slope, _ptr(rw), 65504.0, _stream(), record=record)
    else:
        launch("up2_tap_gather", lib.arseg_upconv3x3_tap_gather_fwd, _ptr(z), 9 * pc.cout, _ptr(pc.scale), _ptr(pc.bias), _ptr(out), _nhwc_ld(out),
               n, h, w, pc.cout, pc.act, pc.slope, _stream(), record=record)


_psp_interp = {}


def psp_x3_foldable(pc) -> bool:
    """psp_bottleneck_x3 pre-divides the pyramid terms by the epilogue's per-channel scale: a channel whose folded scale is 0 (pruned /
    zero-initialised gamma) or tiny would give inf / overflow the split range, so such a module stays on the prior-sum + residual path.
    Decided once per packed conv (one host read at the first forward), cached."""
    ok = pc.__dict__.get("_x3_foldable")
    if ok is None:
        sc = pc.scale_h3.detach().abs()
        ok = pc.__dict__["_x3_foldable"] = bool(torch.isfinite(sc).all().item()) and float(sc.min().item()) > 1e-4 * max(float(sc.max().item()), 1e-30)
    return ok


def psp_bottleneck_x3(feats: torch.Tensor, t: torch.Tensor, pc, sizes, out_split: bool = True):
    """PSPModule's folded bottleneck (model/pspnet.py:14-31) as ONE GEMM:  relu(W_f f + b + sum_s upsample(t_s))  with the pyramid sum written as
    B . T -- B [H*W, 64] the bilinear interpolation matrix of the pooled rows (built once per shape by running psp_prior_sum on an identity, so it
    holds exactly the weights that kernel applies), T the per-image pyramid terms -- and concatenated along K of the bottleneck GEMM
    (arseg_gemm_x3_cat_fwd): [f | B] . [W_f ; T]^T.  The 92 MB prior tensor (written by one kernel, read back as a residual by the next) is
    gone: two more K steps.  feats [N,H,W,C] fp32, t [N, rows, C_out] (rows = sum s^2 <= 64); returns SplitRows / tensor [N,H,W,C_out]."""
    lib = _lib.load()
    N, H, W, C = feats.shape
    rows, Cout, dev = t.shape[1], pc.cout, feats.device
    key = (dev.index, H, W, tuple(sizes))
    B = _psp_interp.get(key)
    if B is None:
        eye = torch.zeros((1, rows, 64), dtype=torch.float32, device=dev)
        eye[0, torch.arange(rows), torch.arange(rows)] = 1.0
        B = _psp_interp[key] = split_rows(psp_prior_sum(eye, sizes, H, W))          # [1,H,W,64] split rows, shared by the batch
    fac = pc.__dict__.get("_x3_unscale")
    if fac is None:
        fac = pc.__dict__["_x3_unscale"] = (1.0 / pc.scale_h3).contiguous()          # the epilogue multiplies the accumulator by scale_h3
        # (a channel whose folded scale is 0 or tiny cannot be un-scaled: psp_x3_foldable() keeps such a module on the residual path)
    # the per-image pyramid operand [N, Cout, 64] as split rows, straight from t (no torch arithmetic inside the step)
    w2s = SplitRows(torch.empty((N, Cout, 1, 64), dtype=torch.float32, device=dev))
    #  the un-scale factor can be large (psp_x3_foldable admits scale ratios up to 1e4): this pass carries the range watch of its operand
    rw2 = _range_word(dev) if sw.RANGE_MODE == "device" else None
    launch("psp_w2_split", lib.arseg_psp_w2_split_fwd, _ptr(t.contiguous()), _ptr(fac), _ptr(w2s.t), N, rows, Cout, _ptr(rw2), 65504.0, _stream())
    xs = split_rows(feats)
    out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=dev)
    rw = _range_word(dev) if (out_split and sw.RANGE_MODE == "device") else None

    def run(c, record=True):
        launch("conv2d", lib.arseg_gemm_x3_cat_fwd, _ptr(xs.t), _ptr(pc.w_h3), _ptr(B.t), _ptr(w2s.t), _ptr(out), H * W, Cout, C, 64, Cout, N,
               H * W * C * 4, 0, 0, Cout * 64 * 4, H * W * Cout, _ptr(pc.scale_h3), _ptr(pc.bias), pc.act, pc.slope, 1 if out_split else 0, c, _ptr(rw),
               65504.0, _stream(), flops=2 * N * H * W * (C + 64) * Cout, record=record)

    cfg = tuned(("x3cat", dev.index, N, H * W, C, Cout, bool(out_split)), range(7), lambda c: run(c, False))
    if cfg is None:
        raise _lib.ArsegError(f"gemm_x3_cat: no tile configuration accepts M={H * W} K={C + 64} N={Cout}")
    with tagged((N, H, W, C, Cout, 1, 1, 1, False, "x3(cat, split out)", 2 * N * H * W * C * Cout)):
        run(cfg, True)
    return SplitRows(out) if out_split else out
