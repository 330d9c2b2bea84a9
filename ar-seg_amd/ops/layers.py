"""Layout helpers, the localAttention pair, ingest, and the small layers (pooling, resizes, ARM / FFM scaling, heads, evaluator tail,
mergeMotion): thin wrappers, one ABI call each."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from .. import _lib
from . import _base
from ._base import _DT16, _need_gpu, _need_gpu16, _nhwc_ld, _ptr, _storage, _stream, is16, workspace
from ._profile import launch


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 <-> fp16 / bf16 element conversion on the GPU (round to nearest even), any shape with numel % 8 == 0."""
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    code = lambda d: _lib.DT_F32 if d == torch.float32 else _DT16[d]
    launch("cast", _lib.load().arseg_cast_fwd, _ptr(x), code(x.dtype), _ptr(out), code(dtype), x.numel(), _stream())
    return out


def frame_ingest(img: torch.Tensor, h: int, w: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """NCHW RGB frame -> the conv engine's input at (h,w): NHWC4 fp32, or NHWC8 fp16 / bf16 on the 16-bit storage path."""
    if dtype == torch.float32:
        return frame_to_nhwc4(img, h, w)
    _need_gpu(img)
    img = img.contiguous()
    N, C, H, W = img.shape
    if C != 3:
        raise _lib.ArsegError("frame_ingest expects 3 input channels")
    out = torch.empty((N, h, w, 8), dtype=dtype, device=img.device)
    launch("frame_to_nhwc8", _lib.load().arseg_frame_to_nhwc8_16_fwd, _ptr(img), _ptr(out), _DT16[dtype], N, H, W, h, w, _stream())
    return out


def _plane_layout(t: torch.Tensor, inner, what: str):
    """(pitch, image stride) in bytes of a uint8 / uint16 plane [N,H,...inner]: rows of ``inner`` contiguous samples, any row pitch / image stride."""
    want, row = [], 1
    for d in reversed(inner):
        want.insert(0, row)
        row *= d
    N, H = t.shape[0], t.shape[1]
    if tuple(t.shape[2:]) != tuple(inner) or tuple(t.stride()[2:]) != tuple(want):
        raise _lib.ArsegError(f"{what}: expected rows of {tuple(inner)} contiguous samples, got shape {tuple(t.shape)} strides {t.stride()}")
    pitch = t.stride(1) if H > 1 else row
    n_stride = t.stride(0) if N > 1 else 0
    if pitch < row or n_stride < 0:
        raise _lib.ArsegError(f"{what}: row pitch {pitch} is smaller than a row of {row} samples (or a negative image stride)")
    return pitch * t.element_size(), n_stride * t.element_size()


# source format -> (public name = launch label, sample dtype, inner shape of each plane at width W): plane 0 is [N,H,...], the chroma planes [N,H/2,...]
_SRC_PLANES = {
    _lib.SRC_RGB8: ("frame_ingest8", torch.uint8, lambda W: ((W, 3),)),
    _lib.SRC_NV12: ("frame_ingest8", torch.uint8, lambda W: ((W,), (W // 2, 2))),
    _lib.SRC_I420: ("frame_ingest_yuv", torch.uint8, lambda W: ((W,), (W // 2,), (W // 2,))),
    _lib.SRC_P010: ("frame_ingest_yuv", torch.uint16, lambda W: ((W,), (W // 2, 2))),
    _lib.SRC_I010: ("frame_ingest_yuv", torch.uint16, lambda W: ((W,), (W // 2,), (W // 2,))),
}
# launch label -> (C entry point, plane arguments it has, what it expects in words)
_INGEST_ENTRY = {
    "frame_ingest8": ("arseg_frame_ingest_fwd", 2, "expects uint8 [N,H,W,3] (RGB8) or luma [N,H,W] + chroma [N,H/2,W/2,2] on one device (NV12)"),
    "frame_ingest_yuv": ("arseg_frame_ingest_yuv_fwd", 3, "expects a luma plane [N,H,W] and its chroma planes on one device"),
}


def _frame_ingest_planes(planes, src_format: int, h: int, w: int, mean, std, dtype: torch.dtype = torch.float32,
                         colour: int = _lib.COLOUR_BT709_LIMITED, only: Optional[str] = None) -> torch.Tensor:
    """The planes of any ``src_format`` -> the conv engine's input at (h,w): checks them against _SRC_PLANES and makes the format's one ABI
    call.  ``only``: the public name asked for, which takes its own formats and no others."""
    name, sample, inner_at = _SRC_PLANES.get(src_format, (None, None, None))
    if name is None or only not in (None, name):
        raise _lib.ArsegError(f"{only or 'frame_ingest'}: unknown source format {src_format}")
    if dtype != torch.float32 and dtype not in _DT16:
        raise _lib.ArsegError(f"{name}: unsupported output dtype {dtype}")
    entry, slots, expects = _INGEST_ENTRY[name]
    planes, n = tuple(planes), len(inner_at(0))
    if len(planes) != n or any(not torch.is_tensor(t) for t in planes):
        raise _lib.ArsegError(f"{name}: expected {n} plane tensors, got {sum(torch.is_tensor(t) for t in planes)}")
    _need_gpu(*planes, dtype=sample)
    p0 = planes[0]
    if p0.dim() != 2 + len(inner_at(0)[0]) or any(t.device != p0.device for t in planes):
        raise _lib.ArsegError(f"{name} {expects}")
    N, H, W = p0.shape[:3]
    inner = inner_at(W)
    if n > 1 and (H % 2 or W % 2 or any(tuple(t.shape) != (N, H // 2) + i for t, i in zip(planes[1:], inner[1:]))):
        raise _lib.ArsegError(f"{name}: needs even H, W and chroma planes {[(N, H // 2) + i for i in inner[1:]]}; got {[tuple(t.shape) for t in planes]}")
    lay = [_plane_layout(t, i, f"{name} plane {k}") for k, (t, i) in enumerate(zip(planes, inner))] + [(0, 0)] * (slots - n)
    ptrs = [_ptr(t) for t in planes] + [_ptr(None)] * (slots - n)
    out = torch.empty((N, h, w, 4 if dtype == torch.float32 else 8), dtype=dtype, device=p0.device)
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    src_bytes = N * H * W * 3 * p0.element_size() // (1 if n == 1 else 2)
    launch(name, getattr(_lib.load(), entry), *ptrs, src_format, *[p for p, _ in lay], *[s for _, s in lay], int(colour), _ptr(out),
           _lib.DT_F32 if dtype == torch.float32 else _DT16[dtype], N, H, W, h, w, m3, s3, _stream(), nbytes=src_bytes + out.numel() * out.element_size())
    return out


def frame_ingest8(plane0: torch.Tensor, plane1: Optional[torch.Tensor], src_format: int, h: int, w: int, mean, std,
                  dtype: torch.dtype = torch.float32, colour: int = _lib.COLOUR_BT709_LIMITED) -> torch.Tensor:
    """8-bit decoder frames -> the conv engine's input at (h,w) in one kernel: NHWC4 fp32, or NHWC8 fp16 / bf16 (csrc/ingest.hip).
    ``src_format`` _lib.SRC_RGB8: plane0 uint8 [N,H,W,3], plane1 None;  _lib.SRC_NV12: plane0 luma uint8 [N,H,W], plane1 chroma uint8
    [N,H/2,W/2,2] (Cb, Cr), ``colour`` one of _lib.COLOUR_*.  Planes may be views with a row pitch and an image stride.  Colour conversion,
    bilinear align_corners=True downscale, ToTensor + Normalize(mean, std): include/arseg_hip.h, arseg_frame_ingest_fwd."""
    planes = (plane0, plane1) if src_format == _lib.SRC_NV12 else (plane0,)
    return _frame_ingest_planes(planes, src_format, h, w, mean, std, dtype, colour, only="frame_ingest8")


def frame_ingest_yuv(planes, src_format: int, h: int, w: int, mean, std, dtype: torch.dtype = torch.float32,
                     colour: int = _lib.COLOUR_BT709_LIMITED) -> torch.Tensor:
    """Planar 4:2:0 / 10-bit decoder frames -> the conv engine's input at (h,w) in one kernel, like ``frame_ingest8`` (csrc/ingest.hip).
    ``src_format`` _lib.SRC_I420: planes = (Y [N,H,W], Cb [N,H/2,W/2], Cr [N,H/2,W/2]) uint8;  _lib.SRC_I010: the same planes, uint16, code in
    the low 10 bits;  _lib.SRC_P010: planes = (Y [N,H,W], (Cb, Cr) [N,H/2,W/2,2]) uint16, code in the high 10 bits.  Planes may be views with a
    row pitch and an image stride.  include/arseg_hip.h, arseg_frame_ingest_yuv_fwd."""
    return _frame_ingest_planes(planes, src_format, h, w, mean, std, dtype, colour, only="frame_ingest_yuv")


def ingest_input(frames, h: int, w: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The one door through which the fast paths take frames: a float NCHW tensor (``frame_ingest``, unchanged) or 8-bit decoder output
    (``arseg_amd.ingest.DecodedFrames``: its ``to_input`` runs ``_frame_ingest_planes``) -> the conv engine's input at (h,w)."""
    if torch.is_tensor(frames):
        return frame_ingest(frames, h, w, dtype)
    to_input = getattr(frames, "to_input", None)
    if to_input is None:
        raise _lib.ArsegError(f"expected a float NCHW tensor or arseg_amd.ingest.DecodedFrames, got {type(frames).__name__}")
    return to_input(h, w, dtype)


# ----------------------------------------------------------------------------------------------
# layout helpers
# ----------------------------------------------------------------------------------------------
def is_nhwc_view(x: torch.Tensor) -> bool:
    """True if logical-NCHW ``x`` is physically NHWC-contiguous (channels_last or a permuted NHWC tensor)."""
    N, C, H, W = x.shape
    return x.stride() == (H * W * C, 1, W * C, C)


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """Logical NCHW tensor -> physical NHWC tensor [N,H,W,C] (zero-copy when already channels_last)."""
    if is16(x):
        _need_gpu16(x)
        return x.permute(0, 2, 3, 1) if is_nhwc_view(x) else x.permute(0, 2, 3, 1).contiguous()
    _need_gpu(x)
    N, C, H, W = x.shape
    if is_nhwc_view(x):
        return x.permute(0, 2, 3, 1)
    x = x.contiguous()
    out = torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    launch("nchw_to_nhwc", _lib.load().arseg_nchw_to_nhwc_fwd, _ptr(x), _ptr(out), N, C, H * W, C, _stream())
    return out


def as_nchw(x_nhwc: torch.Tensor) -> torch.Tensor:
    """Physical NHWC [N,H,W,C] -> logical NCHW view (channels_last strides, no copy)."""
    return x_nhwc.permute(0, 3, 1, 2)


def to_nchw_contiguous(x_nhwc: torch.Tensor) -> torch.Tensor:
    _need_gpu(x_nhwc)
    N, H, W, C = x_nhwc.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x_nhwc.device)
    launch("nhwc_to_nchw", _lib.load().arseg_nhwc_to_nchw_fwd, _ptr(x_nhwc), C, _ptr(out), N, C, H * W, _stream())
    return out


def to_c8(x: torch.Tensor, layout: int) -> torch.Tensor:
    """NCHW-contiguous [N,C,H,W] or NHWC [N,H,W,C] -> channel-blocked [N,C/8,H,W,8]."""
    _need_gpu(x)
    if layout == _lib.NCHW:
        N, C, H, W = x.shape
        x = x.contiguous()
        ld = 0
    else:
        N, H, W, C = x.shape
        x = x.contiguous()
        ld = C
    out = torch.empty((N, C // 8, H, W, 8), dtype=torch.float32, device=x.device)
    launch("to_c8", _lib.load().arseg_to_c8_fwd, _ptr(x), layout, ld, _ptr(out), N, C, H * W, _stream())
    return out


def from_c8(x: torch.Tensor, layout: int) -> torch.Tensor:
    _need_gpu(x)
    N, CB, H, W, _ = x.shape
    C = CB * 8
    shape = (N, C, H, W) if layout == _lib.NCHW else (N, H, W, C)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    launch("from_c8", _lib.load().arseg_from_c8_fwd, _ptr(x), _ptr(out), layout, C, N, C, H * W, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# localAttention pair
# ----------------------------------------------------------------------------------------------
def _is_cl(t: torch.Tensor) -> bool:
    return t.dim() == 4 and t.shape[1] > 1 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def local_similar(q: torch.Tensor, k: torch.Tensor, kH: int, kW: int) -> torch.Tensor:
    """localAttention.similar_forward; channels_last inputs go to the NHWC variant without a layout change."""
    _need_gpu(q, k)
    N, C, H, W = q.shape
    out = torch.empty((N, H, W, kH * kW), dtype=torch.float32, device=q.device)
    if _is_cl(q) and _is_cl(k):
        launch("local_similar", _lib.load().arseg_local_similar_nhwc_fwd, _ptr(q), _ptr(k), C, _ptr(out), N, C, H, W, kH, kW, _stream())
        return out
    q, k = q.contiguous(), k.contiguous()
    launch("local_similar", _lib.load().arseg_local_similar_fwd, _ptr(q), _ptr(k), _ptr(out), N, C, H, W, kH, kW, _stream())
    return out


def local_weighting(v: torch.Tensor, w: torch.Tensor, kH: int, kW: int) -> torch.Tensor:
    """localAttention.weighting_forward; a channels_last ``v`` gives a channels_last result through the NHWC variant."""
    _need_gpu(v, w)
    w = w.contiguous()
    N, C, H, W = v.shape
    if _is_cl(v):
        out = torch.empty_like(v, memory_format=torch.channels_last)
        launch("local_weighting", _lib.load().arseg_local_weighting_nhwc_fwd, _ptr(v), _ptr(w), C, _ptr(out), N, C, H, W, kH, kW, _stream())
        return out
    v = v.contiguous()
    out = torch.empty_like(v)
    launch("local_weighting", _lib.load().arseg_local_weighting_fwd, _ptr(v), _ptr(w), _ptr(out), N, C, H, W, kH, kW, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# small layers
# ----------------------------------------------------------------------------------------------
# A layer that exists in both storages makes one call: `dt = _storage(...)` is the 16-bit dtype code or None (fp32); the 16-bit entry point
# takes the code as an extra argument (``*_dt(dt)``) and the result has the input's dtype.
def _dt(dt):
    return () if dt is None else (dt,)


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    dt = _storage(x)
    x = x.contiguous()
    N, H, W, C = x.shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    launch("maxpool", lib.arseg_maxpool3x3s2_fwd if dt is None else lib.arseg_maxpool3x3s2_16_fwd, _ptr(x), _ptr(out), *_dt(dt), N, H, W, C, _stream())
    return out


def adaptive_avgpool(x: torch.Tensor, oh: int, ow: int, out: Optional[torch.Tensor] = None, out_ld: int = 0, out_n_stride: int = 0
                     ) -> torch.Tensor:
    """NHWC -> [N,oh,ow,C]; or, with ``out`` (a base tensor/view whose data_ptr is the first bin of image 0), into rows of a
    wider matrix: element (n, bin, c) at out + n*out_n_stride + bin*out_ld + c."""
    _need_gpu(x, out)
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty((N, oh, ow, C), dtype=torch.float32, device=x.device)
    launch("adaptive_avgpool", _lib.load().arseg_adaptive_avgpool_fwd, _ptr(x), _nhwc_ld(x), _ptr(out), out_ld, out_n_stride, N, H, W, C,
            oh, ow, _stream())
    return out


def psp_pool_matrix(x: torch.Tensor, sizes) -> torch.Tensor:
    """The folded pyramid's block-structured pooled matrix [N, sum(s^2), 1, len(sizes)*C]: level i's adaptive average pool in columns
    [i*C, (i+1)*C) of its s_i^2 rows, zeros elsewhere -- written entirely by the pooling launches (no fill).
    16-bit input: arseg_psp_pool_matrix16_fwd, the matrix in the storage dtype."""
    dt = _storage(x)
    N, H, W, C = x.shape
    n, rows = len(sizes), sum(s * s for s in sizes)
    out = torch.empty((N, rows, 1, n * C), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    arr = (ctypes.c_int * n)(*[int(s) for s in sizes])
    if dt is not None:
        nb = lib.arseg_psp_pool_matrix16_workspace_bytes(N, H, W, C, n, arr)
        if not nb:
            raise _lib.ArsegError(f"psp_pool_matrix (16-bit): pyramid sizes {tuple(sizes)} are not supported (at most 4 levels of size <= 6)")
        ws = workspace(nb, x.device)
    else:
        nb = lib.arseg_psp_pool_matrix_workspace_bytes(N, H, W, C, n, arr) if (n <= 4 and C % 4 == 0 and N <= 65535) else 0
        ws = torch.empty((nb // 4,), dtype=torch.float32, device=x.device) if nb else None
    if nb:          # one pass over the map: the cells of the grid spanned by all bin edges are summed once, then combined per bin
        launch("adaptive_avgpool", lib.arseg_psp_pool_matrix_fwd if dt is None else lib.arseg_psp_pool_matrix16_fwd, _ptr(x), _nhwc_ld(x), _ptr(out), *_dt(dt),
               _ptr(ws), nb, N, H, W, C, n, arr, _stream())
        return out
    off = 0
    for i, s in enumerate(sizes):          # (fp32 only: a pyramid the one-pass form does not take, level by level)
        launch("adaptive_avgpool", lib.arseg_adaptive_avgpool_blockrow_fwd, _ptr(x), _nhwc_ld(x), _ptr(out[0, off]), rows * n * C,
                N, H, W, C, s, s, n, i, _stream())
        off += s * s
    return out


def psp_prior_sum(t: torch.Tensor, sizes, H: int, W: int) -> torch.Tensor:
    """t [N, sum(s^2), C] (per-level maps after the folded 1x1 convs) -> [N,H,W,C] sum of bilinear upsamples (16-bit t: in the storage dtype,
    summed in fp32 and rounded once)."""
    dt = _storage(t)
    t = t.contiguous()
    N, rows, C = t.shape
    if rows != sum(s * s for s in sizes):
        raise _lib.ArsegError("psp_prior_sum: row count does not match the pyramid sizes")
    out = torch.empty((N, H, W, C), dtype=t.dtype, device=t.device)
    arr = (ctypes.c_int * len(sizes))(*[int(s) for s in sizes])
    lib = _lib.load()
    launch("psp_prior_sum", lib.arseg_psp_prior_sum_fwd if dt is None else lib.arseg_psp_prior_sum16_fwd, _ptr(t), _ptr(out), *_dt(dt), N, H, W, C, len(sizes),
           arr, _stream())
    return out


def global_reduce(x: torch.Tensor, op: int) -> torch.Tensor:
    """NHWC -> [N,1,1,C] mean or max over (H,W)."""
    dt = _storage(x)
    N, H, W, C = x.shape
    out = torch.empty((N, 1, 1, C), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    if dt is None:
        nb = lib.arseg_global_reduce_workspace_bytes(N, H, W, C)
        ws = torch.empty((nb // 4,), dtype=torch.float32, device=x.device) if nb else None       # (large map, few images: two-stage reduce)
        launch("global_reduce", lib.arseg_global_reduce_ws_fwd, _ptr(x), _nhwc_ld(x), _ptr(out), _ptr(ws), nb, N, H, W, C, op, _stream())
        return out
    if op not in (_lib.REDUCE_MEAN, _lib.REDUCE_MAX):          # (16-bit storage: one entry point per op, slices and a final pass)
        raise _lib.ArsegError(f"global_reduce: unknown op {op}")
    nb = lib.arseg_global_mean16_workspace_bytes(N, H, W, C)
    ws = workspace(nb, x.device)
    launch("global_reduce", lib.arseg_global_mean16_fwd if op == _lib.REDUCE_MEAN else lib.arseg_global_max16_fwd, _ptr(x), _nhwc_ld(x), _ptr(out), dt,
           N, H, W, C, _ptr(ws), nb, _stream())
    return out


def resize_nhwc(x: torch.Tensor, Hout: int, Wout: int, mode: int, align_corners: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dt = _storage(x, out)
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty((N, Hout, Wout, C), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    launch("resize_nhwc", lib.arseg_resize_fwd if dt is None else lib.arseg_resize16_fwd, _ptr(x), _ptr(out), *_dt(dt), N, C, H, W, Hout, Wout, mode,
           1 if align_corners else 0, *((_lib.NHWC,) if dt is None else ()), _nhwc_ld(x), _nhwc_ld(out), _stream())
    return out


def resize_nchw(x: torch.Tensor, Hout: int, Wout: int, mode: int, align_corners: bool) -> torch.Tensor:
    _need_gpu(x)
    x = x.contiguous()
    N, C, H, W = x.shape
    out = torch.empty((N, C, Hout, Wout), dtype=torch.float32, device=x.device)
    launch("resize_nchw", _lib.load().arseg_resize_fwd, _ptr(x), _ptr(out), N, C, H, W, Hout, Wout, mode, 1 if align_corners else 0, _lib.NCHW, 0, 0,
                                       _stream())
    return out


def scale_add(x: torch.Tensor, scale: torch.Tensor, add_full: Optional[torch.Tensor] = None, add_vec: Optional[torch.Tensor] = None
              ) -> torch.Tensor:
    """out = x * scale[n,c] (+ add_full[n,h,w,c]) (+ add_vec[n,c]); x NHWC contiguous, scale/add_vec [N,1,1,C]."""
    dt = _storage(x, scale, add_full, add_vec)
    x = x.contiguous()
    N, H, W, C = x.shape
    out = torch.empty_like(x)
    lib = _lib.load()
    launch("scale_add", lib.arseg_scale_add_fwd if dt is None else lib.arseg_scale_add16_fwd, _ptr(x), _ptr(scale.contiguous()),
           _ptr(None if add_full is None else add_full.contiguous()), _ptr(None if add_vec is None else add_vec.contiguous()), _ptr(out), *_dt(dt), N, H * W, C,
           _stream())
    return out


def head(p_nhwc: torch.Tensor, wf: torch.Tensor, bf: torch.Tensor, log_softmax: bool) -> torch.Tensor:
    """1x1 classifier on an NHWC feature (fp32 or 16-bit; fp32 weights) -> NCHW fp32 logits (optionally LogSoftmax over classes)."""
    dt = _storage(p_nhwc)
    _need_gpu(wf, bf)
    N, H, W, C = p_nhwc.shape
    n_cls = wf.shape[0]
    out = torch.empty((N, n_cls, H, W), dtype=torch.float32, device=p_nhwc.device)
    lib = _lib.load()
    launch("head", lib.arseg_head_fwd if dt is None else lib.arseg_head16_fwd, _ptr(p_nhwc), _nhwc_ld(p_nhwc), *_dt(dt), _ptr(wf), _ptr(bf), _ptr(out), N, H * W,
           C, n_cls, 1 if log_softmax else 0, _stream())
    return out


def frame_to_nhwc4(img: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """NCHW RGB frame -> NHWC4, bilinear(align_corners=True) resized to (h,w) (evaluation.py:186-188)."""
    _need_gpu(img)
    img = img.contiguous()
    N, C, H, W = img.shape
    if C != 3:
        raise _lib.ArsegError("frame_to_nhwc4 expects 3 input channels")
    out = torch.empty((N, h, w, 4), dtype=torch.float32, device=img.device)
    launch("frame_to_nhwc4", _lib.load().arseg_frame_to_nhwc4_fwd, _ptr(img), _ptr(out), N, H, W, h, w, _stream())
    return out


def frame_u8_to_nhwc4(img_u8: torch.Tensor, h: int, w: int, mean, std) -> torch.Tensor:
    """Decoded uint8 frames [N,H,W,3] (HWC, on the GPU) -> normalised NHWC4 [N,h,w,4] (ToTensor + Normalize + bilinear
    align_corners=True downscale in one kernel; the float frame is never materialised)."""
    if img_u8.dtype != torch.uint8 or not img_u8.is_cuda or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise _lib.ArsegError("frame_u8_to_nhwc4 expects a CUDA uint8 tensor [N,H,W,3]")
    img_u8 = img_u8.contiguous()
    N, H, W, _ = img_u8.shape
    out = torch.empty((N, h, w, 4), dtype=torch.float32, device=img_u8.device)
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    launch("frame_u8_to_nhwc4", _lib.load().arseg_frame_u8_to_nhwc4_fwd, _ptr(img_u8), _ptr(out), N, H, W, h, w, m3, s3, _stream())
    return out


def merge_motion(flows: torch.Tensor, frame_start: int = 0) -> torch.Tensor:
    """Codec motion fields int16 [F+1,H,W,3] (mv_x, mv_y quarter-pel, reference index; on the GPU) -> accumulated quarter-pel
    motion to the keyframe, int16 [F+1,H,W,2] (frame 0 = -1, as the reference's mergeMotion leaves it)."""
    if flows.dtype != torch.int16 or not flows.is_cuda or flows.dim() != 4 or flows.shape[-1] != 3:
        raise _lib.ArsegError("merge_motion expects a CUDA int16 tensor [F+1,H,W,3]")
    flows = flows.contiguous()
    F1, H, W, _ = flows.shape
    lib = _lib.load()
    nbytes = lib.arseg_merge_motion_workspace_bytes(F1 - 1, H, W)
    ws = workspace(nbytes, flows.device)
    out = torch.empty((F1, H, W, 2), dtype=torch.int16, device=flows.device)
    launch("merge_motion", lib.arseg_merge_motion_fwd, _ptr(flows), _ptr(out), _ptr(ws), nbytes, F1 - 1, frame_start, H, W, _stream())
    return out


def _mv_records(records: torch.Tensor, what: str) -> int:
    """Checks a record buffer (int16 [n,8], contiguous, on the GPU; include/arseg_hip.h, arseg_mv_records_*) and returns its capacity n."""
    if not torch.is_tensor(records) or records.dtype != torch.int16 or not records.is_cuda or records.dim() != 2 or records.shape[1] != 8 \
            or not records.is_contiguous():
        raise _lib.ArsegError(f"{what} expects records as a contiguous CUDA int16 tensor [n,8] (x, y, w, h, mvx, mvy, ref, reserved)")
    return int(records.shape[0])


def _mv_chain_state(merged: torch.Tensor, index_map: torch.Tensor, what: str, maps: int = 1):
    if not torch.is_tensor(merged) or merged.dtype != torch.int16 or not merged.is_cuda or merged.dim() != 4 or merged.shape[-1] != 2 \
            or not merged.is_contiguous():
        raise _lib.ArsegError(f"{what} expects merged as a contiguous CUDA int16 tensor [gop,H,W,2]")
    gop, H, W, _ = merged.shape
    if not torch.is_tensor(index_map) or index_map.dtype != torch.int32 or index_map.device != merged.device or not index_map.is_contiguous() \
            or index_map.numel() < maps * H * W:
        raise _lib.ArsegError(f"{what} expects the index map as a contiguous int32 tensor of at least {maps if maps > 1 else ''}H*W = {maps * H * W} elements on "
                              f"merged's device")
    return gop, H, W


def mv_records_reset(merged: torch.Tensor, index_map: torch.Tensor) -> None:
    """Starts a GOP of the record chain: index map = -1, merged[0] = -1 (what merge_motion leaves in frame 0).  merged int16 [gop,H,W,2],
    index_map int32 [H*W] (or [H,W]), both caller-owned on one GPU."""
    _, H, W = _mv_chain_state(merged, index_map, "mv_records_reset")
    launch("mv_records_reset", _lib.load().arseg_mv_records_reset, _ptr(merged), _ptr(index_map), index_map.numel() * 4, H, W, _stream())


def mv_records_step(records: torch.Tensor, merged: torch.Tensor, f: int, index_map: torch.Tensor, max_ref: int = 3) -> torch.Tensor:
    """One P-frame of the record chain: rasterises the frame's block records (highest index wins) and chains them to the keyframe through
    merged[f2], f2 < f; writes and returns the view merged[f] (int16 [H,W,2] quarter-pel, the mv_q of frame f).  Two kernels, no
    synchronisation, no allocation; frames go in order 1, 2, ... after mv_records_reset."""
    n = _mv_records(records, "mv_records_step")
    gop, H, W = _mv_chain_state(merged, index_map, "mv_records_step")
    if records.device != merged.device:
        raise _lib.ArsegError(f"mv_records_step: records are on {records.device}, merged on {merged.device}")
    launch("mv_records_step", _lib.load().arseg_mv_records_step_fwd, _ptr(records), n, _ptr(merged), int(f), gop, _ptr(index_map), index_map.numel() * 4,
           H, W, int(max_ref), _stream())
    return merged[f]


def _mv_link_state(link: torch.Tensor, link_stats, gop: int, H: int, W: int, dev, what: str) -> None:
    if not torch.is_tensor(link) or link.dtype != torch.uint8 or link.device != dev or tuple(link.shape) != (gop, H, W) or not link.is_contiguous():
        raise _lib.ArsegError(f"{what} expects link as a contiguous uint8 tensor {(gop, H, W)} on {dev}")
    if link_stats is not None and (not torch.is_tensor(link_stats) or link_stats.dtype != torch.int64 or link_stats.device != dev
                                   or tuple(link_stats.shape) != (gop, _lib.LINK_NSTATS) or not link_stats.is_contiguous()):
        raise _lib.ArsegError(f"{what} expects link_stats as a contiguous int64 tensor {(gop, _lib.LINK_NSTATS)} on {dev} (or None)")


def mv_link_reset(link: torch.Tensor, link_stats: Optional[torch.Tensor] = None) -> None:
    """Starts a GOP of the link bytes (include/arseg_hip.h, arseg_mv_link_reset): link[0] = 0 and every row of link_stats = 0.  link uint8
    [gop,H,W], link_stats int64 [gop, LINK_NSTATS] or None, caller-owned on one GPU.  Goes with mv_records_reset / mv_records_bi_reset."""
    if not torch.is_tensor(link) or not link.is_cuda or link.dim() != 3:
        raise _lib.ArsegError("mv_link_reset expects link as a contiguous CUDA uint8 tensor [gop,H,W]")
    gop, H, W = link.shape
    _mv_link_state(link, link_stats, gop, H, W, link.device, "mv_link_reset")
    launch("mv_link_reset", _lib.load().arseg_mv_link_reset, _ptr(link), _ptr(link_stats), gop, H, W, _stream())


def mv_records_step_link(records: torch.Tensor, merged: torch.Tensor, f: int, index_map: torch.Tensor, link: torch.Tensor,
                         link_stats: Optional[torch.Tensor] = None, max_ref: int = 3):
    """mv_records_step that also writes the link bytes of frame f (uint8 [H,W]: bit 0 intra, bit 1 uncovered, bit 2 clamped -- at this hop or at
    any hop towards the keyframe -- and the hops in bits 4..7) into link[f] and adds the frame's counts to link_stats[f] (None: not wanted).
    merged[f] is bit-equal to mv_records_step's; the same two kernels.  Returns the views (merged[f], link[f])."""
    n = _mv_records(records, "mv_records_step_link")
    gop, H, W = _mv_chain_state(merged, index_map, "mv_records_step_link")
    if records.device != merged.device:
        raise _lib.ArsegError(f"mv_records_step_link: records are on {records.device}, merged on {merged.device}")
    _mv_link_state(link, link_stats, gop, H, W, merged.device, "mv_records_step_link")
    launch("mv_records_step_link", _lib.load().arseg_mv_records_step_link_fwd, _ptr(records), n, _ptr(merged), int(f), gop, _ptr(index_map),
           index_map.numel() * 4, H, W, int(max_ref), _ptr(link), _ptr(link_stats), _stream())
    return merged[f], link[f]


MV_BI_POLICIES = {"list0": _lib.MVR_BI_LIST0, "near": _lib.MVR_BI_NEAR, "mean": _lib.MVR_BI_MEAN}


def mv_records_bi_reset(merged: torch.Tensor, index_maps: torch.Tensor) -> None:
    """Starts a GOP of the two-list (B-frame) record chain: both index maps = -1, merged[0] = -1.  merged int16 [gop,H,W,2], index_maps int32
    of at least 2*H*W elements (list 0's map, then list 1's), both caller-owned on one GPU."""
    _, H, W = _mv_chain_state(merged, index_maps, "mv_records_bi_reset", maps=2)
    launch("mv_records_bi_reset", _lib.load().arseg_mv_records_bi_reset, _ptr(merged), _ptr(index_maps), index_maps.numel() * 4, H, W, _stream())


def mv_records_bi_step(records: torch.Tensor, merged: torch.Tensor, f: int, done_mask: int, index_maps: torch.Tensor, max_ref: int = 3,
                       policy="list0") -> torch.Tensor:
    """One frame of the two-list record chain (include/arseg_hip.h, arseg_mv_records_bi_*): frame f of a GOP pushed in decode order, with
    done_mask = the frames already chained (bit g = frame g; bit 0, the keyframe, always; bit f never).  A record's `reserved & 1` is its
    prediction list, `ref < 0` points forward in display order; policy "list0" | "near" | "mean" decides a pixel both of whose lists are
    usable.  Writes and returns the view merged[f]; two kernels, no synchronisation, no allocation."""
    n = _mv_records(records, "mv_records_bi_step")
    gop, H, W = _mv_chain_state(merged, index_maps, "mv_records_bi_step", maps=2)
    if records.device != merged.device:
        raise _lib.ArsegError(f"mv_records_bi_step: records are on {records.device}, merged on {merged.device}")
    if policy not in MV_BI_POLICIES:
        raise _lib.ArsegError(f"mv_records_bi_step: policy is one of {sorted(MV_BI_POLICIES)}, got {policy!r}")
    f, done_mask = int(f), int(done_mask)
    if gop > 64 or not 1 <= f < gop or not done_mask & 1 or (done_mask >> f) & 1 or done_mask < 0 or done_mask >> gop:
        raise _lib.ArsegError(f"mv_records_bi_step: gop <= 64, f in [1, gop), done_mask with bit 0 set, bit f clear and no bit >= gop; got gop {gop}, "
                              f"f {f}, done_mask {done_mask:#x}")
    launch("mv_records_bi_step", _lib.load().arseg_mv_records_bi_step_fwd, _ptr(records), n, _ptr(merged), f, gop, done_mask,
           MV_BI_POLICIES[policy], _ptr(index_maps), index_maps.numel() * 4, H, W, int(max_ref), _stream())
    return merged[f]


def mv_records_bi_step_link(records: torch.Tensor, merged: torch.Tensor, f: int, done_mask: int, index_maps: torch.Tensor, link: torch.Tensor,
                            link_stats: Optional[torch.Tensor] = None, max_ref: int = 3, policy="list0"):
    """mv_records_bi_step that also writes link[f] and adds to link_stats[f], as mv_records_step_link does for the P-frame step; under "mean"
    a pixel with both lists usable carries the flags of both and the larger hop count.  Returns the views (merged[f], link[f])."""
    n = _mv_records(records, "mv_records_bi_step_link")
    gop, H, W = _mv_chain_state(merged, index_maps, "mv_records_bi_step_link", maps=2)
    if records.device != merged.device:
        raise _lib.ArsegError(f"mv_records_bi_step_link: records are on {records.device}, merged on {merged.device}")
    if policy not in MV_BI_POLICIES:
        raise _lib.ArsegError(f"mv_records_bi_step_link: policy is one of {sorted(MV_BI_POLICIES)}, got {policy!r}")
    f, done_mask = int(f), int(done_mask)
    if gop > 64 or not 1 <= f < gop or not done_mask & 1 or (done_mask >> f) & 1 or done_mask < 0 or done_mask >> gop:
        raise _lib.ArsegError(f"mv_records_bi_step_link: gop <= 64, f in [1, gop), done_mask with bit 0 set, bit f clear and no bit >= gop; got gop {gop}, "
                              f"f {f}, done_mask {done_mask:#x}")
    _mv_link_state(link, link_stats, gop, H, W, merged.device, "mv_records_bi_step_link")
    launch("mv_records_bi_step_link", _lib.load().arseg_mv_records_bi_step_link_fwd, _ptr(records), n, _ptr(merged), f, gop, done_mask,
           MV_BI_POLICIES[policy], _ptr(index_maps), index_maps.numel() * 4, H, W, int(max_ref), _ptr(link), _ptr(link_stats), _stream())
    return merged[f], link[f]


def mv_records_rasterize(records: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Block records int16 [n,8] -> the dense field int16 [H,W,3] = (mvx, mvy, ref) the reference's decoder dumps per frame ((0, 0, -1)
    where no record covers a pixel): the rasterisation of mv_records_step alone."""
    n = _mv_records(records, "mv_records_rasterize")
    lib = _lib.load()
    nbytes = lib.arseg_mv_records_workspace_bytes(int(H), int(W))
    if nbytes == 0:
        raise _lib.ArsegError(f"mv_records_rasterize: H and W must be in 1..8192, got {H}x{W}")
    ws = workspace(nbytes, records.device)
    out = torch.empty((H, W, 3), dtype=torch.int16, device=records.device)
    launch("mv_records_rasterize", lib.arseg_mv_records_rasterize_fwd, _ptr(records), n, _ptr(out), _ptr(ws), nbytes, int(H), int(W), _stream())
    return out


def _luma_plane(t: torch.Tensor, src_format: int, what: str):
    """(H, W, row pitch in bytes) of the plane block_motion reads: [H,W] or [1,H,W] samples (uint8; uint16 or int16 bits for the 10-bit formats), for
    RGB8 [H,W,3] or [1,H,W,3] bytes; rows contiguous, any row pitch."""
    if src_format not in _SRC_PLANES:
        raise _lib.ArsegError(f"{what}: unknown source format {src_format!r}")
    dtype, tail = _SRC_PLANES[src_format][1], (3,) if src_format == _lib.SRC_RGB8 else ()
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.ArsegError(f"{what} runs on the GPU only (expected a CUDA tensor); ingest.block_motion_numpy is the host form")
    if t.dtype != dtype and not (dtype == torch.uint16 and t.dtype == torch.int16):
        raise _lib.ArsegError(f"{what}: expected {dtype} samples for source format {src_format}, got {t.dtype}")
    if t.dim() == 3 + len(tail) and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 + len(tail) or tuple(t.shape[2:]) != tail or 0 in t.shape:
        raise _lib.ArsegError(f"{what}: expected one frame [H,W{',3' if tail else ''}], got {tuple(t.shape)}")
    H, W = int(t.shape[0]), int(t.shape[1])
    row = W * (3 if tail else 1)
    if t.stride(1) != (3 if tail else 1) or (tail and t.stride(2) != 1) or (H > 1 and t.stride(0) < row):
        raise _lib.ArsegError(f"{what}: expected rows of contiguous samples at a pitch of at least a row, got strides {t.stride()}")
    return H, W, (t.stride(0) if H > 1 else row) * t.element_size()


def _bm_outputs(who: str, H: int, W: int, B: int, dev, records, sad, stats):
    """The output buffers of a block search over an H x W frame in blocks of B, checked or -- None -- allocated (stats zeroed); False leaves
    sad or stats out (None is returned for it)."""
    n = -(-H // B) * -(-W // B)
    if records is None:
        records = torch.empty((n, 8), dtype=torch.int16, device=dev)
    elif _mv_records(records, who) != n or records.device != dev:
        raise _lib.ArsegError(f"{who}: {H}x{W} in blocks of {B} is {n} records on {dev}, got {tuple(records.shape)} on {records.device}")
    if sad is None:
        sad = torch.empty(n, dtype=torch.int32, device=dev)
    elif sad is False:
        sad = None
    elif not torch.is_tensor(sad) or sad.dtype not in (torch.int32, torch.uint32) or sad.device != dev or sad.numel() != n or not sad.is_contiguous():
        raise _lib.ArsegError(f"{who} expects sad as a contiguous int32 (uint32 bits) tensor of {n} elements on {dev}")
    if stats is None:
        stats = torch.zeros(_lib.BM_NSTATS, dtype=torch.int64, device=dev)
    elif stats is False:
        stats = None
    elif not torch.is_tensor(stats) or stats.dtype != torch.int64 or stats.device != dev or stats.numel() != _lib.BM_NSTATS or not stats.is_contiguous():
        raise _lib.ArsegError(f"{who} expects stats as a contiguous int64 tensor of {_lib.BM_NSTATS} elements on {dev}")
    return records, sad, stats


def block_motion(cur_plane: torch.Tensor, ref_plane: torch.Tensor, src_format: int, B: int = 16, R: int = 16, lam: int = 2, intra: int = 255,
                 ref_index: int = 0, records: Optional[torch.Tensor] = None, sad=None, stats=None):
    """Block motion of one frame against a reference frame (include/arseg_hip.h, arseg_block_motion_fwd): full search of every B x B block of
    ``cur_plane``'s luma8 in ``ref_plane``'s, |dx|, |dy| <= R, cost = SAD + lam (|dx| + |dy|) -> the block records ``mv_records_step`` takes,
    int16 [ceil(H/B) * ceil(W/B), 8]; a block whose best SAD exceeds ``intra`` per pixel is written intra (ref = BM_INTRA_REF).  The planes
    are what ``DecodedFrames.luma_plane()`` returns.  ``records`` / ``sad`` (uint32 per block: the winner's SAD) / ``stats`` (int64
    [BM_NSTATS], accumulated into) are allocated when None -- stats zeroed -- and ``sad=False`` / ``stats=False`` leave that output out.
    One launch, no synchronisation; with all three buffers passed in, no allocation.  Returns (records, sad, stats)."""
    H, W, cur_pitch = _luma_plane(cur_plane, src_format, "block_motion (current frame)")
    H2, W2, ref_pitch = _luma_plane(ref_plane, src_format, "block_motion (reference frame)")
    B, R, lam, intra, ref_index = int(B), int(R), int(lam), int(intra), int(ref_index)
    if (H2, W2) != (H, W) or ref_plane.device != cur_plane.device:
        raise _lib.ArsegError(f"block_motion: the current frame is {H}x{W} on {cur_plane.device}, the reference {H2}x{W2} on {ref_plane.device}")
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or B not in (8, 16) or not 1 <= R <= 32 or not 0 <= lam <= 255 or not 0 <= intra <= 255 \
            or not 0 <= ref_index <= 15:
        raise _lib.ArsegError(f"block_motion: H, W in 1..8192, B in (8, 16), R in 1..32, lam and intra in 0..255, ref_index in 0..15; got {H}x{W}, "
                              f"B {B}, R {R}, lam {lam}, intra {intra}, ref_index {ref_index}")
    records, sad, stats = _bm_outputs("block_motion", H, W, B, cur_plane.device, records, sad, stats)
    launch("block_motion", _lib.load().arseg_block_motion_fwd, _ptr(cur_plane), cur_pitch, _ptr(ref_plane), ref_pitch, int(src_format), H, W, B, R, lam,
           intra, ref_index, _ptr(records), _ptr(sad), _ptr(stats), None, 0, _stream())
    return records, sad, stats


def _pyramid_buffer(t, H: int, W: int, levels: int, what: str) -> int:
    """Checks a luma pyramid buffer (contiguous CUDA uint8 of at least arseg_luma_pyramid_bytes elements, 16-byte aligned) and returns that size."""
    if not (1 <= H <= 8192 and 1 <= W <= 8192 and 1 <= levels <= 3):
        raise _lib.ArsegError(f"{what}: H, W in 1..8192 and levels in 1..3; got {H}x{W}, levels {levels}")
    nbytes = int(_lib.load().arseg_luma_pyramid_bytes(H, W, levels))
    if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.numel() < nbytes
                          or t.data_ptr() % 16):
        raise _lib.ArsegError(f"{what}: a pyramid of {H}x{W} with {levels} levels is a contiguous, 16-byte aligned CUDA uint8 tensor of {nbytes} bytes")
    return nbytes


def luma_pyramid(plane: torch.Tensor, src_format: int, levels: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The luma8 pyramid of one frame (include/arseg_hip.h, arseg_luma_pyramid_fwd): ``plane`` is what ``DecodedFrames.luma_plane()`` returns;
    level l of the flat uint8 buffer is at the offsets and pitches the header gives (``ingest.LumaPyramid`` holds the views).  One launch,
    no synchronisation; with ``out`` passed, no allocation."""
    H, W, pitch = _luma_plane(plane, src_format, "luma_pyramid")
    levels = int(levels)
    nbytes = _pyramid_buffer(out, H, W, levels, "luma_pyramid")
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=plane.device)
    elif out.device != plane.device:
        raise _lib.ArsegError(f"luma_pyramid: the plane is on {plane.device}, out on {out.device}")
    launch("luma_pyramid", _lib.load().arseg_luma_pyramid_fwd, _ptr(plane), pitch, int(src_format), H, W, levels, _ptr(out), out.numel(), _stream())
    return out


def block_motion_pyr(cur_pyr: torch.Tensor, ref_pyr: torch.Tensor, H: int, W: int, levels: int, B: int = 16, Rt: int = 8, r: int = 1, lam: int = 2,
                     intra: int = 255, ref_index: int = 0, records: Optional[torch.Tensor] = None, sad=None, stats=None,
                     workspace: Optional[torch.Tensor] = None):
    """Hierarchical block motion of one frame against a reference frame (include/arseg_hip.h, arseg_block_motion_pyr_fwd) from their luma
    pyramids (``luma_pyramid``): the full search with |dx|, |dy| <= Rt on level ``levels``, then per level below it +-r around twice the
    vectors of the parent block and of its two neighbours on the block's side -> the records, sad and stats of ``block_motion``, with its
    conventions for the three buffers.  ``workspace``: uint8, at least arseg_block_motion_pyr_workspace_bytes; None takes the host layer's.
    ``levels`` + 1 launches, no synchronisation; with all four buffers passed in, no allocation.  Returns (records, sad, stats)."""
    H, W, levels, B, Rt, r, lam, intra, ref_index = (int(v) for v in (H, W, levels, B, Rt, r, lam, intra, ref_index))
    _pyramid_buffer(cur_pyr, H, W, levels, "block_motion_pyr (current frame)")
    _pyramid_buffer(ref_pyr, H, W, levels, "block_motion_pyr (reference frame)")
    if cur_pyr is None or ref_pyr is None or cur_pyr.device != ref_pyr.device:
        raise _lib.ArsegError("block_motion_pyr: two pyramids on one device")
    if B not in (8, 16) or not 1 <= Rt <= 32 or not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 or not 0 <= ref_index <= 15:
        raise _lib.ArsegError(f"block_motion_pyr: B in (8, 16), Rt in 1..32, r in 1..3, lam and intra in 0..255, ref_index in 0..15; got B {B}, Rt {Rt}, "
                              f"r {r}, lam {lam}, intra {intra}, ref_index {ref_index}")
    dev = cur_pyr.device
    records, sad, stats = _bm_outputs("block_motion_pyr", H, W, B, dev, records, sad, stats)
    nbytes = int(_lib.load().arseg_block_motion_pyr_workspace_bytes(H, W, B, levels))
    if workspace is None:
        workspace = _base.workspace(nbytes, dev)
    elif not torch.is_tensor(workspace) or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous() \
            or workspace.numel() < nbytes or workspace.data_ptr() % 16:
        raise _lib.ArsegError(f"block_motion_pyr expects workspace as a contiguous, 16-byte aligned uint8 tensor of at least {nbytes} bytes on {dev}")
    launch("block_motion_pyr", _lib.load().arseg_block_motion_pyr_fwd, _ptr(cur_pyr), _ptr(ref_pyr), H, W, levels, B, Rt, r, lam, intra, ref_index,
           _ptr(records), _ptr(sad), _ptr(stats), _ptr(workspace), workspace.numel(), _stream())
    return records, sad, stats


def _aligned_luma_pair(who: str, cur_plane, key_plane):
    """The current frame's and the keyframe's uint8 luma planes as the keyframe anchor and the chain healing read them: one size in 1..8192, one
    device, the base 4-byte aligned and the pitch a multiple of 4 of at least (W + 3) & ~3.  Returns (H, W, device, cur_pitch, key_pitch)."""
    H, W, cur_pitch = _luma_plane(cur_plane, _lib.SRC_NV12, f"{who} (current frame)")
    H2, W2, key_pitch = _luma_plane(key_plane, _lib.SRC_NV12, f"{who} (keyframe)")
    dev = cur_plane.device
    if (H2, W2) != (H, W) or key_plane.device != dev:
        raise _lib.ArsegError(f"{who}: the current frame is {H}x{W} on {dev}, the keyframe {H2}x{W2} on {key_plane.device}")
    if not (1 <= H <= 8192 and 1 <= W <= 8192):
        raise _lib.ArsegError(f"{who}: H, W in 1..8192; got {H}x{W}")
    for what, t, pitch in (("current frame", cur_plane, cur_pitch), ("keyframe", key_plane, key_pitch)):
        if t.data_ptr() % 4 or pitch % 4 or pitch < ((W + 3) & ~3):
            raise _lib.ArsegError(f"{who} ({what}): the plane's base must be 4-byte aligned and its pitch a multiple of 4 of at least "
                                  f"{(W + 3) & ~3} bytes, got an offset of {t.data_ptr() % 4} and a pitch of {pitch} (level 0 of a LumaPyramid qualifies)")
    return H, W, dev, cur_pitch, key_pitch


def block_motion_anchor(cur_plane: torch.Tensor, key_plane: torch.Tensor, records: torch.Tensor, merged_prev: Optional[torch.Tensor], f: int, B: int = 16,
                        r: int = 2, lam: int = 2, intra: int = 255, out: Optional[torch.Tensor] = None, sad=None, stats=None):
    """Anchors the estimated hop records of frame ``f`` on the keyframe (include/arseg_hip.h, arseg_block_motion_anchor_fwd): every block of
    ``cur_plane`` is matched in ``key_plane`` within +-r of the displacement the chain would compose for it from ``records`` and
    ``merged_prev`` (= merged[f - 1], int16 [H,W,2]; None at f = 1) and of its neighbours' and the co-located one; a block whose best SAD
    is at most ``intra`` per pixel gets a record with ref = f - 1 (target: the keyframe), any other keeps its hop record.  The planes are
    uint8 luma planes [H,W] with a 4-byte aligned base and pitch (level 0 of a ``LumaPyramid``, an aligned NV12 / I420 luma plane).
    ``out`` / ``sad`` / ``stats`` with ``block_motion``'s conventions, except that sad is read-modify-write (entries of anchored blocks
    only; allocated zeroed) and stats is int64 [BMA_NSTATS].  ``out`` must not overlap ``records``.  One launch, no synchronisation; with
    all three buffers passed in, no allocation.  Returns (out, sad, stats)."""
    H, W, dev, cur_pitch, key_pitch = _aligned_luma_pair("block_motion_anchor", cur_plane, key_plane)
    f, B, r, lam, intra = int(f), int(B), int(r), int(lam), int(intra)
    if B not in (8, 16) or not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 or not 1 <= f <= 16:
        raise _lib.ArsegError(f"block_motion_anchor: H, W in 1..8192, B in (8, 16), r in 1..3, lam and intra in 0..255, f in 1..16; got {H}x{W}, B {B}, "
                              f"r {r}, lam {lam}, intra {intra}, f {f}")
    n = -(-H // B) * -(-W // B)
    if _mv_records(records, "block_motion_anchor") != n or records.device != dev:
        raise _lib.ArsegError(f"block_motion_anchor: {H}x{W} in blocks of {B} is {n} records on {dev}, got {tuple(records.shape)} on {records.device}")
    if merged_prev is None:
        if f >= 2:
            raise _lib.ArsegError(f"block_motion_anchor: frame {f} needs merged_prev = merged[{f - 1}]")
    elif not torch.is_tensor(merged_prev) or merged_prev.dtype != torch.int16 or merged_prev.device != dev or tuple(merged_prev.shape) != (H, W, 2) \
            or not merged_prev.is_contiguous():
        raise _lib.ArsegError(f"block_motion_anchor expects merged_prev as a contiguous int16 tensor [{H},{W},2] on {dev}")
    if sad is None:
        sad = torch.zeros(n, dtype=torch.int32, device=dev)
    out, sad, stats = _bm_outputs("block_motion_anchor", H, W, B, dev, out, sad, stats)
    lo, hi = records.data_ptr(), records.data_ptr() + 16 * n
    if out.data_ptr() < hi and lo < out.data_ptr() + 16 * n:
        raise _lib.ArsegError("block_motion_anchor: out must not overlap records (neighbour blocks read the input while the output is written)")
    launch("block_motion_anchor", _lib.load().arseg_block_motion_anchor_fwd, _ptr(cur_plane), cur_pitch, _ptr(key_plane), key_pitch, H, W, B, r, lam, intra, f,
           _ptr(records), _ptr(merged_prev), _ptr(out), _ptr(sad), _ptr(stats), _stream())
    return out, sad, stats


def block_motion_split(cur_plane: torch.Tensor, ref_plane: torch.Tensor, records_in: torch.Tensor, r: int = 2, lam: int = 2, intra: int = 255,
                       split_gain: int = 32, ref_index: int = 0, children: Optional[torch.Tensor] = None, sad=None, stats=None):
    """Splits estimated 16 x 16 block records into 8 x 8 children where that pays (include/arseg_hip.h, arseg_block_motion_split_fwd): the four
    children of every parent of ``records_in`` (int16 [n,8], the B = 16 grid of ``block_motion``) are searched in ``ref_plane`` within +-r of
    (0, 0), of the parent's vector and of its neighbours' on the child's side; a parent is split where its children's costs undercut its own
    by more than ``split_gain``, an intra parent where a child matches.  ``children`` int16 [4 n,8] gets a record per child of a split parent
    and eight zeros -- a record that covers nothing -- everywhere else, so ``records_in`` followed by ``children`` is one list of 5 n records
    for ``mv_records_step``.  The planes are as ``block_motion_anchor`` takes them.  ``children`` / ``sad`` (uint32 [4 n]: every existing
    child's SAD) / ``stats`` (int64 [BMS_NSTATS], accumulated into) with ``block_motion``'s conventions.  ``children`` must not overlap
    ``records_in``.  One launch, no synchronisation; with all three buffers passed in, no allocation.  Returns (children, sad, stats)."""
    H, W, dev, cur_pitch, ref_pitch = _aligned_luma_pair("block_motion_split", cur_plane, ref_plane)
    r, lam, intra, split_gain, ref_index = int(r), int(lam), int(intra), int(split_gain), int(ref_index)
    if not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 or not 0 <= split_gain <= 65535 or not 0 <= ref_index <= 15:
        raise _lib.ArsegError(f"block_motion_split: r in 1..3, lam and intra in 0..255, split_gain in 0..65535, ref_index in 0..15; got r {r}, lam {lam}, "
                              f"intra {intra}, split_gain {split_gain}, ref_index {ref_index}")
    n = -(-H // 16) * -(-W // 16)
    if _mv_records(records_in, "block_motion_split") != n or records_in.device != dev:
        raise _lib.ArsegError(f"block_motion_split: {H}x{W} in blocks of 16 is {n} records on {dev}, got {tuple(records_in.shape)} on {records_in.device}")
    if children is None:
        children = torch.empty((4 * n, 8), dtype=torch.int16, device=dev)
    elif _mv_records(children, "block_motion_split") != 4 * n or children.device != dev:
        raise _lib.ArsegError(f"block_motion_split: {n} parents have {4 * n} child records on {dev}, got {tuple(children.shape)} on {children.device}")
    if sad is None:
        sad = torch.empty(4 * n, dtype=torch.int32, device=dev)
    elif sad is False:
        sad = None
    elif not torch.is_tensor(sad) or sad.dtype not in (torch.int32, torch.uint32) or sad.device != dev or sad.numel() != 4 * n or not sad.is_contiguous():
        raise _lib.ArsegError(f"block_motion_split expects sad as a contiguous int32 (uint32 bits) tensor of {4 * n} elements on {dev}")
    if stats is None:
        stats = torch.zeros(_lib.BMS_NSTATS, dtype=torch.int64, device=dev)
    elif stats is False:
        stats = None
    elif not torch.is_tensor(stats) or stats.dtype != torch.int64 or stats.device != dev or stats.numel() != _lib.BMS_NSTATS or not stats.is_contiguous():
        raise _lib.ArsegError(f"block_motion_split expects stats as a contiguous int64 tensor of {_lib.BMS_NSTATS} elements on {dev}")
    lo, hi = records_in.data_ptr(), records_in.data_ptr() + 16 * n
    if children.data_ptr() < hi and lo < children.data_ptr() + 64 * n:
        raise _lib.ArsegError("block_motion_split: children must not overlap records_in (neighbour parents are read while the children are written)")
    launch("block_motion_split", _lib.load().arseg_block_motion_split_fwd, _ptr(cur_plane), cur_pitch, _ptr(ref_plane), ref_pitch, H, W, r, lam, intra,
           split_gain, ref_index, _ptr(records_in), _ptr(children), _ptr(sad), _ptr(stats), _stream())
    return children, sad, stats


def mv_chain_heal(cur_plane: torch.Tensor, key_plane: torch.Tensor, merged_f: torch.Tensor, link_f: torch.Tensor, B: int = 16, r: int = 2, lam: int = 2,
                  intra: int = 20, flag_mask: int = _lib.LINK_INTRA | _lib.LINK_UNCOVERED, min_flagged: int = 1, decisions: Optional[torch.Tensor] = None,
                  sad=None, stats=None, link_stats_row=None):
    """Heals the flagged pixels of one frame of a motion chain on the keyframe (include/arseg_hip.h, arseg_mv_chain_heal_fwd), IN PLACE:
    ``merged_f`` int16 [H,W,2] and ``link_f`` uint8 [H,W] are merged[f] and link[f] as the chain's step left them.  Every B x B block with at
    least ``min_flagged`` pixels whose link byte has a bit of ``flag_mask`` is matched in ``key_plane`` within +-r of the chain's own vector at
    its centre, of its neighbours' where those are unflagged, of its own first unflagged pixel and of (0, 0); where the winner's SAD over the
    flagged pixels is at most ``intra`` per flagged pixel they get (4 dx, 4 dy) and the link byte 0x10.  The planes are as
    ``block_motion_anchor`` takes them.  ``decisions`` (int16 [n,8]: x0, y0, w, h, 4 dx, 4 dy, state, flagged pixels; state 0 healed, 1 kept,
    2 skipped) / ``sad`` (uint32 per block, examined blocks only; allocated zeroed) / ``stats`` (int64 [HEAL_NSTATS], accumulated into) with
    ``block_motion``'s conventions; ``link_stats_row`` (int64 [LINK_NSTATS], row f of the chain's counters, corrected to a recount of the new
    plane) is left out when None or False.  Two launches, no synchronisation; with the buffers passed in, no allocation.  Returns
    (decisions, sad, stats)."""
    H, W, dev, cur_pitch, key_pitch = _aligned_luma_pair("mv_chain_heal", cur_plane, key_plane)
    B, r, lam, intra, flag_mask, min_flagged = int(B), int(r), int(lam), int(intra), int(flag_mask), int(min_flagged)
    if B not in (8, 16) or not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 or not 1 <= flag_mask <= 7 or not 1 <= min_flagged <= 64:
        raise _lib.ArsegError(f"mv_chain_heal: B in (8, 16), r in 1..3, lam and intra in 0..255, flag_mask in 1..7, min_flagged in 1..64; got B {B}, "
                              f"r {r}, lam {lam}, intra {intra}, flag_mask {flag_mask}, min_flagged {min_flagged}")
    if not torch.is_tensor(merged_f) or merged_f.dtype != torch.int16 or merged_f.device != dev or tuple(merged_f.shape) != (H, W, 2) or not merged_f.is_contiguous() \
            or merged_f.data_ptr() % 4:
        raise _lib.ArsegError(f"mv_chain_heal expects merged_f as a contiguous, 4-byte aligned int16 tensor [{H},{W},2] on {dev}")
    if not torch.is_tensor(link_f) or link_f.dtype != torch.uint8 or link_f.device != dev or tuple(link_f.shape) != (H, W) or not link_f.is_contiguous():
        raise _lib.ArsegError(f"mv_chain_heal expects link_f as a contiguous uint8 tensor [{H},{W}] on {dev}")
    n = -(-H // B) * -(-W // B)
    if sad is None:
        sad = torch.zeros(n, dtype=torch.int32, device=dev)
    decisions, sad, _ = _bm_outputs("mv_chain_heal", H, W, B, dev, decisions, sad, False)
    for name, t, size in (("stats", stats, _lib.HEAL_NSTATS), ("link_stats_row", link_stats_row, _lib.LINK_NSTATS)):
        if t is not None and t is not False and (not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != dev or t.numel() != size or not t.is_contiguous()
                                                 or t.data_ptr() % 8):
            raise _lib.ArsegError(f"mv_chain_heal expects {name} as a contiguous int64 tensor of {size} elements on {dev}")
    if stats is None:
        stats = torch.zeros(_lib.HEAL_NSTATS, dtype=torch.int64, device=dev)
    elif stats is False:
        stats = None
    if link_stats_row is False:
        link_stats_row = None
    launch("mv_chain_heal", _lib.load().arseg_mv_chain_heal_fwd, _ptr(cur_plane), cur_pitch, _ptr(key_plane), key_pitch, H, W, B, r, lam, intra, flag_mask,
           min_flagged, _ptr(merged_f), _ptr(link_f), _ptr(decisions), _ptr(sad), _ptr(stats), _ptr(link_stats_row), _stream())
    return decisions, sad, stats


def argmax_confusion(logits: torch.Tensor, label: Optional[torch.Tensor], H: int, W: int, hist: Optional[torch.Tensor] = None,
                     ignore_label: int = 255, want_pred: bool = True, align_corners: bool = True):
    """Evaluator tail (evaluation.py:201-209): returns (pred int32 [N,H,W] or None, hist int64 [n_cls,n_cls] or None).
    ``align_corners=False``: the resize is BiSeNetOutput's ``nn.Upsample(x8, align_corners=False)`` (model/bisenet.py:215-216) --
    head logits at 1/8 resolution go straight to the argmax, the full-resolution logits are never written."""
    _need_gpu(logits)
    logits = logits.contiguous()
    N, n_cls, h, w = logits.shape
    pred = torch.empty((N, H, W), dtype=torch.int32, device=logits.device) if want_pred else None
    if label is not None:
        _need_gpu(label, dtype=torch.int64)
        label = label.contiguous()
        if hist is None:
            hist = torch.zeros((n_cls, n_cls), dtype=torch.int64, device=logits.device)
    launch("argmax_confusion", _lib.load().arseg_argmax_confusion_fwd, _ptr(logits), _ptr(label), _ptr(pred), _ptr(hist if label is not None else None), N,
                                                 n_cls, h, w, H, W, ignore_label, 1 if align_corners else 0, _stream())
    return pred, hist


_group_uploads = {}          # (group ids, device) -> int32 device tensor: a replayed GOP step uploads nothing


def _group_ids(groups, n_groups: int):
    """A Python sequence of group ids, range-checked on the host -> tuple; a tensor -> None (never read here)."""
    if n_groups < 1:
        raise ValueError(f"n_groups must be positive, got {n_groups}")
    if torch.is_tensor(groups):
        return None
    ids = tuple(int(g) for g in groups)
    bad = [g for g in ids if not 0 <= g < n_groups]
    if bad:
        raise ValueError(f"group id {bad[0]} is outside [0, {n_groups})")
    return ids


def _groups_tensor(groups, ids, N: int, device) -> torch.Tensor:
    if ids is None:                      # a tensor is taken as is: no host read, ids outside [0, n_groups) count nowhere
        if not groups.is_cuda or groups.dtype != torch.int32 or groups.dim() != 1 or groups.shape[0] != N:
            raise _lib.ArsegError(f"groups: expected an int32 GPU tensor [{N}], got {groups.dtype} {tuple(groups.shape)} on {groups.device}")
        return groups.contiguous()
    if len(ids) != N:
        raise ValueError(f"groups names {len(ids)} frames, the batch has {N}")
    key = (ids, str(device))
    t = _group_uploads.get(key)
    if t is None:
        if len(_group_uploads) >= 256:
            _group_uploads.clear()
        t = _group_uploads[key] = torch.tensor(ids, dtype=torch.int32, device=device)
    return t


def argmax_confusion_grouped(logits: torch.Tensor, label: Optional[torch.Tensor], groups, n_groups: int, H: int, W: int,
                             hist: Optional[torch.Tensor] = None, ignore_label: int = 255, want_pred: bool = True, align_corners: bool = True):
    """The evaluator tail with one confusion matrix per group of frames (the reference reports the mIoU per keyframe distance,
    evaluation.py:272-303): frame n counts into hist[groups[n]].  Returns (pred int32 [N,H,W] or None, hist int64 [n_groups,n_cls,n_cls]
    or None); pred is bit-equal to ``argmax_confusion``'s.  ``groups``: an int32 GPU tensor [N] (taken as is; a frame whose id is outside
    [0, n_groups) is labelled and counted nowhere) or a sequence of ints (range-checked here, uploaded once per distinct sequence)."""
    ids = _group_ids(groups, n_groups)
    _need_gpu(logits)
    logits = logits.contiguous()
    N, n_cls, h, w = logits.shape
    pred = torch.empty((N, H, W), dtype=torch.int32, device=logits.device) if want_pred else None
    grp = None
    if label is not None:
        _need_gpu(label, dtype=torch.int64)
        label = label.contiguous()
        grp = _groups_tensor(groups, ids, N, logits.device)
        if hist is None:
            hist = torch.zeros((n_groups, n_cls, n_cls), dtype=torch.int64, device=logits.device)
        elif tuple(hist.shape) != (n_groups, n_cls, n_cls) or hist.dtype != torch.int64 or not hist.is_cuda or not hist.is_contiguous():
            raise _lib.ArsegError(f"hist: expected a contiguous int64 GPU tensor [{n_groups},{n_cls},{n_cls}], got {hist.dtype} {tuple(hist.shape)}")
    launch("argmax_confusion_grouped", _lib.load().arseg_argmax_confusion_grouped_fwd, _ptr(logits), _ptr(label), _ptr(grp), _ptr(pred),
           _ptr(hist if label is not None else None), N, n_groups, n_cls, h, w, H, W, ignore_label, 1 if align_corners else 0, _stream())
    return pred, hist


_stream_workspace = workspace          # (label_bands takes a ``workspace`` argument of its own)


def band_radii(radii) -> tuple:
    """The radii of ``label_bands`` as a tuple of ints after their check: 1 .. 8 of them, each in 1 .. 32, strictly ascending."""
    r = tuple(int(v) for v in radii)
    if not 1 <= len(r) <= 8 or any(not 1 <= v <= 32 for v in r) or any(b <= a for a, b in zip(r, r[1:])):
        raise ValueError(f"radii: 1 to 8 strictly ascending integers in 1..32, got {r}")
    return r


def label_bands(label: torch.Tensor, radii, pred: Optional[torch.Tensor] = None, groups=None, n_groups: int = 1, n_cls: Optional[int] = None,
                hist: Optional[torch.Tensor] = None, ignore_label: int = 255, band_out=None, workspace: Optional[torch.Tensor] = None):
    """Confusion counts in bands around the label boundaries (include/arseg_hip.h, arseg_label_bands_fwd): ``label`` int64 [N,H,W] and
    ``pred`` int32 [N,H,W] (``argmax_confusion*``'s) -> ``hist`` int64 [n_groups, len(radii) + 1, n_cls, n_cls], accumulated: frame n counts
    into hist[groups[n]][band], the band of a pixel being the first radius its Chebyshev distance to a pixel of another label (void is
    one label) does not exceed, ``len(radii)`` for the interior.  The sum over the bands is ``argmax_confusion_grouped``'s hist.
    ``groups`` as ``argmax_confusion_grouped`` takes them, or None with ``n_groups == 1``.  ``n_cls``: default ``hist.shape[-1]``.
    ``band_out``: a uint8 [N,H,W] plane (rows contiguous, any pitch / image stride) for the band of every pixel, True to have it
    allocated, None for no plane -- except without ``pred``, where the plane is all the call gives (``hist`` must then be None too).
    ``workspace``: a device tensor of at least ``arseg_label_bands_workspace_bytes(N, H, W)`` bytes (default: the stream's shared one).
    One ABI call; with every buffer given nothing is allocated and nothing synchronises.  Returns (bands or None, hist or None)."""
    what = "label_bands"
    rad = band_radii(radii)
    ids = None if groups is None else _group_ids(groups, n_groups)
    if groups is None and n_groups != 1:
        raise ValueError(f"{what}: groups=None needs n_groups == 1, got {n_groups}")
    if pred is None and hist is not None:
        raise ValueError(f"{what}: hist needs pred")
    _need_gpu(label, dtype=torch.int64)
    if label.dim() != 3 or not label.is_contiguous():
        raise _lib.ArsegError(f"{what}: label must be a contiguous int64 [N,H,W] tensor, got {tuple(label.shape)} strides {label.stride()}")
    N, H, W = label.shape
    dev = label.device
    if n_cls is None:
        if hist is None:
            raise ValueError(f"{what}: n_cls is required without hist")
        n_cls = hist.shape[-1]
    n_cls = int(n_cls)
    if not 1 <= n_cls <= 32:
        raise ValueError(f"{what}: 1..32 classes, got {n_cls}")
    grp = None
    if pred is not None:
        _need_gpu(pred, dtype=torch.int32)
        if tuple(pred.shape) != (N, H, W) or not pred.is_contiguous() or pred.device != dev:
            raise _lib.ArsegError(f"{what}: pred must be a contiguous int32 {(N, H, W)} tensor on {dev}, got {tuple(pred.shape)} on {pred.device}")
        if groups is not None:
            grp = _groups_tensor(groups, ids, N, dev)
        shape = (n_groups, len(rad) + 1, n_cls, n_cls)
        if hist is None:
            hist = torch.zeros(shape, dtype=torch.int64, device=dev)
        elif tuple(hist.shape) != shape or hist.dtype != torch.int64 or hist.device != dev or not hist.is_contiguous():
            raise _lib.ArsegError(f"{what}: hist must be a contiguous int64 GPU tensor {list(shape)}, got {hist.dtype} {tuple(hist.shape)}")
    if band_out is True or (band_out is None and pred is None):
        band_out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    pitch, ns = 0, 0
    if band_out is not None:
        _need_gpu(band_out, dtype=torch.uint8)
        if tuple(band_out.shape) != (N, H, W) or band_out.device != dev:
            raise ValueError(f"{what}: band_out must be uint8 {(N, H, W)} on {dev}, got {tuple(band_out.shape)} on {band_out.device}")
        pitch, ns = _plane_layout(band_out, (W,), f"{what} band_out")
    lib = _lib.load()
    need = lib.arseg_label_bands_workspace_bytes(N, H, W)
    if need == 0:
        raise ValueError(f"{what}: frames of 1..16384 rows and columns, got {H}x{W}")
    if workspace is None:
        workspace = _stream_workspace(need, dev)
    elif not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous() or workspace.data_ptr() % 2 or \
            workspace.numel() * workspace.element_size() < need:
        raise _lib.ArsegError(f"{what}: workspace must be a contiguous, 2-byte aligned tensor of at least {need} bytes on {dev}")
    launch(what, lib.arseg_label_bands_fwd, _ptr(label), _ptr(pred), _ptr(grp), (ctypes.c_int * len(rad))(*rad), len(rad), _ptr(band_out), pitch, ns,
           _ptr(hist), N, n_groups, n_cls, H, W, int(ignore_label), _ptr(workspace), workspace.numel() * workspace.element_size(), _stream(),
           nbytes=N * H * W * (8 + 4 + (4 if pred is not None else 0) + (1 if band_out is not None else 0)))
    return band_out, hist


def boundary_radii(radii) -> tuple:
    """The radii of ``boundary_iou`` as a tuple of ints after their check: 1 .. 8 of them, each in 1 .. 64, strictly ascending."""
    r = tuple(int(v) for v in radii)
    if not 1 <= len(r) <= 8 or any(not 1 <= v <= 64 for v in r) or any(b <= a for a, b in zip(r, r[1:])):
        raise ValueError(f"radii: 1 to 8 strictly ascending integers in 1..64, got {r}")
    return r


def boundary_radius(H: int, W: int, ratio: float = 0.02) -> int:
    """The band width of Boundary IoU (Cheng et al., CVPR 2021) in pixels: ``ratio`` of the image diagonal, at least 1."""
    return max(1, int(round(ratio * math.sqrt(H * H + W * W))))


def _band_plane(what, name, plane, N, H, W, dev):
    """A band plane argument (None / True / a uint8 [N,H,W] tensor) -> (tensor or None, row pitch, image stride)."""
    if plane is None:
        return None, 0, 0
    if plane is True:
        plane = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    _need_gpu(plane, dtype=torch.uint8)
    if tuple(plane.shape) != (N, H, W) or plane.device != dev:
        raise ValueError(f"{what}: {name} must be uint8 {(N, H, W)} on {dev}, got {tuple(plane.shape)} on {plane.device}")
    pitch, ns = _plane_layout(plane, (W,), f"{what} {name}")
    return plane, pitch, ns


def boundary_iou(label: torch.Tensor, pred: torch.Tensor, radii, groups=None, n_groups: int = 1, n_cls: Optional[int] = None,
                 counts: Optional[torch.Tensor] = None, ignore_label: int = 255, border: bool = True, label_band_out=None, pred_band_out=None,
                 workspace: Optional[torch.Tensor] = None):
    """Boundary IoU counts from joint label / prediction bands (include/arseg_hip.h, arseg_boundary_iou_fwd): ``label`` int64 [N,H,W] and
    ``pred`` int32 [N,H,W] -> ``counts`` int64 [n_groups, 3, len(radii) + 1, n_cls], accumulated: per band of Chebyshev distance to the
    nearest other byte of the label plane / of the prediction plane (and, with ``border``, to the image border) the pixels of the
    ground-truth mask (row 0), of the predicted mask (row 1) and of both (row 2, at the larger of the two bands).  Summed over the bands
    the rows are the row sums, column sums and diagonal of ``argmax_confusion_grouped``'s hist.  ``groups`` as ``argmax_confusion_grouped``
    takes them, or None with ``n_groups == 1``.  ``n_cls``: default ``counts.shape[-1]``.  ``label_band_out`` / ``pred_band_out``: a
    uint8 [N,H,W] plane (rows contiguous, any pitch / image stride), True to have it allocated, None for no plane.  ``workspace``: a
    device tensor of at least ``arseg_boundary_iou_workspace_bytes(N, H, W)`` bytes (default: the stream's shared one).  One ABI call;
    with every buffer given nothing is allocated and nothing synchronises.  Returns (counts, label bands or None, pred bands or None)."""
    what = "boundary_iou"
    rad = boundary_radii(radii)
    ids = None if groups is None else _group_ids(groups, n_groups)
    if groups is None and n_groups != 1:
        raise ValueError(f"{what}: groups=None needs n_groups == 1, got {n_groups}")
    _need_gpu(label, dtype=torch.int64)
    if label.dim() != 3 or not label.is_contiguous():
        raise _lib.ArsegError(f"{what}: label must be a contiguous int64 [N,H,W] tensor, got {tuple(label.shape)} strides {label.stride()}")
    N, H, W = label.shape
    dev = label.device
    _need_gpu(pred, dtype=torch.int32)
    if tuple(pred.shape) != (N, H, W) or not pred.is_contiguous() or pred.device != dev:
        raise _lib.ArsegError(f"{what}: pred must be a contiguous int32 {(N, H, W)} tensor on {dev}, got {tuple(pred.shape)} on {pred.device}")
    if n_cls is None:
        if counts is None:
            raise ValueError(f"{what}: n_cls is required without counts")
        n_cls = counts.shape[-1]
    n_cls = int(n_cls)
    if not 1 <= n_cls <= 32:
        raise ValueError(f"{what}: 1..32 classes, got {n_cls}")
    grp = None if groups is None else _groups_tensor(groups, ids, N, dev)
    shape = (n_groups, 3, len(rad) + 1, n_cls)
    if counts is None:
        counts = torch.zeros(shape, dtype=torch.int64, device=dev)
    elif tuple(counts.shape) != shape or counts.dtype != torch.int64 or counts.device != dev or not counts.is_contiguous():
        raise _lib.ArsegError(f"{what}: counts must be a contiguous int64 GPU tensor {list(shape)}, got {counts.dtype} {tuple(counts.shape)}")
    label_band_out, lpitch, lns = _band_plane(what, "label_band_out", label_band_out, N, H, W, dev)
    pred_band_out, ppitch, pns = _band_plane(what, "pred_band_out", pred_band_out, N, H, W, dev)
    lib = _lib.load()
    need = lib.arseg_boundary_iou_workspace_bytes(N, H, W)
    if need == 0:
        raise ValueError(f"{what}: frames of 1..16384 rows and columns, got {H}x{W}")
    if workspace is None:
        workspace = _stream_workspace(need, dev)
    elif not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous() or workspace.data_ptr() % 2 or \
            workspace.numel() * workspace.element_size() < need:
        raise _lib.ArsegError(f"{what}: workspace must be a contiguous, 2-byte aligned tensor of at least {need} bytes on {dev}")
    launch(what, lib.arseg_boundary_iou_fwd, _ptr(label), _ptr(pred), _ptr(grp), (ctypes.c_int * len(rad))(*rad), len(rad), 1 if border else 0,
           _ptr(label_band_out), lpitch, lns, _ptr(pred_band_out), ppitch, pns, _ptr(counts), N, n_groups, n_cls, H, W, int(ignore_label),
           _ptr(workspace), workspace.numel() * workspace.element_size(), _stream(),
           nbytes=N * H * W * (12 + 8 + (1 if label_band_out is not None else 0) + (1 if pred_band_out is not None else 0)))
    return counts, label_band_out, pred_band_out


def contour_radii(radii) -> tuple:
    """The radii of ``contour_f`` as a tuple of ints after their check: 1 .. 8 of them, each in 0 .. 32, strictly ascending."""
    r = tuple(int(v) for v in radii)
    if not 1 <= len(r) <= 8 or any(not 0 <= v <= 32 for v in r) or any(b <= a for a, b in zip(r, r[1:])):
        raise ValueError(f"radii: 1 to 8 strictly ascending integers in 0..32, got {r}")
    return r


def contour_radius(H: int, W: int, ratio: float = 0.008) -> int:
    """The contour tolerance of the DAVIS protocol's F-measure in pixels: ``ratio`` of the image diagonal, rounded up."""
    return int(math.ceil(ratio * math.sqrt(H * H + W * W)))


def contour_f(label: torch.Tensor, pred: torch.Tensor, radii, groups=None, n_groups: int = 1, n_cls: Optional[int] = None,
              counts: Optional[torch.Tensor] = None, ignore_label: int = 255, label_match_out=None, pred_match_out=None,
              workspace: Optional[torch.Tensor] = None):
    """Contour F-measure counts from matched class contours (include/arseg_hip.h, arseg_contour_f_fwd): ``label`` int64 [N,H,W] and
    ``pred`` int32 [N,H,W] -> ``counts`` int64 [n_groups, 2, len(radii) + 1, n_cls], accumulated: the contour pixels of the ground truth
    (row 0) and of the prediction (row 1) per class and band of Euclidean distance to the nearest contour pixel of the same class on the
    other plane -- band k: within radii[k] and not within radii[k - 1]; the last band: unmatched.  Recall at radii[k] is row 0 summed over
    the bands 0 .. k over row 0 summed over all bands, precision the same on row 1 (``evaluation.ContourTable``).  ``groups`` as
    ``argmax_confusion_grouped`` takes them, or None with ``n_groups == 1``.  ``n_cls``: default ``counts.shape[-1]``.
    ``label_match_out`` / ``pred_match_out``: a uint8 [N,H,W] plane (rows contiguous, any pitch / image stride) for the band of every
    contour pixel of that plane (255 elsewhere), True to have it allocated, None for no plane.  ``workspace``: a device tensor of at
    least ``arseg_contour_f_workspace_bytes(N, H, W)`` bytes (default: the stream's shared one).  One ABI call; with every buffer given
    nothing is allocated and nothing synchronises.  Returns (counts, label plane or None, pred plane or None)."""
    what = "contour_f"
    rad = contour_radii(radii)
    ids = None if groups is None else _group_ids(groups, n_groups)
    if groups is None and n_groups != 1:
        raise ValueError(f"{what}: groups=None needs n_groups == 1, got {n_groups}")
    _need_gpu(label, dtype=torch.int64)
    if label.dim() != 3 or not label.is_contiguous():
        raise _lib.ArsegError(f"{what}: label must be a contiguous int64 [N,H,W] tensor, got {tuple(label.shape)} strides {label.stride()}")
    N, H, W = label.shape
    dev = label.device
    _need_gpu(pred, dtype=torch.int32)
    if tuple(pred.shape) != (N, H, W) or not pred.is_contiguous() or pred.device != dev:
        raise _lib.ArsegError(f"{what}: pred must be a contiguous int32 {(N, H, W)} tensor on {dev}, got {tuple(pred.shape)} on {pred.device}")
    if n_cls is None:
        if counts is None:
            raise ValueError(f"{what}: n_cls is required without counts")
        n_cls = counts.shape[-1]
    n_cls = int(n_cls)
    if not 1 <= n_cls <= 32:
        raise ValueError(f"{what}: 1..32 classes, got {n_cls}")
    grp = None if groups is None else _groups_tensor(groups, ids, N, dev)
    shape = (n_groups, 2, len(rad) + 1, n_cls)
    if counts is None:
        counts = torch.zeros(shape, dtype=torch.int64, device=dev)
    elif tuple(counts.shape) != shape or counts.dtype != torch.int64 or counts.device != dev or not counts.is_contiguous():
        raise _lib.ArsegError(f"{what}: counts must be a contiguous int64 GPU tensor {list(shape)}, got {counts.dtype} {tuple(counts.shape)}")
    label_match_out, lpitch, lns = _band_plane(what, "label_match_out", label_match_out, N, H, W, dev)
    pred_match_out, ppitch, pns = _band_plane(what, "pred_match_out", pred_match_out, N, H, W, dev)
    lib = _lib.load()
    need = lib.arseg_contour_f_workspace_bytes(N, H, W)
    if need == 0:
        raise ValueError(f"{what}: frames of 1..16384 rows and columns, got {H}x{W}")
    if workspace is None:
        workspace = _stream_workspace(need, dev)
    elif not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous() or workspace.data_ptr() % 2 or \
            workspace.numel() * workspace.element_size() < need:
        raise _lib.ArsegError(f"{what}: workspace must be a contiguous, 2-byte aligned tensor of at least {need} bytes on {dev}")
    launch(what, lib.arseg_contour_f_fwd, _ptr(label), _ptr(pred), _ptr(grp), (ctypes.c_int * len(rad))(*rad), len(rad),
           _ptr(label_match_out), lpitch, lns, _ptr(pred_match_out), ppitch, pns, _ptr(counts), N, n_groups, n_cls, H, W, int(ignore_label),
           _ptr(workspace), workspace.numel() * workspace.element_size(), _stream(),
           nbytes=N * H * W * (12 + 4 + (1 if label_match_out is not None else 0) + (1 if pred_match_out is not None else 0)))
    return counts, label_match_out, pred_match_out


_CAL_KINDS = {"top1": _lib.CONF_TOP1, "margin": _lib.CONF_MARGIN}


def calibration(logits: torch.Tensor, label: torch.Tensor, H: int, W: int, groups=None, n_groups: int = 1, cal: Optional[torch.Tensor] = None,
                ignore_label: int = 255, kind: str = "top1", align_corners: bool = True):
    """Calibration counts of the confidence code (include/arseg_hip.h, arseg_calibration_fwd): head logits fp32 [N,n_cls,h,w] and ``label``
    int64 [N,H,W] -> ``cal`` int64 [n_groups, n_cls, 256, 2], accumulated: per group of frames, predicted class k* and 8-bit code q
    (``segment_confidence``'s labels and codes, bit for bit, ``kind`` and ``align_corners`` as it takes them) the pixels with a valid
    label (column 0) and those of them whose label is k* (column 1).  Summed over the codes, column 0 is the column sums and column 1
    the diagonal of ``argmax_confusion_grouped``'s hist.  ``groups`` as ``argmax_confusion_grouped`` takes them, or None with
    ``n_groups == 1``.  One ABI call and one pass over the logits; with ``cal`` given nothing is allocated and nothing synchronises.
    Returns cal (``evaluation.CalibrationTable`` reads it)."""
    what = "calibration"
    if kind not in _CAL_KINDS:
        raise ValueError(f"{what}: kind is 'top1' or 'margin', got {kind!r}")
    ids = None if groups is None else _group_ids(groups, n_groups)
    if groups is None and n_groups != 1:
        raise ValueError(f"{what}: groups=None needs n_groups == 1, got {n_groups}")
    _need_gpu(logits)
    if logits.dim() != 4 or not logits.is_contiguous():
        raise _lib.ArsegError(f"{what}: logits must be a contiguous fp32 [N,n_cls,h,w] tensor, got {tuple(logits.shape)} strides {logits.stride()}")
    N, n_cls, h, w = logits.shape
    H, W = int(H), int(W)
    dev = logits.device
    if not 1 <= n_cls <= 32:
        raise ValueError(f"{what}: 1..32 classes, got {n_cls}")
    if H < 1 or W < 1:
        raise ValueError(f"{what}: a positive output size, got {H}x{W}")
    _need_gpu(label, dtype=torch.int64)
    if tuple(label.shape) != (N, H, W) or not label.is_contiguous() or label.device != dev:
        raise _lib.ArsegError(f"{what}: label must be a contiguous int64 {(N, H, W)} tensor on {dev}, got {tuple(label.shape)} on {label.device}")
    grp = None if groups is None else _groups_tensor(groups, ids, N, dev)
    shape = (n_groups, n_cls, 256, 2)
    if cal is None:
        cal = torch.zeros(shape, dtype=torch.int64, device=dev)
    elif tuple(cal.shape) != shape or cal.dtype != torch.int64 or cal.device != dev or not cal.is_contiguous():
        raise _lib.ArsegError(f"{what}: cal must be a contiguous int64 GPU tensor {list(shape)}, got {cal.dtype} {tuple(cal.shape)}")
    launch(what, _lib.load().arseg_calibration_fwd, _ptr(logits), _ptr(label), _ptr(grp), _ptr(cal), N, n_groups, n_cls, h, w, H, W,
           int(ignore_label), 1 if align_corners else 0, _CAL_KINDS[kind], _stream(), nbytes=logits.numel() * 4 + N * H * W * 8)
    return cal
