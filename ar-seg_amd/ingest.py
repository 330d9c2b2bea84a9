"""Inputs of the hot path as the reference's datasets hold them on disk.

* motion vectors: ``.bin`` files of int16 quarter-pel ``[H,W,2]`` (dataset/camvid.py:624-626, dataset/cityscapes.py:282-285).
  The reference reads them with ``np.fromfile(..., np.short).reshape(H,W,2) / 4`` into float64 pixels and ships 16 B/pixel to
  the GPU; here the int16 array is uploaded as is (4 B/pixel) and consumed by ``ops.warp_mvq`` (MV resize + warp fused).
* decoded frames: uint8 HWC; ``ToTensor`` + ``Normalize`` (dataset/camvid.py:503-506) and the evaluator's downscale
  (evaluation.py:186-188) run in one kernel, ``ops.frame_u8_to_nhwc4``.
* decoder output as the fast paths take it: ``DecodedFrames`` (uint8 RGB, NV12 or I420 planes, 10-bit P010 or I010 planes + normalisation +
  colour matrix); every fast path that accepts float NCHW frames accepts one of these instead and ingests it with ``ops.frame_ingest8`` /
  ``ops.frame_ingest_yuv`` (csrc/ingest.hip).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

CAMVID_MEAN, CAMVID_STD = (0.39068785, 0.40521392, 0.41434407), (0.29652068, 0.30514979, 0.30080369)      # camvid.py:505
CITY_BISE_MEAN, CITY_BISE_STD = (0.3257, 0.3690, 0.3223), (0.2112, 0.2148, 0.2115)                          # cityscapes.py:211-212


def read_mv_bin(path, H: int, W: int) -> np.ndarray:
    """int16 quarter-pel motion vectors [H,W,2] (x, y) of one non-keyframe, accumulated back to its keyframe."""
    mv = np.fromfile(path, dtype=np.int16)
    if mv.size != H * W * 2:
        raise ValueError(f"{path}: expected {H * W * 2} int16 values for a {H}x{W} frame, found {mv.size}")
    return mv.reshape(H, W, 2)


def mv_to_device(mv_q: np.ndarray, device) -> torch.Tensor:
    """[H,W,2] or [N,H,W,2] int16 -> device tensor [N,H,W,2] (the layout ops.warp_mvq takes)."""
    t = torch.from_numpy(np.ascontiguousarray(mv_q, dtype=np.int16))
    return (t.unsqueeze(0) if t.dim() == 3 else t).to(device)


def frames_to_nhwc4(frames_u8, h: int, w: int, mean=CAMVID_MEAN, std=CAMVID_STD, device="cuda") -> torch.Tensor:
    """uint8 frames [H,W,3] / [N,H,W,3] (numpy or tensor) -> normalised NHWC4 [N,h,w,4] on the GPU."""
    t = torch.as_tensor(np.ascontiguousarray(frames_u8)) if not torch.is_tensor(frames_u8) else frames_u8
    if t.dim() == 3:
        t = t.unsqueeze(0)
    return ops.frame_u8_to_nhwc4(t.to(device), h, w, mean, std)


# ----------------------------------------------------------------------------------------------
# decoder frames for the fast paths
# ----------------------------------------------------------------------------------------------
# (Kr, Kb) of Y' = Kr R + Kg G + Kb B; include/arseg_hip.h (arseg_frame_ingest_fwd) writes the inverse matrices out
_LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
_COLOUR = {("bt601", False): _lib.COLOUR_BT601_LIMITED, ("bt601", True): _lib.COLOUR_BT601_FULL,
           ("bt709", False): _lib.COLOUR_BT709_LIMITED, ("bt709", True): _lib.COLOUR_BT709_FULL}


def colour_enum(matrix: str = "bt709", full_range: bool = False) -> int:
    """("bt601" | "bt709", full_range) -> enum arseg_colour."""
    try:
        return _COLOUR[(str(matrix).lower(), bool(full_range))]
    except KeyError:
        raise ValueError(f"matrix must be 'bt601' or 'bt709', got {matrix!r}") from None


def rgb_to_nv12(rgb_u8, matrix: str = "bt709", full_range: bool = False):
    """uint8 RGB [H,W,3] / [N,H,W,3] (numpy) -> (luma uint8 [..,H,W], chroma uint8 [..,H/2,W/2,2] = (Cb, Cr)), H and W even: what a decoder
    would hand over for these frames.  Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)); limited range
    Y = 16 + 219/255 Y', C = 128 + 224/255 C', full range Y = Y', C = 128 + C'; chroma is the 2x2 box average (the sample between two luma
    rows), everything rounded to nearest once.  For tests, tools and callers without a decoder; runs on the host."""
    colour_enum(matrix, full_range)
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim not in (3, 4) or rgb.shape[-1] != 3:
        raise ValueError(f"rgb_to_nv12 expects uint8 [H,W,3] or [N,H,W,3], got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[-3], rgb.shape[-2]
    if H % 2 or W % 2:
        raise ValueError(f"NV12 needs even H and W, got {H}x{W}")
    kr, kb = _LUMA[str(matrix).lower()]
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    yl = kr * r + (1.0 - kr - kb) * g + kb * b
    cb, cr = (b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr))
    sy, sc, y0 = (1.0, 1.0, 0.0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    box = lambda c: c.reshape(c.shape[:-2] + (H // 2, 2, W // 2, 2)).mean(axis=(-3, -1))
    q = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return q(y0 + sy * yl), np.stack([q(128.0 + sc * box(cb)), q(128.0 + sc * box(cr))], axis=-1)


_LAYOUTS = ("nv12", "i420", "p010", "i010")


def rgb_to_yuv420(rgb_u8, layout: str = "nv12", matrix: str = "bt709", full_range: bool = False):
    """uint8 RGB [H,W,3] / [N,H,W,3] (numpy) -> the planes of one 4:2:0 ``layout``, with ``rgb_to_nv12``'s fp64 arithmetic and 2x2 box chroma:
    "nv12" (Y uint8, (Cb, Cr) uint8 [..,H/2,W/2,2]) and "i420" (Y, Cb, Cr uint8) hold exactly ``rgb_to_nv12``'s samples; "i010" (Y, Cb, Cr
    uint16, code in the low 10 bits) and "p010" (Y, (Cb, Cr) uint16, code << 6) quantise ONCE to 10 bits -- limited range Y = 64 + 876/255 Y',
    C = 512 + 896/255 C', full range Y = 1023/255 Y', C = 512 + 1023/255 C' -- so the low bits carry picture.  For tests and tools."""
    layout = str(layout).lower()
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be one of {_LAYOUTS}, got {layout!r}")
    if layout in ("nv12", "i420"):
        y, uv = rgb_to_nv12(rgb_u8, matrix, full_range)
        return (y, uv) if layout == "nv12" else (y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]))
    colour_enum(matrix, full_range)
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim not in (3, 4) or rgb.shape[-1] != 3:
        raise ValueError(f"rgb_to_yuv420 expects uint8 [H,W,3] or [N,H,W,3], got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[-3], rgb.shape[-2]
    if H % 2 or W % 2:
        raise ValueError(f"4:2:0 needs even H and W, got {H}x{W}")
    kr, kb = _LUMA[str(matrix).lower()]
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    yl = kr * r + (1.0 - kr - kb) * g + kb * b
    cb, cr = (b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr))
    sy, sc, y0 = (1023.0 / 255.0, 1023.0 / 255.0, 0.0) if full_range else (876.0 / 255.0, 896.0 / 255.0, 64.0)
    box = lambda c: c.reshape(c.shape[:-2] + (H // 2, 2, W // 2, 2)).mean(axis=(-3, -1))
    q = lambda v: np.clip(np.rint(v), 0, 1023).astype(np.uint16)
    y, u, v = q(y0 + sy * yl), q(512.0 + sc * box(cb)), q(512.0 + sc * box(cr))
    return (y, u, v) if layout == "i010" else (y << 6, np.stack([u, v], axis=-1) << 6)


def _plane(t, what):
    t = torch.as_tensor(np.ascontiguousarray(t)) if not torch.is_tensor(t) else t
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: expected uint8, got {t.dtype}")
    return t


def _plane16(t, what):
    """16-bit samples: torch.uint16 or numpy uint16; torch.int16 is taken as the same bit pattern (a view, not a copy)."""
    t = torch.as_tensor(np.ascontiguousarray(t)) if not torch.is_tensor(t) else t
    if t.dtype == torch.int16:
        t = t.view(torch.uint16)
    if t.dtype != torch.uint16:
        raise ValueError(f"{what}: expected uint16 (or int16 holding the same bits), got {t.dtype}")
    return t


def _rows(t, inner):
    """Keep a view whose rows are contiguous (a pitch / an image stride is what the kernel takes); anything else is copied."""
    want, n = [], 1
    for d in reversed(inner):
        want.insert(0, n)
        n *= d
    return t if tuple(t.stride()[2:]) == tuple(want) and (t.shape[1] == 1 or t.stride(1) >= n) and (t.shape[0] == 1 or t.stride(0) >= 0) else t.contiguous()


def _bits(p):
    return p.view(torch.int16) if p.dtype == torch.uint16 else p          # (comparisons of uint16 tensors are not implemented everywhere)


class DecodedFrames(object):
    """A batch of frames as a decoder (NV12, I420; 10-bit P010, I010) or the datasets (RGB) hold them, with what the ingest kernel needs to turn them into the
    conv engine's input: source format, the plane tensor(s), ``H``, ``W``, ``mean``, ``std``, the colour enum.  Accepted wherever the fast
    paths take float NCHW frames (``evaluation.alter_res_*``, ``EvalAlterRes`` / ``EvalByDistance``, the models' ``forward_keyframe`` /
    ``forward``, ``gop.GopRunner``); ``shape`` answers ``(N, 3, H, W)`` like the float tensor it stands for."""

    def __init__(self, src_format, planes, mean, std, colour=_lib.COLOUR_BT709_LIMITED):
        self.src_format, self.planes, self.colour = src_format, tuple(planes), int(colour)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or any(v == 0.0 for v in self.std):
            raise ValueError(f"mean / std: three values each and no zero std, got {mean} / {std}")
        self.N, self.H, self.W = (int(v) for v in self.planes[0].shape[:3])

    @classmethod
    def rgb8(cls, frames, mean=CAMVID_MEAN, std=CAMVID_STD):
        """uint8 [H,W,3] / [N,H,W,3] (tensor or numpy), interleaved RGB; a view with a row pitch is taken as it is."""
        t = _plane(frames, "DecodedFrames.rgb8")
        t = t.unsqueeze(0) if t.dim() == 3 else t
        if t.dim() != 4 or t.shape[-1] != 3 or 0 in t.shape:
            raise ValueError(f"DecodedFrames.rgb8 expects uint8 [H,W,3] or [N,H,W,3], got {tuple(t.shape)}")
        return cls(_lib.SRC_RGB8, (_rows(t, (t.shape[2], 3)),), mean, std)

    @classmethod
    def nv12(cls, y, uv, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """luma uint8 [H,W] / [N,H,W] and chroma uint8 [H/2,W/2,2] / [N,H/2,W/2,2] (Cb, Cr interleaved), H and W even, both on one device."""
        colour = colour_enum(matrix, full_range)
        y, uv = _plane(y, "DecodedFrames.nv12 luma"), _plane(uv, "DecodedFrames.nv12 chroma")
        y, uv = (y.unsqueeze(0) if y.dim() == 2 else y), (uv.unsqueeze(0) if uv.dim() == 3 else uv)
        if y.dim() != 3 or uv.dim() != 4 or 0 in y.shape:
            raise ValueError(f"DecodedFrames.nv12 expects luma [N,H,W] and chroma [N,H/2,W/2,2], got {tuple(y.shape)} and {tuple(uv.shape)}")
        N, H, W = y.shape
        if H % 2 or W % 2:
            raise ValueError(f"NV12 needs even H and W, got {H}x{W}")
        if tuple(uv.shape) != (N, H // 2, W // 2, 2):
            raise ValueError(f"chroma plane of {N} frames {H}x{W} must be {(N, H // 2, W // 2, 2)}, got {tuple(uv.shape)}")
        if y.device != uv.device:
            raise ValueError(f"luma is on {y.device}, chroma on {uv.device}: both planes must be on one device")
        return cls(_lib.SRC_NV12, (_rows(y, (W,)), _rows(uv, (W // 2, 2))), mean, std, colour)

    @classmethod
    def _planar(cls, src_format, name, plane, y, u, v, mean, std, matrix, full_range):
        colour = colour_enum(matrix, full_range)
        y, u, v = plane(y, f"DecodedFrames.{name} luma"), plane(u, f"DecodedFrames.{name} Cb"), plane(v, f"DecodedFrames.{name} Cr")
        y, u, v = (t.unsqueeze(0) if t.dim() == 2 else t for t in (y, u, v))
        if y.dim() != 3 or u.dim() != 3 or v.dim() != 3 or 0 in y.shape:
            raise ValueError(f"DecodedFrames.{name} expects luma [N,H,W] and Cb, Cr [N,H/2,W/2], got {tuple(y.shape)}, {tuple(u.shape)} and {tuple(v.shape)}")
        N, H, W = y.shape
        if H % 2 or W % 2:
            raise ValueError(f"{name.upper()} needs even H and W, got {H}x{W}")
        for what, c in (("Cb", u), ("Cr", v)):
            if tuple(c.shape) != (N, H // 2, W // 2):
                raise ValueError(f"{what} plane of {N} frames {H}x{W} must be {(N, H // 2, W // 2)}, got {tuple(c.shape)}")
        if y.device != u.device or y.device != v.device:
            raise ValueError(f"luma is on {y.device}, Cb on {u.device}, Cr on {v.device}: all planes must be on one device")
        return cls(src_format, (_rows(y, (W,)), _rows(u, (W // 2,)), _rows(v, (W // 2,))), mean, std, colour)

    @classmethod
    def i420(cls, y, u, v, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """Planar 8-bit 4:2:0 (yuv420p, what a software HEVC decoder hands over): luma uint8 [H,W] / [N,H,W], Cb and Cr uint8 [H/2,W/2] /
        [N,H/2,W/2], H and W even, all on one device."""
        return cls._planar(_lib.SRC_I420, "i420", _plane, y, u, v, mean, std, matrix, full_range)

    @classmethod
    def i010(cls, y, u, v, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """Planar 10-bit 4:2:0 (yuv420p10le): the planes of ``i420`` as uint16 (torch.uint16, numpy uint16, or torch.int16 holding the same
        bits), the code in the low 10 bits; the high 6 bits are ignored."""
        return cls._planar(_lib.SRC_I010, "i010", _plane16, y, u, v, mean, std, matrix, full_range)

    @classmethod
    def p010(cls, y, uv, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """P010 (a hardware decoder's 10-bit output): luma uint16 [H,W] / [N,H,W] and chroma uint16 [H/2,W/2,2] / [N,H/2,W/2,2] (Cb, Cr
        interleaved), the code in the high 10 bits of each word; the low 6 bits are ignored.  uint16 as for ``i010``."""
        colour = colour_enum(matrix, full_range)
        y, uv = _plane16(y, "DecodedFrames.p010 luma"), _plane16(uv, "DecodedFrames.p010 chroma")
        y, uv = (y.unsqueeze(0) if y.dim() == 2 else y), (uv.unsqueeze(0) if uv.dim() == 3 else uv)
        if y.dim() != 3 or uv.dim() != 4 or 0 in y.shape:
            raise ValueError(f"DecodedFrames.p010 expects luma [N,H,W] and chroma [N,H/2,W/2,2], got {tuple(y.shape)} and {tuple(uv.shape)}")
        N, H, W = y.shape
        if H % 2 or W % 2:
            raise ValueError(f"P010 needs even H and W, got {H}x{W}")
        if tuple(uv.shape) != (N, H // 2, W // 2, 2):
            raise ValueError(f"chroma plane of {N} frames {H}x{W} must be {(N, H // 2, W // 2, 2)}, got {tuple(uv.shape)}")
        if y.device != uv.device:
            raise ValueError(f"luma is on {y.device}, chroma on {uv.device}: both planes must be on one device")
        return cls(_lib.SRC_P010, (_rows(y, (W,)), _rows(uv, (W // 2, 2))), mean, std, colour)

    # ---- what callers of the float tensor ask of it
    @property
    def shape(self):
        return (self.N, 3, self.H, self.W)

    @property
    def device(self):
        return self.planes[0].device

    @property
    def is_cuda(self):
        return self.planes[0].is_cuda

    def __len__(self):
        return self.N

    def _with(self, planes):
        return DecodedFrames(self.src_format, planes, self.mean, self.std, self.colour)

    def to(self, device, non_blocking=False):
        return self._with([p.to(device, non_blocking=non_blocking) for p in self.planes])

    def cuda(self, device=None, non_blocking=False):
        return self if self.is_cuda and device is None else self._with([p.cuda(device, non_blocking=non_blocking) for p in self.planes])

    def __getitem__(self, idx):
        """Frames along the batch axis: an int keeps the axis (one frame is a batch of one)."""
        if isinstance(idx, int):
            idx = slice(idx, idx + 1) if idx != -1 else slice(-1, None)
        if not isinstance(idx, slice):
            raise TypeError("DecodedFrames are indexed along the batch axis by an int or a slice")
        return self._with([p[idx] for p in self.planes])

    def equal(self, other):
        return (self.src_format, self.colour, self.mean, self.std, self.shape) == (other.src_format, other.colour, other.mean, other.std, other.shape) \
            and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(self.planes, other.planes))

    def to_input(self, h, w, dtype=torch.float32):
        """-> NHWC4 fp32 [N,h,w,4] or NHWC8 fp16 / bf16 [N,h,w,8] on the planes' (GPU) device: one kernel."""
        if self.src_format in (_lib.SRC_I420, _lib.SRC_P010, _lib.SRC_I010):
            return ops.frame_ingest_yuv(self.planes, self.src_format, h, w, self.mean, self.std, dtype, self.colour)
        return ops.frame_ingest8(self.planes[0], self.planes[1] if self.src_format == _lib.SRC_NV12 else None, self.src_format, h, w,
                                 self.mean, self.std, dtype, self.colour)
