"""Inputs of the hot path as the reference's datasets hold them on disk.

* motion vectors: ``.bin`` files of int16 quarter-pel ``[H,W,2]`` (dataset/camvid.py:624-626, dataset/cityscapes.py:282-285).
  The reference reads them with ``np.fromfile(..., np.short).reshape(H,W,2) / 4`` into float64 pixels and ships 16 B/pixel to
  the GPU; here the int16 array is uploaded as is (4 B/pixel) and consumed by ``ops.warp_mvq`` (MV resize + warp fused).
* decoded frames: uint8 HWC; ``ToTensor`` + ``Normalize`` (dataset/camvid.py:503-506) and the evaluator's downscale
  (evaluation.py:186-188) run in one kernel, ``ops.frame_u8_to_nhwc4``.
* decoder output as the fast paths take it: ``DecodedFrames`` (uint8 RGB, NV12 or I420 planes, 10-bit P010 or I010 planes + normalisation +
  colour matrix); every fast path that accepts float NCHW frames accepts one of these instead and ingests it with the one implementation
  behind ``ops.frame_ingest8`` / ``ops.frame_ingest_yuv`` (csrc/ingest.hip).
* decoder motion as a decoder holds it: block records ``int16 [n,8]`` per P-frame (x, y, w, h, mvx, mvy, ref, reserved; the contract is in
  include/arseg_hip.h, arseg_mv_records_*).  ``MotionChain`` rasterises and chains them to the keyframe frame by frame on the GPU
  (csrc/mv_records.hip) into the ``mv_qs`` tensor the fast paths read; ``mv_to_records`` / ``records_to_dense`` convert the reference's
  dense per-frame dumps to records and back on the host.  ``MotionChain(bidirectional=True)`` takes B-frames as well: two prediction lists
  per frame, forward references, frames in decode order (arseg_mv_records_bi_*); ``chain_records_numpy`` is that rule on the host,
  ``motion_vectors_to_records`` the mapping from ``AVMotionVector``-style arrays.
* no decoder motion at all (a hardware decoder's frames): ``MotionEstimator`` makes the records on the GPU by block matching of a frame's luma
  against the previous frame's (csrc/block_motion.hip; include/arseg_hip.h, arseg_block_motion_*); ``block_motion_numpy`` is that search on the host.
  ``MotionEstimator(levels=...)`` searches coarse to fine over a ``LumaPyramid`` and reaches past 32 pixels (csrc/block_motion_pyr.hip;
  arseg_luma_pyramid_*, arseg_block_motion_pyr_*; ``luma_pyramid_numpy`` and ``block_motion_pyr_numpy`` on the host).
  ``MotionEstimator(anchor_refine=...)`` checks every block's composed displacement against the keyframe and re-anchors it there
  (csrc/block_motion_anchor.hip; arseg_block_motion_anchor_fwd; ``block_motion_anchor_numpy`` on the host).
  ``MotionEstimator(split_refine=...)`` splits a 16 x 16 block that straddles two motions into 8 x 8 children with vectors of their own
  (csrc/block_motion_split.hip; arseg_block_motion_split_fwd; ``block_motion_split_numpy`` on the host).
* intra and uncovered pixels of any chain, whoever made its records: ``ChainHealer`` matches the flagged pixels of a pushed frame against the
  keyframe and rewrites ``merged`` / ``link`` in place (csrc/mv_chain_heal.hip; arseg_mv_chain_heal_fwd; ``mv_chain_heal_numpy`` on the host).
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


def _rgb_to_yuv(rgb_u8, who, what, bits, matrix, full_range):
    """The fp64 core of ``rgb_to_nv12`` / ``rgb_to_yuv420``: -> (Y [..,H,W], Cb, Cr [..,H/2,W/2]) codes of depth ``bits``, rounded to nearest once."""
    colour_enum(matrix, full_range)
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim not in (3, 4) or rgb.shape[-1] != 3:
        raise ValueError(f"{who} expects uint8 [H,W,3] or [N,H,W,3], got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[-3], rgb.shape[-2]
    if H % 2 or W % 2:
        raise ValueError(f"{what} needs even H and W, got {H}x{W}")
    kr, kb = _LUMA[str(matrix).lower()]
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    yl = kr * r + (1.0 - kr - kb) * g + kb * b
    cb, cr = (b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr))
    top, k = (1 << bits) - 1, 1 << (bits - 8)
    sy, sc, y0 = (top / 255.0, top / 255.0, 0.0) if full_range else (219.0 * k / 255.0, 224.0 * k / 255.0, 16.0 * k)
    box = lambda c: c.reshape(c.shape[:-2] + (H // 2, 2, W // 2, 2)).mean(axis=(-3, -1))
    q = lambda v: np.clip(np.rint(v), 0, top).astype(np.uint8 if bits == 8 else np.uint16)
    return q(y0 + sy * yl), q(128.0 * k + sc * box(cb)), q(128.0 * k + sc * box(cr))


def rgb_to_nv12(rgb_u8, matrix: str = "bt709", full_range: bool = False):
    """uint8 RGB [H,W,3] / [N,H,W,3] (numpy) -> (luma uint8 [..,H,W], chroma uint8 [..,H/2,W/2,2] = (Cb, Cr)), H and W even: what a decoder
    would hand over for these frames.  Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)); limited range
    Y = 16 + 219/255 Y', C = 128 + 224/255 C', full range Y = Y', C = 128 + C'; chroma is the 2x2 box average (the sample between two luma
    rows), everything rounded to nearest once.  For tests, tools and callers without a decoder; runs on the host."""
    y, u, v = _rgb_to_yuv(rgb_u8, "rgb_to_nv12", "NV12", 8, matrix, full_range)
    return y, np.stack([u, v], axis=-1)


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
        y, u, v = _rgb_to_yuv(rgb_u8, "rgb_to_nv12", "NV12", 8, matrix, full_range)
        return (y, np.stack([u, v], axis=-1)) if layout == "nv12" else (y, u, v)
    y, u, v = _rgb_to_yuv(rgb_u8, "rgb_to_yuv420", "4:2:0", 10, matrix, full_range)
    return (y, u, v) if layout == "i010" else (y << 6, np.stack([u, v], axis=-1) << 6)


def _plane(t, what, dtype=torch.uint8):
    """Samples as they are (a view, not a copy); where uint16 is wanted, torch.int16 is taken as the same bit pattern."""
    t = torch.as_tensor(np.ascontiguousarray(t)) if not torch.is_tensor(t) else t
    if dtype == torch.uint16 and t.dtype == torch.int16:
        t = t.view(torch.uint16)
    if t.dtype != dtype:
        raise ValueError(f"{what}: expected {'uint8' if dtype == torch.uint8 else 'uint16 (or int16 holding the same bits)'}, got {t.dtype}")
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
    def _semi_planar(cls, src_format, name, dtype, y, uv, mean, std, matrix, full_range):
        colour = colour_enum(matrix, full_range)
        y, uv = _plane(y, f"DecodedFrames.{name} luma", dtype), _plane(uv, f"DecodedFrames.{name} chroma", dtype)
        y, uv = (y.unsqueeze(0) if y.dim() == 2 else y), (uv.unsqueeze(0) if uv.dim() == 3 else uv)
        if y.dim() != 3 or uv.dim() != 4 or 0 in y.shape:
            raise ValueError(f"DecodedFrames.{name} expects luma [N,H,W] and chroma [N,H/2,W/2,2], got {tuple(y.shape)} and {tuple(uv.shape)}")
        N, H, W = y.shape
        if H % 2 or W % 2:
            raise ValueError(f"{name.upper()} needs even H and W, got {H}x{W}")
        if tuple(uv.shape) != (N, H // 2, W // 2, 2):
            raise ValueError(f"chroma plane of {N} frames {H}x{W} must be {(N, H // 2, W // 2, 2)}, got {tuple(uv.shape)}")
        if y.device != uv.device:
            raise ValueError(f"luma is on {y.device}, chroma on {uv.device}: both planes must be on one device")
        return cls(src_format, (_rows(y, (W,)), _rows(uv, (W // 2, 2))), mean, std, colour)

    @classmethod
    def nv12(cls, y, uv, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """luma uint8 [H,W] / [N,H,W] and chroma uint8 [H/2,W/2,2] / [N,H/2,W/2,2] (Cb, Cr interleaved), H and W even, both on one device."""
        return cls._semi_planar(_lib.SRC_NV12, "nv12", torch.uint8, y, uv, mean, std, matrix, full_range)

    @classmethod
    def _planar(cls, src_format, name, dtype, y, u, v, mean, std, matrix, full_range):
        colour = colour_enum(matrix, full_range)
        y, u, v = _plane(y, f"DecodedFrames.{name} luma", dtype), _plane(u, f"DecodedFrames.{name} Cb", dtype), _plane(v, f"DecodedFrames.{name} Cr", dtype)
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
        return cls._planar(_lib.SRC_I420, "i420", torch.uint8, y, u, v, mean, std, matrix, full_range)

    @classmethod
    def i010(cls, y, u, v, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """Planar 10-bit 4:2:0 (yuv420p10le): the planes of ``i420`` as uint16 (torch.uint16, numpy uint16, or torch.int16 holding the same
        bits), the code in the low 10 bits; the high 6 bits are ignored."""
        return cls._planar(_lib.SRC_I010, "i010", torch.uint16, y, u, v, mean, std, matrix, full_range)

    @classmethod
    def p010(cls, y, uv, mean=CAMVID_MEAN, std=CAMVID_STD, matrix="bt709", full_range=False):
        """P010 (a hardware decoder's 10-bit output): luma uint16 [H,W] / [N,H,W] and chroma uint16 [H/2,W/2,2] / [N,H/2,W/2,2] (Cb, Cr
        interleaved), the code in the high 10 bits of each word; the low 6 bits are ignored.  uint16 as for ``i010``."""
        return cls._semi_planar(_lib.SRC_P010, "p010", torch.uint16, y, uv, mean, std, matrix, full_range)

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
        return ops._frame_ingest_planes(self.planes, self.src_format, h, w, self.mean, self.std, dtype, self.colour)

    def luma_plane(self):
        """(plane, src_format): what block motion estimation reads of these frames (``ops.block_motion``, ``MotionEstimator``) -- plane 0, a
        view with its row pitch kept: the luma plane [N,H,W] of the 4:2:0 formats, the interleaved plane [N,H,W,3] of RGB8."""
        return self.planes[0], self.src_format


# ----------------------------------------------------------------------------------------------
# decoder motion: block records -> mv_q
# ----------------------------------------------------------------------------------------------
RECORD_FIELDS = ("x", "y", "w", "h", "mvx", "mvy", "ref", "reserved")          # one record: eight int16, 16 bytes


def mv_to_records(dense) -> np.ndarray:
    """A dense per-frame motion field int16 [H,W,3] = (mvx, mvy, ref), as the reference's decoder dumps it, -> block records int16 [n,8]:
    greedily the largest aligned squares (64, 32, ... 1 pixels, inside the frame) on which all three channels are constant, listed in raster
    order of their top-left corners.  The squares do not overlap and cover the frame, so ``records_to_dense`` gives ``dense`` back.  Host,
    numpy; for tests, tools and callers who hold the reference's dumps."""
    d = np.asarray(dense)
    if d.dtype != np.int16 or d.ndim != 3 or d.shape[2] != 3:
        raise ValueError(f"mv_to_records expects int16 [H,W,3], got {d.dtype} {d.shape}")
    H, W, _ = d.shape
    covered = np.zeros((H, W), dtype=bool)
    found = []
    s = 64
    while s >= 1:
        hb, wb = H // s, W // s
        if hb and wb:
            blk = d[:hb * s, :wb * s].reshape(hb, s, wb, s, 3)
            const = (blk.max(axis=(1, 3)) == blk.min(axis=(1, 3))).all(axis=-1)
            const &= ~covered[:hb * s, :wb * s].reshape(hb, s, wb, s).any(axis=(1, 3))
            by, bx = np.nonzero(const)
            if by.size:
                rec = np.zeros((by.size, 8), dtype=np.int16)
                rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = bx * s, by * s, s, s
                rec[:, 4:7] = d[by * s, bx * s]
                found.append(rec)
                covered[:hb * s, :wb * s] |= np.repeat(np.repeat(const, s, axis=0), s, axis=1)
        s //= 2
    rec = np.concatenate(found) if found else np.zeros((0, 8), dtype=np.int16)
    return np.ascontiguousarray(rec[np.lexsort((rec[:, 0], rec[:, 1]))])


def records_to_dense(records, H: int, W: int) -> np.ndarray:
    """Block records int16 [n,8] -> the dense field int16 [H,W,3] they rasterise to, by the rules of include/arseg_hip.h: records in index
    order, each assigned to its rectangle clipped to the frame (so the highest index wins an overlap), w <= 0 or h <= 0 covers nothing,
    uncovered pixels read (0, 0, -1).  The host restatement of ``ops.mv_records_rasterize``, for callers without a GPU at hand."""
    r = np.asarray(records)
    if r.dtype != np.int16 or r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"records_to_dense expects int16 [n,8], got {r.dtype} {r.shape}")
    out = np.zeros((H, W, 3), dtype=np.int16)
    out[..., 2] = -1
    for x, y, w, h, mvx, mvy, ref, _ in r.astype(np.int64):
        if w <= 0 or h <= 0:
            continue
        x0, x1, y0, y1 = max(x, 0), min(x + w, W), max(y, 0), min(y + h, H)
        if x0 < x1 and y0 < y1:
            out[y0:y1, x0:x1] = (mvx, mvy, ref)
    return out


def pad_records(records, capacity: int) -> np.ndarray:
    """int16 [n,8] -> int16 [capacity,8], the tail filled with zero records (w = h = 0: they cover nothing) -- the fixed-size buffer a
    captured graph reads."""
    r = np.asarray(records, dtype=np.int16)
    if r.ndim != 2 or r.shape[1] != 8 or r.shape[0] > capacity:
        raise ValueError(f"pad_records: {r.shape} does not fit a buffer of {capacity} records")
    out = np.zeros((capacity, 8), dtype=np.int16)
    out[:r.shape[0]] = r
    return out


def _as_int_array(v, name: str, n=None) -> np.ndarray:
    a = np.asarray(v)
    if a.dtype.kind not in "iu" and a.size:
        raise ValueError(f"motion_vectors_to_records: {name} must hold integers, got {a.dtype}")
    a = a.astype(np.int64)
    if n is not None:
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
            raise ValueError(f"motion_vectors_to_records: {name} must be a scalar or hold {n} values, got shape {a.shape}")
        a = np.broadcast_to(a, (n,))
    return a


def motion_vectors_to_records(dst_x, dst_y, w, h, motion_x, motion_y, motion_scale, offset, list_=0) -> np.ndarray:
    """Motion vectors as FFmpeg's ``AVMotionVector`` side data holds them (centre of the block in the current frame, block size, displacement
    to the reference in units of 1 / motion_scale pixel) -> block records int16 [n,8], integer arithmetic throughout:
    ``x = dst_x - w // 2``, ``y = dst_y - h // 2``, ``mvx = 4 * motion_x / motion_scale`` rounded half to even (likewise mvy).  ``offset`` is the
    signed display-order distance of the reference frame, negative = past: -k -> ``ref = k - 1``, +k -> ``ref = -k`` (the codes of
    arseg_mv_records_bi_*; a P-only stream has only negative offsets and gives the records ``MotionChain`` always took).  ``list_`` (0 or 1) goes
    into bit 0 of ``reserved``.  The first six arguments are integer arrays of one length n; motion_scale, offset and list_ are arrays of that
    length or scalars.  ValueError: offset == 0, motion_scale <= 0, list_ outside {0, 1}, any resulting field outside int16."""
    dst_x = _as_int_array(dst_x, "dst_x")
    if dst_x.ndim != 1:
        raise ValueError(f"motion_vectors_to_records: dst_x must be one-dimensional, got shape {dst_x.shape}")
    n = dst_x.shape[0]
    dst_y, w, h, motion_x, motion_y, motion_scale, offset, list_ = (_as_int_array(v, k, n) for k, v in (
        ("dst_y", dst_y), ("w", w), ("h", h), ("motion_x", motion_x), ("motion_y", motion_y), ("motion_scale", motion_scale), ("offset", offset),
        ("list_", list_)))
    if (offset == 0).any():
        raise ValueError("motion_vectors_to_records: offset 0 (a frame predicted from itself) has no record")
    if (motion_scale <= 0).any():
        raise ValueError("motion_vectors_to_records: motion_scale must be positive")
    if ((list_ != 0) & (list_ != 1)).any():
        raise ValueError("motion_vectors_to_records: list_ is 0 or 1")

    def quarter(m):                                                      # 4 m / scale, half to even
        q, r = np.divmod(4 * m, motion_scale)
        return q + ((2 * r > motion_scale) | ((2 * r == motion_scale) & (q & 1 == 1)))

    rec = np.stack([dst_x - w // 2, dst_y - h // 2, w, h, quarter(motion_x), quarter(motion_y), np.where(offset < 0, -offset - 1, -offset), list_], axis=1)
    if rec.size and (rec.min() < -32768 or rec.max() > 32767):
        raise ValueError("motion_vectors_to_records: a field does not fit int16")
    return np.ascontiguousarray(rec.astype(np.int16))


LINK_INTRA, LINK_UNCOVERED, LINK_CLAMPED = _lib.LINK_INTRA, _lib.LINK_UNCOVERED, _lib.LINK_CLAMPED       # flag bits of a link byte (ARSEG_LINK_*)


def link_hops(plane):
    """Link bytes (a tensor or an array of uint8) -> the number of links from each pixel to the keyframe, 0..15 (15 = 15 or more)."""
    return plane >> 4


BIPRED = ("list0", "near", "mean")          # what a pixel reads when both of its lists are usable: ARSEG_MVR_BI_LIST0 / _NEAR / _MEAN


def _round_half_even_div4(v):
    b, r = v >> 2, v & 3
    return b + ((r > 2) | ((r == 2) & (b & 1 == 1)))


def chain_records_numpy(pushes, H: int, W: int, gop: int, max_ref: int = 3, bipred: str = "list0", return_link: bool = False, after_push=None):
    """The two-list chain rule of include/arseg_hip.h (arseg_mv_records_bi_*) on the host, for callers without a GPU at hand: ``pushes`` is a
    list of ``(f, records int16 [n,8])`` in decode order; returns ``merged`` int16 [gop,H,W,2] with frame 0 = -1 and frames never pushed = 0.
    What ``MotionChain(bidirectional=True, bipred=bipred)`` leaves in ``merged`` after the same pushes.  ``return_link=True``: returns
    ``(merged, link)`` with ``link`` uint8 [gop,H,W], the link bytes of include/arseg_hip.h (arseg_mv_records_bi_step_link_fwd) -- what
    ``MotionChain(..., track_links=True)`` leaves in ``link``; frames never pushed = 0.  ``after_push``: called as ``after_push(f, merged_f int16
    [H,W,2], link_f uint8 [H,W])`` once frame f is composed; what it returns, ``(merged_f, link_f)``, replaces the frame in the chain's state
    before the next push reads it (``mv_chain_heal_numpy`` after every push is ``ChainHealer.heal`` after every ``MotionChain.push``)."""
    H, W, gop, max_ref = int(H), int(W), int(gop), int(max_ref)
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or not 2 <= gop <= 64 or not 1 <= max_ref <= 16 or bipred not in BIPRED:
        raise ValueError(f"chain_records_numpy: H, W in 1..8192, gop in 2..64, max_ref in 1..16, bipred in {BIPRED}; got {H}x{W}, gop {gop}, "
                         f"max_ref {max_ref}, bipred {bipred!r}")
    merged = np.zeros((gop, H, W, 2), dtype=np.int64)
    merged[0] = -1
    links = np.zeros((gop, H, W), dtype=np.int64)
    done = np.zeros(gop + 17, dtype=bool)                               # a forward target reaches at most f + 16
    done[0] = True
    ys, xs = np.mgrid[0:H, 0:W]
    for f, records in pushes:
        r = np.asarray(records)
        if r.dtype != np.int16 or r.ndim != 2 or r.shape[1] != 8:
            raise ValueError(f"chain_records_numpy expects records as int16 [n,8], got {r.dtype} {r.shape}")
        if not 1 <= f < gop or done[f]:
            raise ValueError(f"chain_records_numpy: frame {f} is outside [1, {gop}) or was pushed twice")
        r = r.astype(np.int64)
        winner = np.full((2, H, W), -1, dtype=np.int64)
        for i, (x, y, w, h) in enumerate(r[:, :4]):
            if w <= 0 or h <= 0:
                continue
            x0, x1, y0, y1 = max(x, 0), min(x + w, W), max(y, 0), min(y + h, H)
            if x0 < x1 and y0 < y1:
                winner[r[i, 7] & 1, y0:y1, x0:x1] = i
        usable, target, link, byte = [], [], [], []
        for l in (0, 1):
            q = r[np.maximum(winner[l], 0)] if r.shape[0] else np.zeros((H, W, 8), dtype=np.int64)
            ref = q[..., 6]
            t = np.where(ref >= 0, np.maximum(0, f - ref - 1), f - ref)
            ok = (winner[l] >= 0) & (ref >= -max_ref) & (ref < max_ref)
            t = np.where(ok, t, 0)
            k2 = np.clip(xs + _round_half_even_div4(q[..., 4]), 0, W - 1)
            j2 = np.clip(ys + _round_half_even_div4(q[..., 5]), 0, H - 1)
            d = 4 * np.stack([k2 - xs, j2 - ys], axis=-1)
            ok &= done[t]
            t = np.where(ok, t, 0)                                       # a target outside the GOP is never read
            usable.append(ok)
            target.append(t)
            link.append(d + np.where((t > 0)[..., None], merged[t, j2, k2], 0))
            clamped = (k2 != xs + _round_half_even_div4(q[..., 4])) | (j2 != ys + _round_half_even_div4(q[..., 5]))
            g = np.where(t > 0, links[t, j2, k2], 0)
            byte.append(((np.where(clamped, LINK_CLAMPED, 0) | g) & 7) | (np.minimum(15, 1 + (g >> 4)) << 4))
        p = int(np.nonzero(done[:f])[0].max())
        out = np.broadcast_to(merged[p] if p > 0 else 0, (H, W, 2)).copy()
        g = links[p] if p > 0 else np.zeros((H, W), dtype=np.int64)
        own = np.where((winner[0] >= 0) | (winner[1] >= 0), LINK_INTRA, LINK_UNCOVERED)
        lk = ((own | g) & 7) | (np.minimum(15, 1 + (g >> 4)) << 4)
        both = usable[0] & usable[1]
        if bipred == "near":
            first = ~both | (np.abs(target[0] - f) <= np.abs(target[1] - f))
        else:
            first = np.ones((H, W), dtype=bool)
        use0 = usable[0] & first
        use1 = usable[1] & ~use0
        out[use1] = link[1][use1]
        out[use0] = link[0][use0]
        lk[use1] = byte[1][use1]
        lk[use0] = byte[0][use0]
        if bipred == "mean":
            s = link[0] + link[1]
            m = s >> 1
            out[both] = (m + (s & 1 & m))[both]
            lk[both] = ((((byte[0] | byte[1]) & 7) | (np.maximum(byte[0] >> 4, byte[1] >> 4) << 4)))[both]
        merged[f] = out
        links[f] = lk
        if after_push is not None:
            merged[f], links[f] = after_push(f, merged[f].astype(np.int16), links[f].astype(np.uint8))
        done[f] = True
    assert merged.min() >= -32768 and merged.max() <= 32767
    return (merged.astype(np.int16), links.astype(np.uint8)) if return_link else merged.astype(np.int16)


class MotionChain(object):
    """The motion half of a decoder's output on the GPU: block records of one frame at a time -> ``mv_q``, the int16 quarter-pel field
    accumulated back to the keyframe (what mergeMotion writes into the datasets' .bin files).  Owns ``merged`` int16 [gop,H,W,2] and the
    int32 index map, both allocated once; ``push`` is two kernel launches and neither synchronises nor allocates, so a closure over a
    MotionChain and static (padded) record buffers can be captured in a HIP graph (``executor.GopGraph``).

        chain = MotionChain(H, W, gop=12)
        for each GOP:   chain.reset();  for each P-frame:  mv_q = chain.push(records)          # [H,W,2], a view of chain.merged[f]
        chain.mv_q()[1:]                       # [f,H,W,2]: the ``mv_qs`` of alter_res_batch_fast / alter_res_batch_pred / GopRunner

    H, W <= 8192; max_ref as mergeMotion's constant 3 (reference indices >= max_ref are intra), 1..16.

    ``bidirectional=False``: P-frames only, one record per block, pushed in display order (arseg_mv_records_*).  ``bidirectional=True``: streams
    with B-frames (arseg_mv_records_bi_*; gop <= 64, two index maps).  A record's ``reserved & 1`` is its prediction list, ``ref < 0`` points
    forward in display order, and frames are pushed in DECODE order with their display index: ``push(records, at=f)``.  A reference to a frame
    not pushed yet is unusable (the pixel falls to its other list, or to zero motion from the nearest pushed frame before it); ``bipred`` =
    "list0" | "near" | "mean" decides a pixel both of whose lists are usable.  P-only records pushed in order give the same ``merged`` either way.

        chain = MotionChain(H, W, gop=8, bidirectional=True, bipred="near")
        chain.reset();  for f, records in decode_order:  chain.push(records, at=f)
        chain.mv_q()[1:]                       # once frames 1..k are all in

    ``track_links=True``: the chain also owns ``link_bytes`` uint8 [gop,H,W] and ``link_counts`` int64 [gop, LINK_NSTATS] and ``push`` goes
    through the link entry points (arseg_mv_records_*_link_fwd: the same launches, ``merged`` bit-equal).  ``link()`` is the [k+1,H,W] view
    under ``mv_q()``'s prefix rule: per pixel LINK_INTRA / LINK_UNCOVERED / LINK_CLAMPED if that happened at this hop or at any hop towards
    the keyframe, and ``link_hops``; ``link_stats()`` the per-frame counts [intra, uncovered, clamped, any flag, 16 hop bins] -- rows for a
    ``LinkMonitor``, planes for ``egress.consistency_of_planes(..., link=)``.  With ``False`` allocations and entry points are as before.
    """

    def __init__(self, H: int, W: int, gop: int = 12, max_ref: int = 3, device="cuda", bidirectional: bool = False, bipred: str = "list0",
                 track_links: bool = False):
        H, W, gop, max_ref = int(H), int(W), int(gop), int(max_ref)
        if not (1 <= H <= 8192 and 1 <= W <= 8192) or gop < 2 or not 1 <= max_ref <= 16:
            raise _lib.ArsegError(f"MotionChain: H, W in 1..8192, gop >= 2, max_ref in 1..16; got {H}x{W}, gop {gop}, max_ref {max_ref}")
        if bipred not in BIPRED:
            raise _lib.ArsegError(f"MotionChain: bipred is one of {BIPRED}, got {bipred!r}")
        if bidirectional and gop > 64:
            raise _lib.ArsegError(f"MotionChain: a bidirectional chain holds at most 64 frames (the done set is one 64-bit mask), got gop {gop}")
        self.H, self.W, self.gop, self.max_ref = H, W, gop, max_ref
        self.bidirectional, self.bipred = bool(bidirectional), bipred
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ArsegError("MotionChain runs on the GPU only; there is no CPU fallback (records_to_dense is the host restatement)")
        self.merged = torch.empty((gop, H, W, 2), dtype=torch.int16, device=self.device)
        self.index_map = torch.empty((2 if self.bidirectional else 1) * H * W, dtype=torch.int32, device=self.device)
        self.track_links = bool(track_links)
        self.link_bytes = torch.empty((gop, H, W), dtype=torch.uint8, device=self.device) if self.track_links else None
        self.link_counts = torch.empty((gop, _lib.LINK_NSTATS), dtype=torch.int64, device=self.device) if self.track_links else None
        self.f = 0                      # in-order chain: the last frame pushed
        self.done_mask = 1              # bidirectional chain: bit g = frame g is chained
        self.last = 0                   # either chain: the display index of the last frame pushed (0: none yet)
        self.reset()

    def reset(self) -> None:
        """Starts a GOP: frame 0 of ``merged`` = -1 (as ``ops.merge_motion`` leaves it), index map(s) clean, no frame pushed."""
        if self.bidirectional:
            ops.mv_records_bi_reset(self.merged, self.index_map)
        else:
            ops.mv_records_reset(self.merged, self.index_map)
        if self.track_links:
            ops.mv_link_reset(self.link_bytes, self.link_counts)
        self.f, self.done_mask, self.last = 0, 1, 0

    def _records(self, records) -> torch.Tensor:
        if not torch.is_tensor(records):                      # host records: uploaded here (allocates; a graph wants device buffers)
            r = np.ascontiguousarray(records)
            if r.dtype != np.int16 or r.ndim != 2 or r.shape[1] != 8:
                raise _lib.ArsegError(f"MotionChain: records must be int16 [n,8], got {r.dtype} {r.shape}")
            records = torch.from_numpy(r).to(self.device)
        return records

    def frames_done(self) -> tuple:
        """The display indices chained so far in this GOP, sorted, the keyframe 0 included."""
        if not self.bidirectional:
            return tuple(range(self.f + 1))
        return tuple(g for g in range(self.gop) if (self.done_mask >> g) & 1)

    def push(self, records, at=None) -> torch.Tensor:
        """One frame's records (int16 [n,8] on the chain's device; n is the buffer's capacity, zero records are padding) -> its mv_q int16
        [H,W,2], the view ``merged[at]``.  ``at`` is the frame's display index in [1, gop); None = the lowest index not pushed yet (the next
        frame of an in-order stream).  An in-order chain takes only that one.  Raises for an index outside the GOP or pushed before."""
        if not self.bidirectional:
            if self.f >= self.gop - 1:
                raise _lib.ArsegError(f"MotionChain: the GOP holds {self.gop - 1} P-frames and all were pushed; reset() starts the next one")
            if at is not None and int(at) != self.f + 1:
                raise _lib.ArsegError(f"MotionChain: an in-order chain takes frame {self.f + 1} next, not {at}; bidirectional=True takes decode order")
            if self.track_links:
                out, _ = ops.mv_records_step_link(self._records(records), self.merged, self.f + 1, self.index_map, self.link_bytes, self.link_counts,
                                                  self.max_ref)
            else:
                out = ops.mv_records_step(self._records(records), self.merged, self.f + 1, self.index_map, self.max_ref)
            self.f += 1
            self.last = self.f
            return out
        if at is None:
            at = next((g for g in range(1, self.gop) if not (self.done_mask >> g) & 1), self.gop)
        at = int(at)
        if not 1 <= at < self.gop:
            raise _lib.ArsegError(f"MotionChain: frame {at} is outside [1, {self.gop}) (or every frame of the GOP was pushed); reset() starts the next GOP")
        if (self.done_mask >> at) & 1:
            raise _lib.ArsegError(f"MotionChain: frame {at} was pushed before in this GOP")
        if self.track_links:
            out, _ = ops.mv_records_bi_step_link(self._records(records), self.merged, at, self.done_mask, self.index_map, self.link_bytes,
                                                 self.link_counts, self.max_ref, self.bipred)
        else:
            out = ops.mv_records_bi_step(self._records(records), self.merged, at, self.done_mask, self.index_map, self.max_ref, self.bipred)
        self.done_mask |= 1 << at
        self.last = at
        return out

    def push_gop(self, list_of_records, order=None) -> torch.Tensor:
        """reset() + one push per entry; ``order`` = the display index of each entry (decode order; None: 1, 2, ...).  Returns ``mv_q()``."""
        list_of_records = list(list_of_records)
        if order is not None and len(order) != len(list_of_records):
            raise _lib.ArsegError(f"MotionChain: {len(list_of_records)} record lists but {len(order)} display indices")
        self.reset()
        for i, r in enumerate(list_of_records):
            self.push(r, None if order is None else order[i])
        return self.mv_q()

    def mv_q(self) -> torch.Tensor:
        """int16 [k+1,H,W,2], a view: frame 0 = -1 (the keyframe has no motion field), frames 1..k as pushed.  A bidirectional chain raises
        while the frames pushed are not 1..k without a gap (``merged[g]`` of a frame not pushed is not motion); a complete GOP never is."""
        return self.merged[:self._prefix("mv_q()") + 1]

    def _prefix(self, what) -> int:
        if not self.bidirectional:
            return self.f
        k = bin(self.done_mask).count("1") - 1
        if self.done_mask != (1 << (k + 1)) - 1:
            raise _lib.ArsegError(f"MotionChain: frames {self.frames_done()} are chained, which is not 0..{k} without a gap; {what} is whole prefixes only")
        return k

    def link(self) -> torch.Tensor:
        """uint8 [k+1,H,W], a view: the link bytes of frames 0..k (frame 0 all zero), under ``mv_q()``'s prefix rule.  ``track_links=True`` only."""
        if not self.track_links:
            raise _lib.ArsegError("MotionChain: link() needs track_links=True")
        return self.link_bytes[:self._prefix("link()") + 1]

    def link_stats(self) -> torch.Tensor:
        """int64 [gop, LINK_NSTATS]: row f = the counts of frame f as pushed in this GOP (rows of frames not pushed are zero).
        ``track_links=True`` only."""
        if not self.track_links:
            raise _lib.ArsegError("MotionChain: link_stats() needs track_links=True")
        return self.link_counts


class LinkMonitor(object):
    """Reports when too much of a frame has lost its link to the keyframe: an intra block or an uncovered pixel somewhere along its chain
    means the encoder found no prediction there (occlusion, new content, a scene cut -- inside a GOP every block is intra), the cleanest
    re-key signal a compressed stream offers, and it is there before any mask disagrees.  Pure Python on rows of
    ``MotionChain.link_stats()``, in the style of ``egress.DriftMonitor``; it only reports.

    ``max_unlinked``: report when the flagged share of the frame exceeds it (0 <= max_unlinked <= 1).  Required: no value is right for every
    encoder and content; it is the caller's to calibrate on its own streams.
    ``mask``: the flags that count.  The row counts each flag and "any flag", not every union, so the share is exact for a single flag and
    for all three (column 3); for two flags the row gives only bounds and the monitor takes the LOWER one, max(count_a, count_b) <= union:
    it never reports a frame the exact union would not.  A caller that needs the exact union of two flags counts it on the plane:
    ``(chain.link()[f] & mask != 0).sum()``, and passes it as ``flagged``."""

    def __init__(self, max_unlinked, mask=LINK_INTRA | LINK_UNCOVERED):
        self.max_unlinked, self.mask = float(max_unlinked), int(mask)
        if not 0.0 <= self.max_unlinked <= 1.0 or not 0 < self.mask <= 7:
            raise ValueError(f"LinkMonitor: max_unlinked in [0, 1] and a mask of LINK_* flags, got {max_unlinked!r}, {mask!r}")

    def flagged(self, stats_row) -> int:
        """The number of flagged pixels the row vouches for (see ``mask``)."""
        if self.mask == 7:
            return int(stats_row[3])
        return max(int(stats_row[b]) for b in range(3) if (self.mask >> b) & 1)

    def update(self, stats_row, n_pixels, flagged=None) -> bool:
        """One frame: ``stats_row`` its row of ``link_stats()``, ``n_pixels`` = H x W; ``flagged`` overrides the count taken from the row.
        True = refresh the keyframe."""
        n_pixels = int(n_pixels)
        if n_pixels <= 0:
            raise ValueError(f"LinkMonitor.update: n_pixels must be positive, got {n_pixels}")
        n = self.flagged(stats_row) if flagged is None else int(flagged)
        return bool(n / n_pixels > self.max_unlinked)


# ----------------------------------------------------------------------------------------------
# frames without motion vectors: block motion estimation -> records
# ----------------------------------------------------------------------------------------------
BM_INTRA_REF, BM_NSTATS = _lib.BM_INTRA_REF, _lib.BM_NSTATS          # ARSEG_BM_*: the ref of an estimated intra block; the length of the stats row


def luma8_numpy(plane, src_format: int = _lib.SRC_NV12) -> np.ndarray:
    """The 8-bit luma the block search compares (include/arseg_hip.h, arseg_block_motion_fwd), uint8 [H,W]: the byte of an NV12 / I420 luma
    plane, ``(v & 0x3ff) >> 2`` of I010 words, ``v >> 8`` of P010 words, ``(77 R + 150 G + 29 B + 128) >> 8`` of an RGB8 plane [H,W,3].  A
    leading batch axis of one is dropped; tensors are taken through numpy; int16 stands for the same 16 bits."""
    p = plane.cpu() if torch.is_tensor(plane) else plane
    if torch.is_tensor(p):
        p = (p.view(torch.int16) if p.dtype == torch.uint16 else p).numpy()
    p = np.asarray(p)
    rgb = src_format == _lib.SRC_RGB8
    if p.ndim == (4 if rgb else 3) and p.shape[0] == 1:
        p = p[0]
    wide = src_format in (_lib.SRC_P010, _lib.SRC_I010)
    if src_format not in (_lib.SRC_RGB8, _lib.SRC_NV12, _lib.SRC_I420, _lib.SRC_P010, _lib.SRC_I010):
        raise ValueError(f"luma8_numpy: unknown source format {src_format!r}")
    if p.ndim != (3 if rgb else 2) or (rgb and p.shape[2] != 3) or 0 in p.shape or p.dtype not in ((np.uint16, np.int16) if wide else (np.uint8,)):
        raise ValueError(f"luma8_numpy: format {src_format} expects {'uint16' if wide else 'uint8'} [H,W{',3' if rgb else ''}], got {p.dtype} {p.shape}")
    if rgb:
        c = p.astype(np.int64)
        return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)
    if not wide:
        return np.ascontiguousarray(p)
    v = p.view(np.uint16).astype(np.int64)
    return ((v >> 8) if src_format == _lib.SRC_P010 else ((v & 0x3ff) >> 2)).astype(np.uint8)


def _bm_args(who, H, W, B, R, lam, intra, ref_index):
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or B not in (8, 16) or not 1 <= R <= 32 or not 0 <= lam <= 255 or not 0 <= intra <= 255 \
            or not 0 <= ref_index <= 15:
        raise ValueError(f"{who}: H, W in 1..8192, block in (8, 16), search in 1..32, lam and intra in 0..255, ref_index in 0..15; got {H}x{W}, "
                         f"block {B}, search {R}, lam {lam}, intra {intra}, ref_index {ref_index}")


def _bm_outputs(dx, dy, sad, H, W, B, intra, ref_index):
    """The winners int64 [by,bx] of a block search as ``(records, sad, stats)``: a block whose SAD exceeds ``intra`` per pixel is written intra."""
    by, bx = dx.shape
    x0, y0 = np.arange(bx) * B, np.arange(by) * B
    w, h = np.minimum(B, W - x0), np.minimum(B, H - y0)
    is_intra = sad > intra * (h[:, None] * w[None, :])
    rec = np.zeros((by, bx, 8), dtype=np.int64)
    rec[..., 0], rec[..., 1], rec[..., 2], rec[..., 3] = x0[None, :], y0[:, None], w[None, :], h[:, None]
    rec[..., 4], rec[..., 5], rec[..., 6] = np.where(is_intra, 0, 4 * dx), np.where(is_intra, 0, 4 * dy), np.where(is_intra, BM_INTRA_REF, ref_index)
    m = ~is_intra
    stats = np.array([is_intra.sum(), (m & (dx == 0) & (dy == 0)).sum(), sad[m].sum(), (h[:, None] * w[None, :])[m].sum()], dtype=np.int64)
    return np.ascontiguousarray(rec.reshape(-1, 8).astype(np.int16)), sad.reshape(-1).astype(np.uint32), stats


def block_motion_numpy(cur, ref, B: int = 16, R: int = 16, lam: int = 2, intra: int = 255, ref_index: int = 0, src_format: int = _lib.SRC_NV12):
    """The block search of include/arseg_hip.h (arseg_block_motion_fwd) on the host, for callers without a GPU at hand: ``cur`` / ``ref`` are
    the planes ``luma8_numpy`` takes for ``src_format``.  Returns ``(records int16 [by*bx,8], sad uint32 [by*bx], stats int64 [BM_NSTATS])`` --
    what ``ops.block_motion`` writes, stats from zero.  numpy only, one pass over the frame per candidate (a 360 x 480 frame at R = 16 takes
    a couple of seconds)."""
    a, b = luma8_numpy(cur, src_format).astype(np.int32), luma8_numpy(ref, src_format).astype(np.int32)
    B, R, lam, intra, ref_index = int(B), int(R), int(lam), int(intra), int(ref_index)
    H, W = a.shape
    if b.shape != a.shape:
        raise ValueError(f"block_motion_numpy: the current frame is {a.shape}, the reference {b.shape}")
    _bm_args("block_motion_numpy", H, W, B, R, lam, intra, ref_index)
    by, bx, side = -(-H // B), -(-W // B), 2 * R + 1
    x0, y0 = np.arange(bx) * B, np.arange(by) * B
    w, h = np.minimum(B, W - x0), np.minimum(B, H - y0)
    diff = np.zeros((by * B, bx * B), dtype=np.int32)                   # what lies beyond the frame stays 0
    best = np.full((by, bx), (1 << 32) - 1, dtype=np.int64)
    for dy in range(-R, R + 1):
        oky = (y0 + dy >= 0) & (y0 + h + dy <= H)
        ya, yb = max(0, -dy), min(H, H - dy)
        if not oky.any():
            continue
        for dx in range(-R, R + 1):
            okx = (x0 + dx >= 0) & (x0 + w + dx <= W)
            xa, xb = max(0, -dx), min(W, W - dx)
            if not okx.any():
                continue
            # every pixel of a block that counts is inside [ya, yb) x [xa, xb); what an earlier candidate left elsewhere is in no such block
            diff[ya:yb, xa:xb] = np.abs(a[ya:yb, xa:xb] - b[ya + dy:yb + dy, xa + dx:xb + dx])
            sad = diff.reshape(by, B, bx, B).sum(axis=(1, 3), dtype=np.int64)
            rank = 0 if dx == 0 and dy == 0 else 1 + (dy + R) * side + (dx + R)
            key = ((sad + lam * (abs(dx) + abs(dy))) << 13) | rank
            best = np.where(oky[:, None] & okx[None, :], np.minimum(best, key), best)
    rank, cost = best & 0x1fff, best >> 13
    dy = np.where(rank > 0, (rank - 1) // side - R, 0)
    dx = np.where(rank > 0, (rank - 1) % side - R, 0)
    return _bm_outputs(dx, dy, cost - lam * (np.abs(dx) + np.abs(dy)), H, W, B, intra, ref_index)


def luma_pyramid_layout(H: int, W: int, levels: int):
    """``([(offset, pitch, H_l, W_l) for l in 0 .. levels], total bytes)`` of a luma pyramid buffer (include/arseg_hip.h, arseg_luma_pyramid_*):
    H_{l+1} = (H_l + 1) >> 1, rows (W_l + 15) & ~15 bytes apart, the levels back to back."""
    H, W, levels = int(H), int(W), int(levels)
    if not (1 <= H <= 8192 and 1 <= W <= 8192 and 1 <= levels <= 3):
        raise ValueError(f"luma_pyramid_layout: H, W in 1..8192 and levels in 1..3; got {H}x{W}, levels {levels}")
    out, off = [], 0
    for _ in range(levels + 1):
        pitch = (W + 15) & ~15
        out.append((off, pitch, H, W))
        off, H, W = off + pitch * H, (H + 1) >> 1, (W + 1) >> 1
    return out, off


def luma_pyramid_numpy(plane, src_format: int = _lib.SRC_NV12, levels: int = 1) -> list:
    """The luma pyramid of include/arseg_hip.h (arseg_luma_pyramid_fwd) on the host: ``[P_0, .. P_levels]``, uint8 [H_l,W_l] each, P_0 =
    ``luma8_numpy(plane, src_format)``, every further level the rounded 2 x 2 mean with the last row / column replicated for odd sizes."""
    out = [luma8_numpy(plane, src_format)]
    luma_pyramid_layout(out[0].shape[0], out[0].shape[1], levels)
    for _ in range(int(levels)):
        a = out[-1].astype(np.int32)
        H, W = a.shape
        e = a[np.minimum(np.arange(2 * ((H + 1) >> 1)), H - 1)][:, np.minimum(np.arange(2 * ((W + 1) >> 1)), W - 1)]
        out.append(((e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


def _bm_best_key(a, b, B, r, centres, key_of):
    """The smallest ``key_of(sad, dx, dy)`` per block of plane ``a`` int32 [H,W] over the candidates +-``r`` around every centre ``(cx, cy, ok)``
    (int64, int64, bool [by,bx]; a centre counts where ok) that leave the block inside plane ``b``; int64 [by,bx], 1 << 62 where there is none.
    One gather of ``b`` per (centre, offset): every block reads at its own displacement, and what a clipped block lacks counts in neither
    operand."""
    H, W = a.shape
    by, bx = -(-H // B), -(-W // B)
    x0, y0 = (np.arange(bx) * B)[None, :], (np.arange(by) * B)[:, None]
    w, h = np.minimum(B, W - x0), np.minimum(B, H - y0)
    ap = np.zeros((by * B, bx * B), dtype=np.int32)
    ap[:H, :W] = a
    Y, X = np.arange(by * B)[:, None], np.arange(bx * B)[None, :]
    inside = (Y < H) & (X < W)
    best = np.full((by, bx), (1 << 62), dtype=np.int64)
    for cx, cy, ok in centres:
        for oy in range(-r, r + 1):
            for ox in range(-r, r + 1):
                dx, dy = cx + ox, cy + oy
                valid = ok & (x0 + dx >= 0) & (x0 + w + dx <= W) & (y0 + dy >= 0) & (y0 + h + dy <= H)
                if not valid.any():
                    continue
                yy = np.clip(Y + np.repeat(np.repeat(dy, B, axis=0), B, axis=1), 0, H - 1)
                xx = np.clip(X + np.repeat(np.repeat(dx, B, axis=0), B, axis=1), 0, W - 1)
                sad = (np.abs(ap - b[yy, xx]) * inside).reshape(by, B, bx, B).sum(axis=(1, 3), dtype=np.int64)
                key = key_of(sad, dx, dy)
                best = np.where(valid & (key < best), key, best)
    return best


def _refine_numpy(a, b, pvx, pvy, B, r, lam):
    """One refinement level: the planes int32 [H_l,W_l], the parents' vectors int64 [by_{l+1},bx_{l+1}] -> (dx, dy, sad) int64 [by_l,bx_l]."""
    H, W = a.shape
    by, bx = -(-H // B), -(-W // B)
    pby, pbx = pvx.shape
    bi, bj = np.arange(by), np.arange(bx)
    pi, pj = bi >> 1, bj >> 1
    ni, nj = pi + np.where(bi & 1, 1, -1), pj + np.where(bj & 1, 1, -1)
    oki, okj = (ni >= 0) & (ni < pby), (nj >= 0) & (nj < pbx)
    ni, nj = np.clip(ni, 0, pby - 1), np.clip(nj, 0, pbx - 1)
    yes = np.ones((by, bx), dtype=bool)
    centres = [(np.zeros((by, bx), np.int64), np.zeros((by, bx), np.int64), yes),
               (2 * pvx[pi][:, pj], 2 * pvy[pi][:, pj], yes),
               (2 * pvx[pi][:, nj], 2 * pvy[pi][:, nj], yes & okj[None, :]),
               (2 * pvx[ni][:, pj], 2 * pvy[ni][:, pj], yes & oki[:, None])]

    def key_of(sad, dx, dy):
        return ((sad + lam * (np.abs(dx) + np.abs(dy))) << 20) | np.where((dx == 0) & (dy == 0), 0, 1 + (dy + 511) * 1023 + (dx + 511))

    best = _bm_best_key(a, b, B, r, centres, key_of)
    rank, cost = best & 0xfffff, best >> 20
    dy = np.where(rank > 0, (rank - 1) // 1023 - 511, 0)
    dx = np.where(rank > 0, (rank - 1) % 1023 - 511, 0)
    return dx, dy, cost - lam * (np.abs(dx) + np.abs(dy))


def _bmp_args(who, levels, r):
    if not 0 <= levels <= 3 or (levels and not 1 <= r <= 3):
        raise ValueError(f"{who}: levels in 0..3 and refine in 1..3; got levels {levels}, refine {r}")


def block_motion_pyr_numpy(cur, ref, B: int = 16, Rt: int = 8, r: int = 1, lam: int = 2, intra: int = 255, ref_index: int = 0, levels: int = 2,
                           src_format: int = _lib.SRC_NV12):
    """The hierarchical block search of include/arseg_hip.h (arseg_block_motion_pyr_fwd) on the host: ``block_motion_numpy`` with |dx|, |dy| <=
    ``Rt`` on level ``levels`` of the two ``luma_pyramid_numpy``, then per level below it the candidates +-``r`` around (0, 0) and around twice
    the vectors of the parent block and of its neighbours on the block's side.  Returns what ``block_motion_numpy`` returns; ``levels=0`` IS
    ``block_motion_numpy`` with R = ``Rt``.  numpy only, one gather of the frame per centre and offset (360 x 480 at r = 1: about a second)."""
    B, Rt, r, lam, intra, ref_index, levels = int(B), int(Rt), int(r), int(lam), int(intra), int(ref_index), int(levels)
    _bmp_args("block_motion_pyr_numpy", levels, r)
    if levels == 0:
        return block_motion_numpy(cur, ref, B, Rt, lam, intra, ref_index, src_format)
    pc, pr = luma_pyramid_numpy(cur, src_format, levels), luma_pyramid_numpy(ref, src_format, levels)
    H, W = pc[0].shape
    if pr[0].shape != pc[0].shape:
        raise ValueError(f"block_motion_pyr_numpy: the current frame is {pc[0].shape}, the reference {pr[0].shape}")
    _bm_args("block_motion_pyr_numpy", H, W, B, Rt, lam, intra, ref_index)
    top = block_motion_numpy(pc[levels], pr[levels], B, Rt, lam, 255, 0)[0].astype(np.int64)
    shape = (-(-pc[levels].shape[0] // B), -(-pc[levels].shape[1] // B))
    dx, dy = (top[:, 4] // 4).reshape(shape), (top[:, 5] // 4).reshape(shape)
    for l in range(levels - 1, -1, -1):
        dx, dy, sad = _refine_numpy(pc[l].astype(np.int32), pr[l].astype(np.int32), dx, dy, B, r, lam)
    return _bm_outputs(dx, dy, sad, H, W, B, intra, ref_index)


BMA_NSTATS = _lib.BMA_NSTATS          # ARSEG_BMA_NSTATS: anchored blocks, healed blocks, blocks kept on their hop, drift corrected in pixels


def block_motion_anchor_numpy(cur, key, records, merged_prev, f: int, B: int = 16, r: int = 2, lam: int = 2, intra: int = 255):
    """Keyframe anchoring of include/arseg_hip.h (arseg_block_motion_anchor_fwd) on the host: ``cur`` / ``key`` are uint8 luma planes [H,W] of
    frame ``f`` and of the keyframe, ``records`` the hop records int16 [by*bx,8] of the B-grid (``block_motion_numpy``), ``merged_prev`` =
    merged[f - 1] int16 [H,W,2] of the chain (None at f = 1).  Returns ``(records int16 [by*bx,8], sad_of_anchored int64 [by*bx], stats int64
    [BMA_NSTATS])``: the records ``ops.block_motion_anchor`` writes, the anchored SAD of every anchored block and -1 for a block kept on its
    hop (the entries the device form leaves untouched), stats from zero.  numpy only, one gather of the keyframe per centre and offset."""
    a, k = luma8_numpy(cur).astype(np.int32), luma8_numpy(key).astype(np.int32)
    f, B, r, lam, intra = int(f), int(B), int(r), int(lam), int(intra)
    H, W = a.shape
    if k.shape != a.shape:
        raise ValueError(f"block_motion_anchor_numpy: the current frame is {a.shape}, the keyframe {k.shape}")
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or B not in (8, 16) or not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 or not 1 <= f <= 16:
        raise ValueError(f"block_motion_anchor_numpy: H, W in 1..8192, B in (8, 16), r in 1..3, lam and intra in 0..255, f in 1..16; got {H}x{W}, B {B}, "
                         f"r {r}, lam {lam}, intra {intra}, f {f}")
    by, bx = -(-H // B), -(-W // B)
    rec = np.asarray(records)
    if rec.dtype != np.int16 or rec.shape != (by * bx, 8):
        raise ValueError(f"block_motion_anchor_numpy: {H}x{W} in blocks of {B} is int16 [{by * bx},8] records, got {rec.dtype} {rec.shape}")
    if f == 1:
        return rec.copy(), np.full(by * bx, -1, dtype=np.int64), np.zeros(BMA_NSTATS, dtype=np.int64)
    mp = np.asarray(merged_prev)
    if mp.dtype != np.int16 or mp.shape != (H, W, 2):
        raise ValueError(f"block_motion_anchor_numpy: merged_prev is int16 [{H},{W},2], got {mp.dtype} {mp.shape}")
    mp = mp.astype(np.int64)
    x0, y0 = np.arange(bx) * B, np.arange(by) * B
    w, h = np.minimum(B, W - x0), np.minimum(B, H - y0)
    xc, yc = (x0 + w // 2)[None, :], (y0 + h // 2)[:, None]
    q = rec.astype(np.int64).reshape(by, bx, 8)
    usable = q[..., 6] == 0
    hx, hy = np.where(usable, _round_half_even_div4(q[..., 4]), 0), np.where(usable, _round_half_even_div4(q[..., 5]), 0)
    at = mp[np.clip(yc + hy, 0, H - 1), np.clip(xc + hx, 0, W - 1)]
    px, py = hx + (at[..., 0] >> 2), hy + (at[..., 1] >> 2)               # pred(q) of every block
    co = mp[np.broadcast_to(yc, (by, bx)), np.broadcast_to(xc, (by, bx))] >> 2
    yes, zero = np.ones((by, bx), dtype=bool), np.zeros((by, bx), dtype=np.int64)

    def neighbour(v, di, dj, fill):                                      # v of block (bi + di, bj + dj); fill where that is off the grid
        out = np.full((by, bx), fill, dtype=v.dtype)
        out[max(0, -di):by - max(0, di), max(0, -dj):bx - max(0, dj)] = v[max(0, di):by - max(0, -di), max(0, dj):bx - max(0, -dj)]
        return out

    centres = [(zero, zero, yes), (px, py, yes), (co[..., 0], co[..., 1], yes)]
    centres += [(neighbour(px, di, dj, 0), neighbour(py, di, dj, 0), neighbour(usable, di, dj, False)) for di, dj in ((0, -1), (0, 1), (-1, 0), (1, 0))]
    best = _bm_best_key(a, k, B, r, centres, lambda sad, dx, dy: ((sad + lam * (np.abs(dx - px) + np.abs(dy - py))) << 28) | (((dy + 8192) << 14) | (dx + 8192)))
    dy, dx = ((best >> 14) & 16383) - 8192, (best & 16383) - 8192
    drift = np.abs(dx - px) + np.abs(dy - py)
    sad = (best >> 28) - lam * drift
    anchored = sad <= intra * (h[:, None] * w[None, :])
    out = q.copy()
    new = np.zeros((by, bx, 8), dtype=np.int64)
    new[..., 0], new[..., 1], new[..., 2], new[..., 3] = x0[None, :], y0[:, None], w[None, :], h[:, None]
    new[..., 4], new[..., 5], new[..., 6] = 4 * dx, 4 * dy, f - 1
    out[anchored] = new[anchored]
    stats = np.array([anchored.sum(), (anchored & ~usable).sum(), (~anchored).sum(), drift[anchored].sum()], dtype=np.int64)
    return np.ascontiguousarray(out.reshape(-1, 8).astype(np.int16)), np.where(anchored, sad, -1).reshape(-1).astype(np.int64), stats


BMS_NSTATS = _lib.BMS_NSTATS          # ARSEG_BMS_NSTATS: parents split, unusable parents split, children matched / intra, summed gain, matched pixels


def block_motion_split_numpy(cur, ref, records, r: int = 2, lam: int = 2, intra: int = 255, split_gain: int = 32, ref_index: int = 0):
    """The quad-tree split of include/arseg_hip.h (arseg_block_motion_split_fwd) on the host: ``cur`` / ``ref`` are uint8 luma planes [H,W],
    ``records`` the int16 [by*bx,8] records of the B = 16 grid (``block_motion_numpy``, ``block_motion_pyr_numpy``).  Returns ``(children int16
    [4*by*bx,8], child_sad uint32 [4*by*bx], stats int64 [BMS_NSTATS])`` -- what ``ops.block_motion_split`` writes, stats from zero;
    ``np.concatenate([records, children])`` is the list a chain takes.  numpy only, one gather of the frame per centre and offset."""
    a, k = luma8_numpy(cur).astype(np.int32), luma8_numpy(ref).astype(np.int32)
    r, lam, intra, split_gain, ref_index = int(r), int(lam), int(intra), int(split_gain), int(ref_index)
    H, W = a.shape
    if k.shape != a.shape:
        raise ValueError(f"block_motion_split_numpy: the current frame is {a.shape}, the reference {k.shape}")
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 or not 0 <= split_gain <= 65535 \
            or not 0 <= ref_index <= 15:
        raise ValueError(f"block_motion_split_numpy: H, W in 1..8192, r in 1..3, lam and intra in 0..255, split_gain in 0..65535, ref_index in 0..15; got "
                         f"{H}x{W}, r {r}, lam {lam}, intra {intra}, split_gain {split_gain}, ref_index {ref_index}")
    by, bx = -(-H // 16), -(-W // 16)
    rec = np.asarray(records)
    if rec.dtype != np.int16 or rec.shape != (by * bx, 8):
        raise ValueError(f"block_motion_split_numpy: {H}x{W} in blocks of 16 is int16 [{by * bx},8] records, got {rec.dtype} {rec.shape}")
    q = rec.astype(np.int64).reshape(by, bx, 8)
    px0, py0 = (np.arange(bx) * 16)[None, :], (np.arange(by) * 16)[:, None]
    pw, ph = np.minimum(16, W - px0), np.minimum(16, H - py0)
    Px, Py = _round_half_even_div4(q[..., 4]), _round_half_even_div4(q[..., 5])
    usable = (q[..., 6] == ref_index) & (np.abs(Px) <= 500) & (np.abs(Py) <= 500) & (px0 + Px >= 0) & (px0 + pw + Px <= W) & (py0 + Py >= 0) \
        & (py0 + ph + Py <= H)
    # the children that exist are the blocks of the B = 8 grid: child (ci, cj) is child 2 (ci & 1) + (cj & 1) of parent (ci >> 1, cj >> 1)
    cby, cbx = -(-H // 8), -(-W // 8)
    ci, cj = np.arange(cby), np.arange(cbx)
    pi, pj = ci >> 1, cj >> 1
    ni, nj = pi + np.where(ci & 1, 1, -1), pj + np.where(cj & 1, 1, -1)
    oki, okj = (ni >= 0) & (ni < by), (nj >= 0) & (nj < bx)
    ni, nj = np.clip(ni, 0, by - 1), np.clip(nj, 0, bx - 1)
    yes, zero = np.ones((cby, cbx), dtype=bool), np.zeros((cby, cbx), dtype=np.int64)
    own = (Px[pi][:, pj], Py[pi][:, pj], usable[pi][:, pj])
    centres = [(zero, zero, yes), own,
               (Px[pi][:, nj], Py[pi][:, nj], usable[pi][:, nj] & okj[None, :]),
               (Px[ni][:, pj], Py[ni][:, pj], usable[ni][:, pj] & oki[:, None])]

    def key_of(sad, dx, dy):
        return ((sad + lam * (np.abs(dx) + np.abs(dy))) << 20) | np.where((dx == 0) & (dy == 0), 0, 1 + (dy + 511) * 1023 + (dx + 511))

    best = _bm_best_key(a, k, 8, r, centres, key_of)
    rank, cost = best & 0xfffff, best >> 20
    dy = np.where(rank > 0, (rank - 1) // 1023 - 511, 0)
    dx = np.where(rank > 0, (rank - 1) % 1023 - 511, 0)
    sad = cost - lam * (np.abs(dx) + np.abs(dy))
    at_p = np.where(own[2], _bm_best_key(a, k, 8, 0, [own], lambda s, dx, dy: s), 0)      # S_q(P): P is a candidate of every child of a usable parent
    x0, y0 = (cj * 8)[None, :], (ci * 8)[:, None]
    w, h = np.minimum(8, W - x0), np.minimum(8, H - y0)
    matched = sad <= intra * (w * h)

    def per_parent(v):                                                  # [cby,cbx] -> [by,bx,4], child q = 2 qy + qx last; 0 where the child does not exist
        full = np.zeros((2 * by, 2 * bx), dtype=np.int64)
        full[:cby, :cbx] = v
        return full.reshape(by, 2, bx, 2).transpose(0, 2, 1, 3).reshape(by, bx, 4)

    exists = per_parent(yes).astype(bool)
    lhs = per_parent(at_p).sum(axis=2) + lam * (np.abs(Px) + np.abs(Py)) - per_parent(cost).sum(axis=2)
    m = per_parent(matched).astype(bool)
    split = np.where(usable, lhs > split_gain, m.any(axis=2))
    row = np.zeros((cby, cbx, 8), dtype=np.int64)
    row[..., 0], row[..., 1], row[..., 2], row[..., 3] = x0, y0, w, h
    row[..., 4], row[..., 5], row[..., 6] = np.where(matched, 4 * dx, 0), np.where(matched, 4 * dy, 0), np.where(matched, ref_index, BM_INTRA_REF)
    rows = np.stack([per_parent(row[..., c]) for c in range(8)], axis=-1)               # [by,bx,4,8]
    write = split[..., None] & exists
    children = np.where(write[..., None], rows, 0)
    pixels = per_parent(np.where(matched, w * h, 0))
    stats = np.array([split.sum(), (split & ~usable).sum(), (write & m).sum(), (write & ~m).sum(), lhs[split & usable].sum(), pixels[write & m].sum()],
                     dtype=np.int64)
    return np.ascontiguousarray(children.reshape(-1, 8).astype(np.int16)), per_parent(sad).reshape(-1).astype(np.uint32), stats


HEAL_NSTATS = _lib.HEAL_NSTATS        # ARSEG_HEAL_NSTATS: examined blocks, healed blocks, flagged pixels examined, pixels healed, flagged pixels skipped, drift


def mv_chain_heal_numpy(cur, key, merged_f, link_f, B: int = 16, r: int = 2, lam: int = 2, intra: int = 20, flag_mask: int = LINK_INTRA | LINK_UNCOVERED,
                        min_flagged: int = 1, link_stats_row=None):
    """The chain healing of include/arseg_hip.h (arseg_mv_chain_heal_fwd) on the host: ``cur`` / ``key`` are uint8 luma planes [H,W] of frame f and
    of the keyframe, ``merged_f`` int16 [H,W,2] and ``link_f`` uint8 [H,W] the chain's merged[f] and link[f] (not modified: copies are returned),
    ``link_stats_row`` int64 [LINK_NSTATS] row f of the chain's counters or None.  Returns ``(merged_f, link_f, decisions int16 [by*bx,8],
    sad int64 [by*bx] with -1 for a skipped block (the entries the device form leaves untouched), stats int64 [HEAL_NSTATS] from zero,
    link_stats_row corrected or None)``.  numpy only: the examined blocks are gathered once, then one gather of the keyframe per centre and
    offset over those blocks alone."""
    a, k = luma8_numpy(cur).astype(np.int32), luma8_numpy(key).astype(np.int32)
    B, r, lam, intra, flag_mask, min_flagged = int(B), int(r), int(lam), int(intra), int(flag_mask), int(min_flagged)
    H, W = a.shape
    if k.shape != a.shape:
        raise ValueError(f"mv_chain_heal_numpy: the current frame is {a.shape}, the keyframe {k.shape}")
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or B not in (8, 16) or not 1 <= r <= 3 or not 0 <= lam <= 255 or not 0 <= intra <= 255 \
            or not 1 <= flag_mask <= 7 or not 1 <= min_flagged <= 64:
        raise ValueError(f"mv_chain_heal_numpy: H, W in 1..8192, B in (8, 16), r in 1..3, lam and intra in 0..255, flag_mask in 1..7, min_flagged in 1..64; "
                         f"got {H}x{W}, B {B}, r {r}, lam {lam}, intra {intra}, flag_mask {flag_mask}, min_flagged {min_flagged}")
    m, l = np.array(merged_f), np.array(link_f)
    if m.dtype != np.int16 or m.shape != (H, W, 2) or l.dtype != np.uint8 or l.shape != (H, W):
        raise ValueError(f"mv_chain_heal_numpy: merged_f is int16 [{H},{W},2] and link_f uint8 [{H},{W}], got {m.dtype} {m.shape} and {l.dtype} {l.shape}")
    row = None
    if link_stats_row is not None:
        row = np.array(link_stats_row, dtype=np.int64)
        if row.shape != (_lib.LINK_NSTATS,):
            raise ValueError(f"mv_chain_heal_numpy: link_stats_row is int64 [{_lib.LINK_NSTATS}], got {row.shape}")
    by, bx = -(-H // B), -(-W // B)
    flagged = (l & flag_mask) != 0
    fp = np.zeros((by * B, bx * B), dtype=bool)
    fp[:H, :W] = flagged
    n_all = fp.reshape(by, B, bx, B).sum(axis=(1, 3), dtype=np.int64)
    gx0, gy0 = np.arange(bx) * B, np.arange(by) * B
    gw, gh = np.minimum(B, W - gx0), np.minimum(B, H - gy0)
    dec = np.zeros((by, bx, 8), dtype=np.int64)
    dec[..., 0], dec[..., 1], dec[..., 2], dec[..., 3], dec[..., 6], dec[..., 7] = gx0[None, :], gy0[:, None], gw[None, :], gh[:, None], 2, n_all
    sad = np.full((by, bx), -1, dtype=np.int64)
    stats = np.zeros(HEAL_NSTATS, dtype=np.int64)
    examined = n_all >= min_flagged
    stats[4] = n_all[~examined].sum()
    bi, bj = np.nonzero(examined)
    if bi.size:
        x0, y0, w, h, nf = gx0[bj], gy0[bi], gw[bj], gh[bi], n_all[bi, bj]
        Y, X = y0[:, None, None] + np.arange(B)[None, :, None], x0[:, None, None] + np.arange(B)[None, None, :]
        inside = (Y < H) & (X < W)
        Yc, Xc = np.minimum(Y, H - 1), np.minimum(X, W - 1)
        blk = a[Yc, Xc] * inside
        fl = flagged[Yc, Xc] & inside
        mq = m.astype(np.int64) >> 2
        yes, zero = np.ones(bi.size, dtype=bool), np.zeros(bi.size, dtype=np.int64)
        c1 = mq[y0 + h // 2, x0 + w // 2]
        centres = [(zero, zero, yes), (c1[:, 0], c1[:, 1], yes)]
        for di, dj in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            qi, qj = bi + di, bj + dj
            ok = (qi >= 0) & (qi < by) & (qj >= 0) & (qj < bx)
            qi, qj = np.clip(qi, 0, by - 1), np.clip(qj, 0, bx - 1)
            yc, xc = gy0[qi] + gh[qi] // 2, gx0[qj] + gw[qj] // 2
            c = mq[yc, xc]
            centres.append((c[:, 0], c[:, 1], ok & ~flagged[yc, xc]))
        un = (inside & ~fl).reshape(bi.size, B * B)
        first = un.argmax(axis=1)                                        # raster order within the block
        c = mq[np.minimum(y0 + first // B, H - 1), np.minimum(x0 + first % B, W - 1)]
        centres.append((c[:, 0], c[:, 1], un.any(axis=1)))
        for j in range(len(centres)):                                  # the union is a set: a centre equal to an earlier one proposes nothing new
            for cx, cy, ok in centres[:j]:
                centres[j] = (centres[j][0], centres[j][1], centres[j][2] & ~(ok & (cx == centres[j][0]) & (cy == centres[j][1])))
        best = np.full(bi.size, 1 << 62, dtype=np.int64)
        for cx, cy, ok in centres:
            for oy in range(-r, r + 1):
                for ox in range(-r, r + 1):
                    dx, dy = cx + ox, cy + oy
                    valid = ok & (x0 + dx >= 0) & (x0 + w + dx <= W) & (y0 + dy >= 0) & (y0 + h + dy <= H)
                    if not valid.any():
                        continue
                    ref = k[np.clip(Y + dy[:, None, None], 0, H - 1), np.clip(X + dx[:, None, None], 0, W - 1)]
                    s_all = (np.abs(blk - ref) * inside).sum(axis=(1, 2), dtype=np.int64)
                    kq = ((s_all + lam * (np.abs(dx - c1[:, 0]) + np.abs(dy - c1[:, 1]))) << 28) | (((dy + 8192) << 14) | (dx + 8192))
                    best = np.where(valid & (kq < best), kq, best)
        dy, dx = ((best >> 14) & 16383) - 8192, (best & 16383) - 8192
        drift = np.abs(dx - c1[:, 0]) + np.abs(dy - c1[:, 1])
        ref = k[np.clip(Y + dy[:, None, None], 0, H - 1), np.clip(X + dx[:, None, None], 0, W - 1)]
        s_fl = (np.abs(blk - ref) * fl).sum(axis=(1, 2), dtype=np.int64)
        healed = s_fl <= intra * nf
        dec[bi, bj, 4], dec[bi, bj, 5], dec[bi, bj, 6] = 4 * dx, 4 * dy, np.where(healed, 0, 1)
        sad[bi, bj] = s_fl
        stats[:4] = bi.size, healed.sum(), nf.sum(), nf[healed].sum()
        stats[5] = drift[healed].sum()
        pix = fl & healed[:, None, None]
        ys, xs = np.broadcast_to(Y, pix.shape)[pix], np.broadcast_to(X, pix.shape)[pix]
        if row is not None and ys.size:
            old = l[ys, xs].astype(np.int64)
            row[:4] -= np.array([(old & 1).sum(), ((old >> 1) & 1).sum(), ((old >> 2) & 1).sum(), ((old & 7) != 0).sum()])
            row[4:] -= np.bincount(old >> 4, minlength=16)
            row[4 + 1] += ys.size
        m[ys, xs, 0] = np.broadcast_to((4 * dx)[:, None, None], pix.shape)[pix]
        m[ys, xs, 1] = np.broadcast_to((4 * dy)[:, None, None], pix.shape)[pix]
        l[ys, xs] = 0x10
    return m, l, np.ascontiguousarray(dec.reshape(-1, 8).astype(np.int16)), sad.reshape(-1), stats, row


class LumaPyramid(object):
    """The luma8 pyramid of one frame on the GPU (include/arseg_hip.h, arseg_luma_pyramid_fwd; csrc/block_motion_pyr.hip): one uint8 buffer,
    allocated once.  ``build(frame)`` fills it from a one-frame ``DecodedFrames`` -- one launch, no synchronisation, no allocation -- and
    returns the pyramid; ``level(l)`` is the [H_l, W_l] view of level l (rows ``pitch`` bytes apart).  A caller of ``MotionEstimator(levels=L)``
    who keeps two of these and alternates them builds each frame of a stream once."""

    def __init__(self, H: int, W: int, levels: int, device="cuda"):
        self.H, self.W, self.levels = int(H), int(W), int(levels)
        try:
            self.layout, self.nbytes = luma_pyramid_layout(self.H, self.W, self.levels)
        except ValueError as e:
            raise _lib.ArsegError(str(e)) from None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ArsegError("LumaPyramid lives on the GPU; there is no CPU fallback (luma_pyramid_numpy is the host form)")
        self.buffer = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)

    def build(self, frame) -> "LumaPyramid":
        if not isinstance(frame, DecodedFrames) or frame.N != 1 or (frame.H, frame.W) != (self.H, self.W):
            raise _lib.ArsegError(f"LumaPyramid.build: expected one DecodedFrames frame of {self.H}x{self.W}")
        plane, src_format = frame.luma_plane()
        ops.luma_pyramid(plane, src_format, self.levels, out=self.buffer)
        return self

    def level(self, l: int) -> torch.Tensor:
        off, pitch, H, W = self.layout[l]
        return self.buffer[off:off + pitch * H].view(H, pitch)[:, :W]


def _luma_in_place(owner: str, who: str, what: str, frame, H: int, W: int, device) -> torch.Tensor:
    """The uint8 luma plane [H,W] that the keyframe anchor and the chain healing read in place: level 0 of a built ``LumaPyramid`` of this size,
    or the luma plane of a one-frame NV12 / I420 ``DecodedFrames`` if it meets their alignment rule.  ``MotionEstimator`` and ``ChainHealer``
    both take their frames through here."""
    if isinstance(frame, LumaPyramid):
        if (frame.H, frame.W, frame.device) != (H, W, device):
            raise _lib.ArsegError(f"{owner}.{who}: {what} must be a LumaPyramid of {H}x{W} on {device}")
        return frame.level(0)
    if not isinstance(frame, DecodedFrames) or frame.N != 1 or (frame.H, frame.W) != (H, W):
        raise _lib.ArsegError(f"{owner}.{who}: expected one DecodedFrames frame of {H}x{W} or a built LumaPyramid")
    plane, src_format = frame.luma_plane()
    p = plane[0]
    if src_format not in (_lib.SRC_NV12, _lib.SRC_I420) or p.device != device or p.stride(1) != 1 or p.data_ptr() % 4 \
            or (H > 1 and (p.stride(0) % 4 or p.stride(0) < ((W + 3) & ~3))):
        raise _lib.ArsegError(f"{owner}.{who}: with levels=0 the anchor reads the frame's own luma plane, which must be an NV12 / I420 byte "
                              f"plane on {device} with a 4-byte aligned base and a pitch that is a multiple of 4; any other frame needs levels >= 1 "
                              f"(level 0 of the luma pyramid is such a plane)")
    return p


class MotionEstimator(object):
    """Motion for streams whose decoder hands over frames and no motion vectors (a hardware decoder's NV12 / P010 output): block matching of
    a frame's luma against the previous frame's on the GPU (csrc/block_motion.hip), written as the block records ``MotionChain.push`` takes.

        est, chain = MotionEstimator(H, W), MotionChain(H, W, gop=12, max_ref=1, track_links=True)
        for each GOP:   chain.reset();  for each P-frame:  mv_q = chain.push(est.estimate(cur, prev))          # cur, prev: one-frame DecodedFrames

    Owns ``records`` int16 [ceil(H/block) * ceil(W/block), 8], ``stats`` int64 [BM_NSTATS] and, ``with_sad=True``, ``sad`` (the winner's SAD per
    block; int32 holding the uint32 bits), all allocated once: ``estimate`` is one launch that neither synchronises nor allocates, so
    ``chain.push(est.estimate(cur, prev))`` over static frame buffers can be captured in a HIP graph.  ``block`` in (8, 16); ``search``: |dx|, |dy|
    <= search, 1..32, whole pixels; cost = SAD + ``lam`` (|dx| + |dy|); a block whose best SAD exceeds ``intra`` per pixel is written intra
    (``BM_INTRA_REF``: the chain flags it ``LINK_INTRA``; 255 never fires); ``ref_index`` goes into every matched record (0 = the reference
    frame is the previous one).  The definition is include/arseg_hip.h (arseg_block_motion_fwd); ``block_motion_numpy`` is its host form.

    ``levels`` in 1 .. 3 makes the search hierarchical (csrc/block_motion_pyr.hip; arseg_block_motion_pyr_fwd; host form
    ``block_motion_pyr_numpy``): ``search`` then counts pixels of pyramid level ``levels``, every level below it looks +-``refine`` (1 .. 3)
    around its parents' doubled vectors, and ``reach`` = search 2^levels + refine (2^levels - 1) is the largest |dx|, |dy| in frame pixels.
    ``estimate`` then takes a ``DecodedFrames`` or an already built ``LumaPyramid`` for either argument; a frame is built into one of two
    pyramids the estimator owns (two more launches), so a caller who alternates two ``LumaPyramid``s of their own builds each frame once.
    Still no synchronisation and no allocation.  ``levels=0`` is the full search, launch for launch.

    ``anchor_refine`` in 1 .. 3 adds keyframe anchoring (csrc/block_motion_anchor.hip; arseg_block_motion_anchor_fwd; host form
    ``block_motion_anchor_numpy``): hops to the previous frame compound their errors over a GOP, and a block that was intra once stays
    flagged for the rest of it.  ``set_key(frame)`` once per GOP, then

        chain.push(est.estimate_anchored(cur, prev, chain))

    is ``estimate`` plus one launch that matches every block against the keyframe within +-``anchor_refine`` of the displacement the chain
    would compose for it (and of its neighbours' and the co-located one), and rewrites a block whose SAD is at most ``anchor_intra`` per
    pixel with ref = f - 1: target frame 0, one hop, this hop's flags only.  The chain needs ``max_ref`` >= its GOP's last frame index (at
    most 16).  The result is in ``anchored`` (a second record buffer; ``records`` keeps the hops), the counts in ``anchor_stats``.  With 0
    nothing of this is allocated and every path above is launch for launch as before.

    ``split_refine`` in 1 .. 3 adds the quad-tree split (csrc/block_motion_split.hip; arseg_block_motion_split_fwd; host form
    ``block_motion_split_numpy``): one vector per 16 x 16 block warps part of a block that straddles two motions from the wrong place.
    ``estimate`` then is the search plus one launch that searches the four 8 x 8 children of every block within +-``split_refine`` of the
    block's and its neighbours' vectors and writes them as records of their own where they undercut the block's cost by more than
    ``split_gain`` (0 .. 65535), or where an intra block has a child that matches.  It needs ``block=16`` and ``anchor_refine=0``.  One buffer
    ``records_all`` int16 [5 n_blocks, 8] is allocated once; ``records`` is the view of its first n_blocks rows, where the search writes,
    ``children`` the view of the rest, and ``estimate`` returns ``records_all``: the children have the higher indices and win their pixels, a
    child row of a block that was not split is eight zeros and covers nothing, so the count is fixed and ``chain.push(est.estimate(cur,
    prev))`` stays capturable.  With ``levels`` >= 1 the split reads level 0 of the two pyramids; with ``levels=0`` the frames' own luma
    planes in place, which must be NV12 / I420 byte planes with a 4-byte aligned base and pitch.  The counts are in ``split_stats``;
    ``with_sad=True`` also owns ``child_sad``.  With 0 nothing of this is allocated and every path above is launch for launch as before."""

    def __init__(self, H: int, W: int, block: int = 16, search: int = 16, lam: int = 2, intra: int = 255, ref_index: int = 0, device="cuda",
                 with_sad: bool = False, levels: int = 0, refine: int = 1, anchor_refine: int = 0, anchor_intra: int = 255, split_refine: int = 0,
                 split_gain: int = 32):
        self.H, self.W, self.block, self.search = int(H), int(W), int(block), int(search)
        self.lam, self.intra, self.ref_index = int(lam), int(intra), int(ref_index)
        self.levels, self.refine = int(levels), int(refine)
        self.anchor_refine, self.anchor_intra = int(anchor_refine), int(anchor_intra)
        try:
            _bm_args("MotionEstimator", self.H, self.W, self.block, self.search, self.lam, self.intra, self.ref_index)
            _bmp_args("MotionEstimator", self.levels, self.refine)
        except ValueError as e:
            raise _lib.ArsegError(str(e)) from None
        if not 0 <= self.anchor_refine <= 3 or not 0 <= self.anchor_intra <= 255:
            raise _lib.ArsegError(f"MotionEstimator: anchor_refine in 0..3 and anchor_intra in 0..255; got {self.anchor_refine}, {self.anchor_intra}")
        self.split_refine, self.split_gain = int(split_refine), int(split_gain)
        if not 0 <= self.split_refine <= 3 or not 0 <= self.split_gain <= 65535:
            raise _lib.ArsegError(f"MotionEstimator: split_refine in 0..3 and split_gain in 0..65535; got {self.split_refine}, {self.split_gain}")
        if self.split_refine and self.block != 16:
            raise _lib.ArsegError(f"MotionEstimator: split_refine splits 16 x 16 blocks into 8 x 8 children and needs block=16, got block={self.block}")
        if self.split_refine and self.anchor_refine:
            raise _lib.ArsegError("MotionEstimator: split_refine and anchor_refine do not combine (splitting anchored records is not covered)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ArsegError("MotionEstimator runs on the GPU only; there is no CPU fallback (block_motion_numpy is the host form)")
        self.n_blocks = -(-self.H // self.block) * -(-self.W // self.block)
        if self.split_refine:
            self.records_all = torch.zeros((5 * self.n_blocks, 8), dtype=torch.int16, device=self.device)
            self.records, self.children = self.records_all[:self.n_blocks], self.records_all[self.n_blocks:]
            self.split_stats = torch.zeros(BMS_NSTATS, dtype=torch.int64, device=self.device)
            self.child_sad = torch.zeros(4 * self.n_blocks, dtype=torch.int32, device=self.device) if with_sad else None
        else:
            self.records = torch.zeros((self.n_blocks, 8), dtype=torch.int16, device=self.device)
        self.stats = torch.zeros(BM_NSTATS, dtype=torch.int64, device=self.device)
        self.sad = torch.zeros(self.n_blocks, dtype=torch.int32, device=self.device) if with_sad else None
        if self.levels:
            self._pyramids = (LumaPyramid(self.H, self.W, self.levels, self.device), LumaPyramid(self.H, self.W, self.levels, self.device))
            nbytes = _lib.load().arseg_block_motion_pyr_workspace_bytes(self.H, self.W, self.block, self.levels)
            self._workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._key_plane = self._cur_pyramid = None
        if self.anchor_refine:
            self.anchored = torch.zeros((self.n_blocks, 8), dtype=torch.int16, device=self.device)
            self.anchor_stats = torch.zeros(BMA_NSTATS, dtype=torch.int64, device=self.device)
            self._key_pyramid = LumaPyramid(self.H, self.W, self.levels, self.device) if self.levels else None

    @property
    def reach(self) -> int:
        """The largest |dx|, |dy| a record can carry, in frame pixels."""
        return self.search * (1 << self.levels) + self.refine * ((1 << self.levels) - 1) if self.levels else self.search

    def _estimate_pyr(self, cur, ref) -> torch.Tensor:
        pyr = []
        for what, f, own in (("the current frame", cur, self._pyramids[0]), ("the reference frame", ref, self._pyramids[1])):
            if isinstance(f, LumaPyramid):
                if (f.H, f.W, f.levels, f.device) != (self.H, self.W, self.levels, self.device):
                    raise _lib.ArsegError(f"MotionEstimator.estimate: {what} must be a LumaPyramid of {self.H}x{self.W} with {self.levels} levels on {self.device}")
                pyr.append(f)
            elif isinstance(f, DecodedFrames) and f.N == 1 and (f.H, f.W) == (self.H, self.W):
                pyr.append(own.build(f))
            else:
                raise _lib.ArsegError(f"MotionEstimator.estimate: {what} must be one DecodedFrames frame of {self.H}x{self.W} or a built LumaPyramid")
        self._cur_pyramid = pyr[0]
        ops.block_motion_pyr(pyr[0].buffer, pyr[1].buffer, self.H, self.W, self.levels, self.block, self.search, self.refine, self.lam, self.intra,
                             self.ref_index, records=self.records, sad=self.sad if self.sad is not None else False, stats=self.stats,
                             workspace=self._workspace)
        return self._split(pyr[0].level(0), pyr[1].level(0)) if self.split_refine else self.records

    def _split(self, cur_plane, ref_plane) -> torch.Tensor:
        """The split launch on the records the search has just written -> ``records_all``."""
        ops.block_motion_split(cur_plane, ref_plane, self.records, self.split_refine, self.lam, self.intra, self.split_gain, self.ref_index,
                               children=self.children, sad=self.child_sad if self.child_sad is not None else False, stats=self.split_stats)
        return self.records_all

    def estimate(self, cur, ref) -> torch.Tensor:
        """Two one-frame ``DecodedFrames`` of one format and of this estimator's size, on its device -> ``records`` (the same buffer every call);
        with ``split_refine`` -> ``records_all``.  With ``levels`` >= 1 either may be a built ``LumaPyramid`` instead, and the two frames may
        differ in format."""
        if self.levels:
            return self._estimate_pyr(cur, ref)
        for what, f in (("the current frame", cur), ("the reference frame", ref)):
            if not isinstance(f, DecodedFrames) or f.N != 1 or (f.H, f.W) != (self.H, self.W):
                raise _lib.ArsegError(f"MotionEstimator.estimate: {what} must be one DecodedFrames frame of {self.H}x{self.W}")
        if cur.src_format != ref.src_format:
            raise _lib.ArsegError(f"MotionEstimator.estimate: the frames differ in format ({cur.src_format} and {ref.src_format})")
        planes = (self._aligned_luma(cur, "estimate"), self._aligned_luma(ref, "estimate")) if self.split_refine else None
        ops.block_motion(cur.luma_plane()[0], ref.luma_plane()[0], cur.src_format, self.block, self.search, self.lam, self.intra, self.ref_index,
                         records=self.records, sad=self.sad if self.sad is not None else False, stats=self.stats)
        return self._split(*planes) if self.split_refine else self.records

    def _aligned_luma(self, frame, who):
        """The uint8 luma plane [H,W] of a one-frame NV12 / I420 ``DecodedFrames`` if it meets the anchor's alignment rule."""
        if isinstance(frame, LumaPyramid):                            # with levels=0 a pyramid is a keyframe only
            raise _lib.ArsegError(f"MotionEstimator.{who}: expected one DecodedFrames frame of {self.H}x{self.W} or a built LumaPyramid")
        return _luma_in_place("MotionEstimator", who, "the frame", frame, self.H, self.W, self.device)

    def set_key(self, frame) -> None:
        """The keyframe of the GOP that ``estimate_anchored`` anchors on: a one-frame ``DecodedFrames`` (with ``levels`` >= 1 built into a third
        pyramid the estimator owns: one launch; with ``levels=0`` an NV12 / I420 frame whose luma plane is 4-byte aligned, read in place) or a
        built ``LumaPyramid`` of this size, whose level 0 is read in place.  No synchronisation, no allocation."""
        if not self.anchor_refine:
            raise _lib.ArsegError("MotionEstimator.set_key: this estimator was made with anchor_refine=0")
        if isinstance(frame, LumaPyramid) or not self.levels:
            self._key_plane = _luma_in_place("MotionEstimator", "set_key", "the keyframe", frame, self.H, self.W, self.device)
        else:
            if not isinstance(frame, DecodedFrames) or frame.N != 1 or (frame.H, frame.W) != (self.H, self.W):
                raise _lib.ArsegError(f"MotionEstimator.set_key: expected one DecodedFrames frame of {self.H}x{self.W} or a built LumaPyramid")
            self._key_plane = self._key_pyramid.build(frame).level(0)

    def estimate_anchored(self, cur, ref, chain) -> torch.Tensor:
        """``estimate(cur, ref)``, then one anchor launch for frame f = ``chain.f`` + 1 against the keyframe of ``set_key`` with ``chain.merged[f - 1]``
        -> ``anchored`` (the same buffer every call), which ``chain.push`` takes.  ``chain`` is the in-order ``MotionChain`` the result is pushed
        to next; it is read, not advanced.  Raises for a bidirectional chain, for ``chain.max_ref`` < f (ref = f - 1 would be unusable), for a
        size or device mismatch and before ``set_key``.  Neither synchronises nor allocates."""
        if not self.anchor_refine:
            raise _lib.ArsegError("MotionEstimator.estimate_anchored: this estimator was made with anchor_refine=0")
        if self._key_plane is None:
            raise _lib.ArsegError("MotionEstimator.estimate_anchored: set_key(frame) first, once per GOP")
        if not isinstance(chain, MotionChain) or chain.bidirectional:
            raise _lib.ArsegError("MotionEstimator.estimate_anchored: anchoring needs an in-order MotionChain (bidirectional chains are not covered)")
        if (chain.H, chain.W, chain.device) != (self.H, self.W, self.device):
            raise _lib.ArsegError(f"MotionEstimator.estimate_anchored: the chain is {chain.H}x{chain.W} on {chain.device}, the estimator {self.H}x{self.W} on {self.device}")
        f = chain.f + 1
        if f >= chain.gop or f > 16 or chain.max_ref < f:
            raise _lib.ArsegError(f"MotionEstimator.estimate_anchored: frame {f} needs a chain with gop > {f} and max_ref >= {f} (at most 16): an anchored "
                                  f"record carries ref = {f - 1}; the chain has gop {chain.gop}, max_ref {chain.max_ref}")
        cur_plane = None if self.levels else self._aligned_luma(cur, "estimate_anchored")
        records = self.estimate(cur, ref)
        if self.levels:
            cur_plane = self._cur_pyramid.level(0)
        ops.block_motion_anchor(cur_plane, self._key_plane, records, chain.merged[f - 1] if f >= 2 else None, f, self.block, self.anchor_refine, self.lam,
                                self.anchor_intra, out=self.anchored, sad=self.sad if self.sad is not None else False, stats=self.anchor_stats)
        return self.anchored

    def reset_stats(self) -> None:
        self.stats.zero_()
        if self.anchor_refine:
            self.anchor_stats.zero_()
        if self.split_refine:
            self.split_stats.zero_()

    def split_stats_row(self) -> torch.Tensor:
        """int64 [BMS_NSTATS], accumulated since ``reset_stats``: blocks split, of those the intra blocks (healed), child records written matched
        and intra, the summed gain of the split matched blocks, and the pixels in matched children.  A device tensor: reading it on the host
        synchronises."""
        if not self.split_refine:
            raise _lib.ArsegError("MotionEstimator.split_stats_row: this estimator was made with split_refine=0")
        return self.split_stats

    def anchor_stats_row(self) -> torch.Tensor:
        """int64 [BMA_NSTATS], accumulated since ``reset_stats``: anchored blocks, anchored blocks whose hop was unusable (healed), blocks kept on
        their hop, and the drift corrected (sum of |anchor - chain's prediction| in pixels).  A device tensor: reading it on the host synchronises."""
        if not self.anchor_refine:
            raise _lib.ArsegError("MotionEstimator.anchor_stats_row: this estimator was made with anchor_refine=0")
        return self.anchor_stats

    def stats_row(self) -> torch.Tensor:
        """int64 [BM_NSTATS], accumulated since ``reset_stats``: intra blocks, matched blocks with the zero vector, the sum of SAD and the
        number of pixels of the matched blocks.  A device tensor: reading it on the host synchronises."""
        return self.stats


class ChainHealer(object):
    """Heals the intra / uncovered pixels of ANY ``MotionChain(track_links=True)`` on the keyframe (csrc/mv_chain_heal.hip;
    arseg_mv_chain_heal_fwd; host form ``mv_chain_heal_numpy``).  A pixel flagged at one hop stays flagged, on zero motion, for the rest of the
    GOP although its content is usually back one frame later; ``MotionEstimator(anchor_refine=...)`` mends that for its own records only.  This
    works on the chain's output, so it takes a software decoder's records of any geometry, bidirectional chains in decode order and any GOP
    length:

        healer, chain = ChainHealer(H, W), MotionChain(H, W, gop=20, bidirectional=True, track_links=True)
        for each GOP:   chain.reset();  healer.set_key(key_frame)
                        for f, records in decode_order:  chain.push(records, at=f);  mv_q = healer.heal(chain, frame_f)

    Every ``block`` x ``block`` tile (8 or 16) with at least ``min_flagged`` pixels whose link byte has a bit of ``flags`` is searched in the
    keyframe within +-``refine`` (1 .. 3) of the chain's own vector at its centre, of its unflagged neighbours and of its own unflagged part;
    where the winner's SAD over the flagged pixels is at most ``intra`` per flagged pixel they get a one-hop vector to the keyframe and a
    clean link byte, in place in ``chain.merged`` / ``chain.link_bytes``, and the frame's row of ``chain.link_counts`` is corrected, so every
    later frame composing through them inherits the healed value and a ``LinkMonitor`` sees the healed counts.  Owns ``decisions`` int16
    [blocks, 8] (x0, y0, w, h, 4 dx, 4 dy, state, flagged pixels; state 0 healed, 1 kept, 2 skipped), ``heal_stats`` int64 [HEAL_NSTATS] and,
    ``with_sad=True``, ``sad``: ``heal`` is two launches that neither synchronise nor allocate, so ``chain.push(records); healer.heal(chain, cur)``
    over static buffers can be captured in a HIP graph."""

    def __init__(self, H: int, W: int, block: int = 16, refine: int = 2, lam: int = 2, intra: int = 20, flags: int = LINK_INTRA | LINK_UNCOVERED,
                 min_flagged: int = 1, device="cuda", with_sad: bool = False):
        self.H, self.W, self.block, self.refine = int(H), int(W), int(block), int(refine)
        self.lam, self.intra, self.flags, self.min_flagged = int(lam), int(intra), int(flags), int(min_flagged)
        if not (1 <= self.H <= 8192 and 1 <= self.W <= 8192) or self.block not in (8, 16) or not 1 <= self.refine <= 3 or not 0 <= self.lam <= 255 \
                or not 0 <= self.intra <= 255 or not 1 <= self.flags <= 7 or not 1 <= self.min_flagged <= 64:
            raise _lib.ArsegError(f"ChainHealer: H, W in 1..8192, block in (8, 16), refine in 1..3, lam and intra in 0..255, flags in 1..7, min_flagged in "
                                  f"1..64; got {self.H}x{self.W}, block {self.block}, refine {self.refine}, lam {self.lam}, intra {self.intra}, flags "
                                  f"{self.flags}, min_flagged {self.min_flagged}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ArsegError("ChainHealer runs on the GPU only; there is no CPU fallback (mv_chain_heal_numpy is the host form)")
        self.n_blocks = -(-self.H // self.block) * -(-self.W // self.block)
        self.decisions = torch.zeros((self.n_blocks, 8), dtype=torch.int16, device=self.device)
        self.heal_stats = torch.zeros(HEAL_NSTATS, dtype=torch.int64, device=self.device)
        self.sad = torch.zeros(self.n_blocks, dtype=torch.int32, device=self.device) if with_sad else None
        self._key_plane = None

    def set_key(self, frame) -> None:
        """The keyframe of the GOP: what ``MotionEstimator.set_key`` takes with ``levels=0`` -- a one-frame NV12 / I420 ``DecodedFrames`` whose luma
        plane is 4-byte aligned, or a built ``LumaPyramid`` of this size -- read in place.  No launch, no synchronisation, no allocation."""
        self._key_plane = _luma_in_place("ChainHealer", "set_key", "the keyframe", frame, self.H, self.W, self.device)

    def heal(self, chain, cur, at=None) -> torch.Tensor:
        """Heals frame ``at`` of ``chain`` (None: the last one pushed) against the keyframe of ``set_key``; ``cur`` is that frame, as ``set_key``
        takes the keyframe.  Works in place on ``chain.merged[at]``, ``chain.link_bytes[at]`` and ``chain.link_counts[at]`` and returns the
        ``mv_q`` view ``chain.merged[at]``.  Raises for a chain without ``track_links``, a frame not pushed, a size or device mismatch and
        before ``set_key``.  Neither synchronises nor allocates."""
        if self._key_plane is None:
            raise _lib.ArsegError("ChainHealer.heal: set_key(frame) first, once per GOP")
        if not isinstance(chain, MotionChain) or not chain.track_links:
            raise _lib.ArsegError("ChainHealer.heal: healing needs a MotionChain(track_links=True): the link bytes say which pixels to heal")
        if (chain.H, chain.W, chain.device) != (self.H, self.W, self.device):
            raise _lib.ArsegError(f"ChainHealer.heal: the chain is {chain.H}x{chain.W} on {chain.device}, the healer {self.H}x{self.W} on {self.device}")
        at = chain.last if at is None else int(at)
        if not 1 <= at < chain.gop or at not in chain.frames_done():
            raise _lib.ArsegError(f"ChainHealer.heal: frame {at} was not pushed in this GOP (pushed: {chain.frames_done()[1:]})")
        cur_plane = _luma_in_place("ChainHealer", "heal", "the current frame", cur, self.H, self.W, self.device)
        ops.mv_chain_heal(cur_plane, self._key_plane, chain.merged[at], chain.link_bytes[at], self.block, self.refine, self.lam, self.intra, self.flags,
                          self.min_flagged, decisions=self.decisions, sad=self.sad if self.sad is not None else False, stats=self.heal_stats,
                          link_stats_row=chain.link_counts[at])
        return chain.merged[at]

    def reset_stats(self) -> None:
        self.heal_stats.zero_()

    def heal_stats_row(self) -> torch.Tensor:
        """int64 [HEAL_NSTATS], accumulated since ``reset_stats``: examined blocks, healed blocks, flagged pixels in examined blocks, pixels
        healed, flagged pixels in skipped blocks, and the sum over healed blocks of |winner - the chain's own vector| in pixels.  A device
        tensor: reading it on the host synchronises."""
        return self.heal_stats
