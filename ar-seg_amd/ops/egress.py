"""The output half of the pipeline: head logits -> an 8-bit label plane and / or the frame with the classes painted over it, one ABI call
(include/arseg_hip.h, arseg_segment_egress_fwd; csrc/egress.hip); head logits -> an 8-bit confidence plane, the label plane and per-frame
statistics, one ABI call (arseg_segment_confidence_fwd; csrc/confidence.hip); head logits, the keyframe's label plane and the motion back to
it -> the label plane held to the keyframe's where the frame's own decision is marginal, one ABI call (arseg_segment_stabilise_fwd;
csrc/stabilise.hip); an 8-bit plane <-> its row-run code, one ABI call each
(arseg_labels_rle_fwd / arseg_rle_decode_fwd; csrc/rle.hip); a row-run code -> its connected regions, one ABI call (arseg_rle_regions_fwd;
csrc/regions.hip); the regions of two frames -> their links along the motion, one ABI call (arseg_region_links_fwd; csrc/links.hip); a row-run
code and its regions -> the code with the small regions absorbed into their neighbours, one ABI call (arseg_rle_absorb_fwd; csrc/absorb.hip);
the regions' outlines as polygon loops (arseg_rle_contours_fwd; csrc/contours.hip) and those simplified to a pixel tolerance
(arseg_contours_simplify_fwd; csrc/simplify.hip) or, with the borders between neighbours simplified once,
(arseg_contours_simplify_shared_fwd; csrc/simplify_shared.hip), one ABI call each; the polygons filled back into a label plane with the
fidelity counters (arseg_contours_fill_fwd; csrc/fill.hip), one ABI call."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._base import _need_gpu, _ptr, _stream, workspace as _workspace
from ._profile import launch
from .layers import _plane_layout

_INNER = {_lib.SRC_RGB8: lambda W: ((W, 3),), _lib.SRC_NV12: lambda W: ((W,), (W // 2, 2)), _lib.SRC_I420: lambda W: ((W,), (W // 2,), (W // 2,))}


def _host_u8(v, n, what):
    """n host values in 0..255 (any integer sequence or array) -> a ctypes uint8 array."""
    a = np.asarray(v)
    if a.size != n or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_) or (a.size and (a.min() < 0 or a.max() > 255)):
        raise ValueError(f"{what}: expected {n} integers in 0..255, got {a.dtype} {a.shape}")
    return (ctypes.c_uint8 * n).from_buffer_copy(np.ascontiguousarray(a, dtype=np.uint8).tobytes())


def _planes(frames, N, H, W, what):
    """(src_format, [(tensor, pitch, image stride)] * planes) of a DecodedFrames-like object (``src_format``, ``planes``)."""
    fmt = getattr(frames, "src_format", None)
    if fmt not in _INNER:
        raise ValueError(f"{what}: an overlay takes 8-bit RGB8, NV12 or I420 frames; 10-bit and other sources are not covered (format {fmt!r})")
    planes = tuple(frames.planes)
    inner = _INNER[fmt](W)
    if len(planes) != len(inner) or any(not torch.is_tensor(t) or t.dtype != torch.uint8 for t in planes):
        raise ValueError(f"{what}: expected {len(inner)} uint8 plane tensors")
    if fmt != _lib.SRC_RGB8 and (H % 2 or W % 2):
        raise ValueError(f"{what}: 4:2:0 needs even H and W, got {H}x{W}")
    _need_gpu(*planes, dtype=torch.uint8)
    out = []
    for i, (t, inn) in enumerate(zip(planes, inner)):
        want = (N, H if i == 0 else H // 2) + tuple(inn)
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: plane {i} must be {want}, got {tuple(t.shape)}")
        out.append((t,) + _plane_layout(t, inn, f"{what} plane {i}"))
    return fmt, out


def _frame_dims(what, H, W, limit=None, positive=True):
    """H and W as ints, or ValueError.  ``limit``: the most either may be (they share a vertex word); None: the run code's own limits, a column
    in 24 bits and a pixel index in 31."""
    H, W = int(H), int(W)
    over = (W > 1 << 24 or H * W > 2 ** 31 - 1) if limit is None else (H > limit or W > limit)
    if over or (positive and (H <= 0 or W <= 0)):
        bounds = "W <= 2^24 and H * W < 2^31" if limit is None else f"H <= {limit} and W <= {limit}"
        raise ValueError(f"{what}: H and W {'positive, ' if positive else ''}{bounds}, got {H}x{W}")
    return H, W


def _dense(what, name, t, dtype, shape, dev=None):
    """``t`` is a contiguous, aligned ``dtype`` tensor of ``shape`` on ``dev`` (None: wherever it lies), or ArsegError.  A None entry of
    ``shape`` stands for any size, and that size is returned: a capacity, or the number of frames.  ``dtype``: one dtype, or those allowed."""
    if t is None:
        raise ValueError(f"{what}: {name} is required")
    kinds = dtype if isinstance(dtype, tuple) else (dtype,)
    _need_gpu(t, dtype=None)
    if t.dtype not in kinds:
        raise _lib.ArsegError(f"{what}: {name} holds {' or '.join(str(k) for k in kinds)}, got {t.dtype}")
    fits = t.dim() == len(shape) and all(want is None or have == want for have, want in zip(t.shape, shape))
    if not fits or not t.is_contiguous() or (dev is not None and t.device != dev) or t.data_ptr() % t.element_size():
        want = ", ".join("capacity" if s is None else str(s) for s in shape)
        raise _lib.ArsegError(f"{what}: {name} must be a contiguous {kinds[0]} [{want}] tensor on {t.device if dev is None else dev}, got "
                              f"{tuple(t.shape)} strides {t.stride()} on {t.device}")
    return next((int(have) for have, want in zip(t.shape, shape) if want is None), None)


def _out_plane(what, name, t, N, H, W, dev):
    """An 8-bit plane ``t`` [N,H,W] on ``dev`` (rows contiguous, any pitch) -> (pitch, image stride); (0, 0) for None."""
    if t is None:
        return 0, 0
    _need_gpu(t, dtype=torch.uint8)
    if tuple(t.shape) != (N, H, W) or t.device != dev:
        raise ValueError(f"{name} must be uint8 {(N, H, W)} on {dev}, got {tuple(t.shape)} on {t.device}")
    return _plane_layout(t, (W,), f"{what} {name}")


def _mv_field(what, mv_q, N, H, W, dev):
    """The dense quarter-pel field: int16 [N,H,W,2], contiguous and 4-byte aligned (a vector is read as one word)."""
    _need_gpu(mv_q, dtype=torch.int16)
    if tuple(mv_q.shape) != (N, H, W, 2) or not mv_q.is_contiguous() or mv_q.device != dev or mv_q.data_ptr() % 4:
        raise _lib.ArsegError(f"{what}: mv_q must be a contiguous, 4-byte aligned int16 {(N, H, W, 2)} tensor on {dev}, got {tuple(mv_q.shape)} "
                              f"strides {mv_q.stride()} on {mv_q.device}")


def _own_workspace(what, workspace, nbytes, dev, align=1):
    """The caller's workspace after its check, or the stream's shared one -> (the tensor, its size in bytes)."""
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    elif not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous() or workspace.data_ptr() % align or \
            workspace.numel() * workspace.element_size() < nbytes:
        raise _lib.ArsegError(f"{what}: workspace must be a contiguous, {align}-byte aligned tensor of at least {nbytes} bytes on {dev}")
    return workspace, workspace.numel() * workspace.element_size()


def segment_egress(logits: torch.Tensor, H: int, W: int, *, align_corners: bool = True, lut=None, labels_out: Optional[torch.Tensor] = None,
                   src=None, dst=None, palette=None, weights=None):
    """Head logits fp32 [N,n_cls,h,w] -> the label plane ``labels_out`` (uint8 [N,H,W], rows contiguous, any row pitch / image stride; value
    ``lut[k]`` or ``k``) and / or the overlay ``dst`` of ``src`` (both ``ingest.DecodedFrames`` of one 8-bit format, RGB8 / NV12 / I420, [N,.,H,W];
    ``dst`` may be ``src``: painted in place), in one launch.  ``k`` is ``argmax_confusion``'s pred for the same ``H, W, align_corners``, bit for
    bit.  ``palette`` [n_cls,3] integers 0..255 in the destination's codes, ``weights`` n_cls integers 0..256, ``lut`` n_cls integers 0..255 (host
    values: lists or arrays of any integer type).
    Allocates nothing: every output is the caller's, so the call can be captured in a HIP graph.  Returns (labels_out, dst)."""
    _need_gpu(logits)
    if logits.dim() != 4 or not logits.is_contiguous():
        raise _lib.ArsegError(f"segment_egress expects contiguous fp32 logits [N,n_cls,h,w], got {tuple(logits.shape)}")
    N, n_cls, h, w = logits.shape
    H, W = int(H), int(W)
    if labels_out is None and dst is None:
        raise ValueError("segment_egress: nothing to write (labels_out and dst are both None)")
    if not 1 <= n_cls <= 32:
        raise ValueError(f"segment_egress: 1..32 classes, got {n_cls}")
    lab_pitch, lab_ns = _out_plane("segment_egress", "labels_out", labels_out, N, H, W, logits.device)
    lut_c = None if lut is None else _host_u8(lut, n_cls, "lut")
    fmt, sp, dp, pal_c, wt_c = 0, [], [], None, None
    if dst is not None:
        if src is None or palette is None or weights is None:
            raise ValueError("segment_egress: an overlay needs src, palette and weights")
        fmt, sp = _planes(src, N, H, W, "segment_egress src")
        fmt_d, dp = _planes(dst, N, H, W, "segment_egress dst")
        if fmt_d != fmt or any(t.device != logits.device for t, _, _ in sp + dp):
            raise ValueError("segment_egress: src and dst must hold the same format on the logits' device")
        pal_c = _host_u8(palette, 3 * n_cls, "palette")
        wts = np.asarray(weights)
        if wts.size != n_cls or not np.issubdtype(wts.dtype, np.integer) or wts.min() < 0 or wts.max() > 256:
            raise ValueError(f"weights: expected {n_cls} integers in 0..256")
        wt_c = (ctypes.c_uint16 * n_cls).from_buffer_copy(np.ascontiguousarray(wts, dtype=np.uint16).tobytes())
    none = (None, 0, 0)
    sp3, dp3 = (sp + [none] * 3)[:3], (dp + [none] * 3)[:3]
    plane_bytes = sum(t.shape[0] * t.shape[1] * int(np.prod(t.shape[2:])) for t, _, _ in sp + dp)
    launch("segment_egress", _lib.load().arseg_segment_egress_fwd, _ptr(logits), N, n_cls, h, w, H, W, 1 if align_corners else 0, lut_c,
           _ptr(labels_out), lab_pitch, lab_ns, fmt,
           _ptr(sp3[0][0]), _ptr(sp3[1][0]), _ptr(sp3[2][0]), sp3[0][1], sp3[1][1], sp3[2][1], sp3[0][2], sp3[1][2], sp3[2][2],
           _ptr(dp3[0][0]), _ptr(dp3[1][0]), _ptr(dp3[2][0]), dp3[0][1], dp3[1][1], dp3[2][1], dp3[0][2], dp3[1][2], dp3[2][2],
           pal_c, wt_c, _stream(), nbytes=logits.numel() * 4 + plane_bytes + (N * H * W if labels_out is not None else 0))
    return labels_out, dst


_CONF_KINDS = {"top1": _lib.CONF_TOP1, "margin": _lib.CONF_MARGIN}


def segment_confidence(logits: torch.Tensor, H: int, W: int, *, kind: str = "top1", low: int = 128, align_corners: bool = True, lut=None,
                       conf_out: Optional[torch.Tensor] = None, labels_out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None):
    """Head logits fp32 [N,n_cls,h,w] -> any non-empty subset of: the confidence plane ``conf_out`` (uint8 [N,H,W], rows contiguous, any row
    pitch / image stride; ``floor(255 c + 0.5)`` with c the softmax's top-1 probability of the resized logits, ``kind="top1"``, or its margin
    over the runner-up, ``kind="margin"``; 0 where c is NaN), the label plane ``labels_out`` (as ``segment_egress``: ``lut[k]`` or ``k``, ``k``
    = ``argmax_confusion``'s pred bit for bit) and ``stats`` (int64 [N, CONF_NSTATS], contiguous, ACCUMULATED INTO: per frame the sum of the
    codes, the number of pixels with a code below ``low`` (0..256), and the pixels per class from column 2 on), in one launch and one pass
    over the logits.  Allocates nothing: every output is the caller's, so the call can be captured in a HIP graph.
    Returns (conf_out, labels_out, stats)."""
    _need_gpu(logits)
    if logits.dim() != 4 or not logits.is_contiguous():
        raise _lib.ArsegError(f"segment_confidence expects contiguous fp32 logits [N,n_cls,h,w], got {tuple(logits.shape)}")
    N, n_cls, h, w = logits.shape
    H, W = int(H), int(W)
    if conf_out is None and labels_out is None and stats is None:
        raise ValueError("segment_confidence: nothing to write (conf_out, labels_out and stats are all None)")
    if not 1 <= n_cls <= 32:
        raise ValueError(f"segment_confidence: 1..32 classes, got {n_cls}")
    if kind not in _CONF_KINDS:
        raise ValueError(f"segment_confidence: kind is 'top1' or 'margin', got {kind!r}")
    low = int(low)
    if not 0 <= low <= 256:
        raise ValueError(f"segment_confidence: low is a code threshold in 0..256, got {low}")
    conf = _out_plane("segment_confidence", "conf_out", conf_out, N, H, W, logits.device)
    lab = _out_plane("segment_confidence", "labels_out", labels_out, N, H, W, logits.device)
    if stats is not None:
        _dense("segment_confidence", "stats", stats, torch.int64, (N, _lib.CONF_NSTATS), logits.device)
    lut_c = None if lut is None else _host_u8(lut, n_cls, "lut")
    planes = (conf_out is not None) + (labels_out is not None)
    launch("segment_confidence", _lib.load().arseg_segment_confidence_fwd, _ptr(logits), N, n_cls, h, w, H, W, 1 if align_corners else 0,
           _CONF_KINDS[kind], low, lut_c, _ptr(conf_out), conf[0], conf[1], _ptr(labels_out), lab[0], lab[1], _ptr(stats), _stream(),
           nbytes=logits.numel() * 4 + planes * N * H * W)
    return conf_out, labels_out, stats


def _tc_common(what, N, H, W, n_cls, device, ref_labels, mv_q, change_out, stats):
    """The arguments the two consistency forms share -> (ref pitch, ref image stride, change pitch, change image stride)."""
    if not 1 <= n_cls <= 32:
        raise ValueError(f"{what}: 1..32 classes, got {n_cls}")
    _need_gpu(ref_labels, dtype=torch.uint8)
    if ref_labels.dim() != 3 or tuple(ref_labels.shape[1:]) != (H, W) or ref_labels.shape[0] not in (1, N) or ref_labels.device != device:
        raise ValueError(f"ref_labels must be uint8 {(1, H, W)} (shared) or {(N, H, W)} on {device}, got {tuple(ref_labels.shape)} on "
                         f"{ref_labels.device}")
    ref_pitch, ref_ns = _plane_layout(ref_labels, (W,), f"{what} ref_labels")
    if ref_labels.shape[0] == 1 and N > 1:
        ref_ns = 0                                        # one plane for all N frames
    _mv_field(what, mv_q, N, H, W, device)
    chg = _out_plane(what, "change_out", change_out, N, H, W, device)
    if stats is not None:
        _dense(what, "stats", stats, torch.int64, (N, _lib.TC_NSTATS), device)
    return ref_pitch, ref_ns, chg[0], chg[1]


def segment_consistency(logits: torch.Tensor, ref_labels: torch.Tensor, mv_q: torch.Tensor, H: int, W: int, *, align_corners: bool = True,
                        lut=None, labels_out: Optional[torch.Tensor] = None, change_out: Optional[torch.Tensor] = None,
                        stats: Optional[torch.Tensor] = None):
    """Head logits fp32 [N,n_cls,h,w] + the reference's train-id plane(s) ``ref_labels`` (uint8 [1,H,W]: shared by the N frames, or [N,H,W];
    rows contiguous, any pitch; a value >= n_cls is void) + ``mv_q`` (int16 [N,H,W,2], contiguous: quarter pels back to the reference frame)
    -> any non-empty subset of: the label plane ``labels_out`` (as ``segment_egress``: ``lut[k]`` or ``k``, ``k`` = ``argmax_confusion``'s
    pred bit for bit), the change plane ``change_out`` (uint8 [N,H,W]: 0 where ``ref[y + round(mvy / 4), x + round(mvx / 4)] == k``, 255
    where it differs, 128 where the target is off the frame or void) and ``stats`` (int64 [N, TC_NSTATS], contiguous, ACCUMULATED INTO:
    compared, outside, void, then 32 each of cur_k, ref_k, inter_k over the compared pixels), in one launch and one pass over the logits.
    Allocates nothing: every output is the caller's, so the call can be captured in a HIP graph.
    Returns (change_out, labels_out, stats)."""
    _need_gpu(logits)
    if logits.dim() != 4 or not logits.is_contiguous():
        raise _lib.ArsegError(f"segment_consistency expects contiguous fp32 logits [N,n_cls,h,w], got {tuple(logits.shape)}")
    N, n_cls, h, w = logits.shape
    H, W = int(H), int(W)
    if labels_out is None and change_out is None and stats is None:
        raise ValueError("segment_consistency: nothing to write (labels_out, change_out and stats are all None)")
    ref_pitch, ref_ns, chg_pitch, chg_ns = _tc_common("segment_consistency", N, H, W, n_cls, logits.device, ref_labels, mv_q, change_out, stats)
    lab_pitch, lab_ns = _out_plane("segment_consistency", "labels_out", labels_out, N, H, W, logits.device)
    lut_c = None if lut is None else _host_u8(lut, n_cls, "lut")
    planes = (change_out is not None) + (labels_out is not None)
    launch("segment_consistency", _lib.load().arseg_segment_consistency_fwd, _ptr(logits), N, n_cls, h, w, H, W, 1 if align_corners else 0,
           _ptr(ref_labels), ref_pitch, ref_ns, _ptr(mv_q), lut_c, _ptr(labels_out), lab_pitch, lab_ns, _ptr(change_out), chg_pitch, chg_ns,
           _ptr(stats), _stream(), nbytes=logits.numel() * 4 + (5 + planes) * N * H * W)
    return change_out, labels_out, stats


def labels_consistency(labels: torch.Tensor, ref_labels: torch.Tensor, mv_q: torch.Tensor, n_cls: int, *,
                       change_out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None):
    """The plane form of ``segment_consistency``: ``labels`` uint8 [N,H,W] in train ids (rows contiguous, any pitch / image stride; a value
    >= n_cls is void) instead of logits; the same comparison, change plane and counters.  Returns (change_out, stats)."""
    _need_gpu(labels, dtype=torch.uint8)
    if labels.dim() != 3:
        raise _lib.ArsegError(f"labels_consistency expects a uint8 label plane [N,H,W], got {tuple(labels.shape)}")
    N, H, W = labels.shape
    n_cls = int(n_cls)
    if change_out is None and stats is None:
        raise ValueError("labels_consistency: nothing to write (change_out and stats are both None)")
    ref_pitch, ref_ns, chg_pitch, chg_ns = _tc_common("labels_consistency", N, H, W, n_cls, labels.device, ref_labels, mv_q, change_out, stats)
    in_pitch, in_ns = _plane_layout(labels, (W,), "labels_consistency labels")
    launch("labels_consistency", _lib.load().arseg_labels_consistency_fwd, _ptr(labels), in_pitch, in_ns, N, n_cls, H, W, _ptr(ref_labels),
           ref_pitch, ref_ns, _ptr(mv_q), _ptr(change_out), chg_pitch, chg_ns, _ptr(stats), _stream(),
           nbytes=(6 + (change_out is not None)) * N * H * W)
    return change_out, stats


def labels_consistency_linked(labels: torch.Tensor, ref_labels: torch.Tensor, mv_q: torch.Tensor, n_cls: int, link: torch.Tensor, link_mask: int, *,
                              change_out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                              unlinked: Optional[torch.Tensor] = None):
    """``labels_consistency`` gated by the chain's link bytes: ``link`` uint8 [N,H,W] (rows contiguous, any pitch / image stride; a frame's
    plane of ``MotionChain.link()``), ``link_mask`` 0..255 the bits that gate.  A pixel with ``link & link_mask`` is unlinked: decided first,
    ``change_out`` 128, no counter of ``stats``, one count in ``unlinked`` (int64 [N], contiguous, ACCUMULATED INTO; None: not wanted).
    ``link_mask=0`` gives ``labels_consistency``'s outputs bit for bit.  Returns (change_out, stats, unlinked)."""
    _need_gpu(labels, dtype=torch.uint8)
    if labels.dim() != 3:
        raise _lib.ArsegError(f"labels_consistency_linked expects a uint8 label plane [N,H,W], got {tuple(labels.shape)}")
    N, H, W = labels.shape
    n_cls, link_mask = int(n_cls), int(link_mask)
    if change_out is None and stats is None:
        raise ValueError("labels_consistency_linked: nothing to write (change_out and stats are both None)")
    if not 0 <= link_mask <= 255:
        raise ValueError(f"labels_consistency_linked: link_mask is a byte, got {link_mask}")
    what = "labels_consistency_linked"
    ref_pitch, ref_ns, chg_pitch, chg_ns = _tc_common(what, N, H, W, n_cls, labels.device, ref_labels, mv_q, change_out, stats)
    in_pitch, in_ns = _plane_layout(labels, (W,), f"{what} labels")
    if link is None:
        raise _lib.ArsegError(f"{what}: link is required (labels_consistency is the form without)")
    _need_gpu(link, dtype=torch.uint8)
    if tuple(link.shape) != (N, H, W) or link.device != labels.device:
        raise _lib.ArsegError(f"{what}: link must be uint8 {(N, H, W)} on {labels.device}, got {tuple(link.shape)} on {link.device}")
    link_pitch, link_ns = _plane_layout(link, (W,), f"{what} link")
    if unlinked is not None:
        _dense(what, "unlinked", unlinked, torch.int64, (N,), labels.device)
    launch(what, _lib.load().arseg_labels_consistency_linked_fwd, _ptr(labels), in_pitch, in_ns, N, n_cls, H, W, _ptr(ref_labels),
           ref_pitch, ref_ns, _ptr(mv_q), _ptr(change_out), chg_pitch, chg_ns, _ptr(stats), _ptr(link), link_pitch, link_ns, link_mask,
           _ptr(unlinked), _stream(), nbytes=(7 + (change_out is not None)) * N * H * W)
    return change_out, stats, unlinked


def segment_stabilise(logits: torch.Tensor, ref_labels: torch.Tensor, mv_q: torch.Tensor, H: int, W: int, bonus: torch.Tensor, *,
                      align_corners: bool = True, lut=None, link: Optional[torch.Tensor] = None, link_mask: int = 0,
                      ref_conf: Optional[torch.Tensor] = None, ref_low: int = 0, labels_out: Optional[torch.Tensor] = None,
                      hold_out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None):
    """The keyframe prior along the motion chain (include/arseg_hip.h, arseg_segment_stabilise_fwd): logits, ``ref_labels`` and ``mv_q`` as
    ``segment_consistency`` takes them; ``bonus`` fp32 [N] on the device, the hold threshold of each frame in logit units; ``link`` uint8
    [N,H,W] with ``link_mask`` as ``labels_consistency_linked`` takes them (None or a zero mask: no gate); ``ref_conf`` uint8 [1,H,W] or
    [N,H,W], the reference's confidence codes, with ``ref_low`` 0..256 (None or 0: no gate) -> any non-empty subset of: ``labels_out``
    (uint8 [N,H,W]: the reference's class where the pixel is HELD, ``k*`` otherwise, through ``lut``), ``hold_out`` (uint8 [N,H,W]: 0 agree,
    255 held, 192 own, 128 no prior) and ``stats`` (int64 [N, ST_NSTATS], contiguous, ACCUMULATED INTO: the seven outcome counts, a
    reserved word, then 32 each of into_k, from_k over the held pixels), in one launch and one pass over the logits.  Allocates nothing:
    every output is the caller's, so the call can be captured in a HIP graph.  Returns (labels_out, hold_out, stats)."""
    what = "segment_stabilise"
    _need_gpu(logits)
    if logits.dim() != 4 or not logits.is_contiguous():
        raise _lib.ArsegError(f"{what} expects contiguous fp32 logits [N,n_cls,h,w], got {tuple(logits.shape)}")
    N, n_cls, h, w = logits.shape
    H, W, link_mask, ref_low = int(H), int(W), int(link_mask), int(ref_low)
    dev = logits.device
    if labels_out is None and hold_out is None and stats is None:
        raise ValueError(f"{what}: nothing to write (labels_out, hold_out and stats are all None)")
    if not 0 <= link_mask <= 255:
        raise ValueError(f"{what}: link_mask is a byte, got {link_mask}")
    if not 0 <= ref_low <= 256:
        raise ValueError(f"{what}: ref_low is a code threshold in 0..256, got {ref_low}")
    ref_pitch, ref_ns, _, _ = _tc_common(what, N, H, W, n_cls, dev, ref_labels, mv_q, None, None)
    hold_pitch, hold_ns = _out_plane(what, "hold_out", hold_out, N, H, W, dev)
    lab_pitch, lab_ns = _out_plane(what, "labels_out", labels_out, N, H, W, dev)
    _dense(what, "bonus", bonus, torch.float32, (N,), dev)
    if stats is not None:
        _dense(what, "stats", stats, torch.int64, (N, _lib.ST_NSTATS), dev)
    link_pitch = link_ns = conf_pitch = conf_ns = 0
    if link is not None:
        _need_gpu(link, dtype=torch.uint8)
        if tuple(link.shape) != (N, H, W) or link.device != dev:
            raise _lib.ArsegError(f"{what}: link must be uint8 {(N, H, W)} on {dev}, got {tuple(link.shape)} on {link.device}")
        link_pitch, link_ns = _plane_layout(link, (W,), f"{what} link")
    if ref_conf is not None:
        _need_gpu(ref_conf, dtype=torch.uint8)
        if ref_conf.dim() != 3 or tuple(ref_conf.shape[1:]) != (H, W) or ref_conf.shape[0] not in (1, N) or ref_conf.device != dev:
            raise ValueError(f"ref_conf must be uint8 {(1, H, W)} (shared) or {(N, H, W)} on {dev}, got {tuple(ref_conf.shape)} on {ref_conf.device}")
        conf_pitch, conf_ns = _plane_layout(ref_conf, (W,), f"{what} ref_conf")
        if ref_conf.shape[0] == 1 and N > 1:
            conf_ns = 0                                       # one plane for all N frames
    lut_c = None if lut is None else _host_u8(lut, n_cls, "lut")
    planes = (hold_out is not None) + (labels_out is not None)
    launch(what, _lib.load().arseg_segment_stabilise_fwd, _ptr(logits), N, n_cls, h, w, H, W, 1 if align_corners else 0, _ptr(ref_labels),
           ref_pitch, ref_ns, _ptr(mv_q), _ptr(bonus), _ptr(link), link_pitch, link_ns, link_mask, _ptr(ref_conf), conf_pitch, conf_ns, ref_low,
           lut_c, _ptr(labels_out), lab_pitch, lab_ns, _ptr(hold_out), hold_pitch, hold_ns, _ptr(stats), _stream(),
           nbytes=logits.numel() * 4 + (5 + (link is not None) + (ref_conf is not None) + planes) * N * H * W)
    return labels_out, hold_out, stats


_RUN_DTYPES = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)          # one 32-bit word per run, either sign


def labels_rle(labels: torch.Tensor, row_start: torch.Tensor, runs: Optional[torch.Tensor] = None):
    """An 8-bit plane uint8 [N,H,W] (rows contiguous, any pitch / image stride; any byte values) -> its row-run code (include/arseg_hip.h,
    arseg_labels_rle_fwd): ``row_start`` int32 [N,H+1], contiguous, OVERWRITTEN with the exclusive prefix of the rows' run counts
    (``row_start[n, H]`` = the runs frame n needs, exact whatever the capacity), and ``runs`` 32-bit [N,cap], contiguous: run i of frame n in
    (y, x) order as ``(x_first << 8) | value``; words with an index >= cap are not written, nothing from ``runs[n, cap]`` on is touched.
    ``runs=None``: the sizing pass, ``row_start`` only.  Allocates nothing and synchronises nothing: capturable in a HIP graph.
    Returns (row_start, runs)."""
    _need_gpu(labels, dtype=torch.uint8)
    if labels.dim() != 3:
        raise _lib.ArsegError(f"labels_rle expects a uint8 plane [N,H,W], got {tuple(labels.shape)}")
    N, H, W = labels.shape
    _frame_dims("labels_rle", H, W, positive=False)
    _dense("labels_rle", "row_start", row_start, torch.int32, (N, H + 1), labels.device)
    cap = 0 if runs is None else _dense("labels_rle", "runs", runs, _RUN_DTYPES, (N, None), labels.device)
    pitch, ns = _plane_layout(labels, (W,), "labels_rle labels")
    launch("labels_rle", _lib.load().arseg_labels_rle_fwd, _ptr(labels), pitch, ns, N, H, W, _ptr(row_start), _ptr(runs), cap, _stream(),
           nbytes=(2 if runs is not None else 1) * N * H * W + 12 * N * (H + 1))          # (+ 4 bytes per run, known on the device only)
    return row_start, runs


def rle_decode(row_start: torch.Tensor, runs: torch.Tensor, labels_out: torch.Tensor):
    """The inverse of ``labels_rle`` (arseg_rle_decode_fwd): ``row_start`` int32 [N,H+1] and ``runs`` 32-bit [N,cap] -> ``labels_out`` uint8
    [N,H,W] (rows contiguous, any pitch / image stride).  Every pixel of a stored run is written; the pixels of runs with an index >= cap
    keep what they held (of a run whose successor in the row was cut off, the first pixel is written); nothing past a row is written.
    Allocates nothing.  Returns labels_out."""
    _need_gpu(labels_out, dtype=torch.uint8)
    if labels_out.dim() != 3:
        raise _lib.ArsegError(f"rle_decode expects a uint8 plane [N,H,W] to write into, got {tuple(labels_out.shape)}")
    N, H, W = labels_out.shape
    _frame_dims("rle_decode", H, W, positive=False)
    _dense("rle_decode", "row_start", row_start, torch.int32, (N, H + 1), labels_out.device)
    cap = _dense("rle_decode", "runs", runs, _RUN_DTYPES, (N, None), labels_out.device)
    pitch, ns = _plane_layout(labels_out, (W,), "rle_decode labels_out")
    if cap == 0:          # no run is stored (an empty tensor has no address to hand over): every pixel keeps what it held
        return labels_out
    launch("rle_decode", _lib.load().arseg_rle_decode_fwd, _ptr(row_start), _ptr(runs), cap, N, H, W, _ptr(labels_out), pitch, ns, _stream(),
           nbytes=N * H * W + 4 * N * (H + 1))
    return labels_out


def _run_side(what, side, H, row_start, runs, n_regions, run_region, dev=None):
    """A run code with its regions, the four arrays of one side (``side``: the prefix of their names) -> (frames, cap, device)."""
    N = _dense(what, side + "row_start", row_start, torch.int32, (None, H + 1), dev)
    dev = row_start.device
    cap = _dense(what, side + "runs", runs, _RUN_DTYPES, (N, None), dev)
    if cap == 0:
        raise ValueError(f"{what}: the {side}run buffer holds no run (capacity 0)")
    _dense(what, side + "n_regions", n_regions, torch.int32, (N,), dev)
    _dense(what, side + "run_region", run_region, torch.int32, (N, cap), dev)
    return N, cap, dev


def rle_regions(row_start: torch.Tensor, runs: torch.Tensor, H: int, W: int, n_regions: torch.Tensor, run_region: torch.Tensor,
                regions: Optional[torch.Tensor] = None, connectivity: int = 8, workspace: Optional[torch.Tensor] = None):
    """The connected regions of a row-run code (include/arseg_hip.h, arseg_rle_regions_fwd): ``row_start`` int32 [N,H+1] and ``runs`` 32-bit
    [N,cap] as ``labels_rle`` wrote them -> ``n_regions`` int32 [N] (R per frame, -1 for a frame whose run code overflowed), ``run_region``
    int32 [N,cap] (the region number of every stored run) and, when given, ``regions`` int64 [N,rcap,8]: per region ``value, area, x_min,
    y_min, x_max, y_max, sum_x, sum_y``, exact below ``min(R, rcap)``, untouched from there on.  Regions are numbered in the raster order of
    their first pixel.  ``connectivity`` 4 or 8.  ``workspace``: a device tensor of at least ``arseg_rle_regions_workspace_bytes(N, cap)``
    bytes (default: the stream's shared workspace).  With every buffer given nothing is allocated and nothing synchronises: capturable in a
    HIP graph.  Returns (n_regions, run_region, regions)."""
    what = "rle_regions"
    H, W = _frame_dims(what, H, W)
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity is 4 or 8, got {connectivity!r}")
    N, cap, dev = _run_side(what, "", H, row_start, runs, n_regions, run_region)
    rcap = 0 if regions is None else _dense(what, "regions", regions, torch.int64, (N, None, 8), dev)
    lib = _lib.load()
    workspace, ws_bytes = _own_workspace(what, workspace, lib.arseg_rle_regions_workspace_bytes(N, cap), dev)
    launch(what, lib.arseg_rle_regions_fwd, _ptr(row_start), _ptr(runs), cap, N, H, W, int(connectivity), _ptr(n_regions),
           _ptr(run_region), _ptr(regions if rcap else None), rcap, _ptr(workspace), ws_bytes, _stream(),
           nbytes=4 * N * (H + 1))          # (+ about 50 bytes per run, known on the device only)
    return n_regions, run_region, regions


def region_links(row_start: torch.Tensor, runs: torch.Tensor, n_regions: torch.Tensor, run_region: torch.Tensor, ref_row_start: torch.Tensor,
                 ref_runs: torch.Tensor, ref_n_regions: torch.Tensor, ref_run_region: torch.Tensor, H: int, W: int, n_pairs: torch.Tensor,
                 links: Optional[torch.Tensor] = None, back: Optional[torch.Tensor] = None, mv_q: Optional[torch.Tensor] = None,
                 pair_capacity: Optional[int] = None, workspace: Optional[torch.Tensor] = None):
    """Which region of a reference frame every region of a frame came from, along the motion (include/arseg_hip.h, arseg_region_links_fwd):
    the current frames' ``row_start`` int32 [N,H+1], ``runs`` 32-bit [N,cap], ``n_regions`` int32 [N] and ``run_region`` int32 [N,cap] as
    ``labels_rle`` + ``rle_regions`` wrote them, the reference's four alike ([1,...]: one reference shared by the N frames, or [N,...]) and
    ``mv_q`` (int16 [N,H,W,2], contiguous: quarter pels back to the reference; None: zero motion) -> ``n_pairs`` int32 [N] (the distinct
    pairs of a frame; -1: a run code overflowed or a side has no regions; -2: more than ``pair_capacity`` pairs) and, when given, ``links``
    int64 [N,rcap,6] (``ref_region, overlap, same, outside, mutual, n_ref`` per region) and ``back`` int64 [N,kcap,4] (``cur_region,
    overlap, covered, n_cur`` per reference region), exact below the region counts and untouched from there on.  ``pair_capacity``: the
    slots of the pair table (default ``4 * cap``).  ``workspace``: a device tensor of at least
    ``arseg_region_links_workspace_bytes(N, pair_capacity)`` bytes, 8-byte aligned (default: the stream's shared workspace).  With every
    buffer given nothing is allocated and nothing synchronises: capturable in a HIP graph.  Returns (n_pairs, links, back)."""
    what = "region_links"
    H, W = _frame_dims(what, H, W)
    N, cap, dev = _run_side(what, "", H, row_start, runs, n_regions, run_region)
    R, ref_cap, _ = _run_side(what, "ref_", H, ref_row_start, ref_runs, ref_n_regions, ref_run_region, dev)
    if R not in (1, N):
        raise ValueError(f"{what}: one reference frame (shared) or {N}, got {R}")
    pcap = 4 * cap if pair_capacity is None else int(pair_capacity)
    if pcap < 1:
        raise ValueError(f"{what}: pair_capacity must be at least 1, got {pair_capacity!r}")
    _dense(what, "n_pairs", n_pairs, torch.int32, (N,), dev)
    rcap = 0 if links is None else _dense(what, "links", links, torch.int64, (N, None, 6), dev)
    kcap = 0 if back is None else _dense(what, "back", back, torch.int64, (N, None, 4), dev)
    if mv_q is not None:
        _mv_field(what, mv_q, N, H, W, dev)
    lib = _lib.load()
    workspace, ws_bytes = _own_workspace(what, workspace, lib.arseg_region_links_workspace_bytes(N, pcap), dev, 8)
    launch(what, lib.arseg_region_links_fwd, _ptr(row_start), _ptr(runs), _ptr(n_regions), _ptr(run_region), cap, _ptr(ref_row_start),
           _ptr(ref_runs), _ptr(ref_n_regions), _ptr(ref_run_region), ref_cap, 1 if R == 1 else 0, _ptr(mv_q), N, H, W, _ptr(n_pairs),
           _ptr(links if rcap else None), rcap, _ptr(back if kcap else None), kcap, pcap, _ptr(workspace), ws_bytes, _stream(),
           nbytes=(4 * N * H * W if mv_q is not None else 0) + 64 * N * pcap)          # the field once from HBM; the tables cleared and read
    return n_pairs, links, back


def protect_table(protect, what="protect"):
    """The protected values of ``rle_absorb`` -- any collection of integers 0..255, or a table of 256 boolean flags -> the 256 flags."""
    flags = np.asarray(sorted(protect) if isinstance(protect, (set, frozenset)) else protect)
    if flags.dtype == np.bool_ and flags.shape == (256,):
        return flags.copy()
    values = flags.reshape(-1)
    if values.size and (not np.issubdtype(values.dtype, np.integer) or values.min() < 0 or values.max() > 255):
        raise ValueError(f"{what}: protect holds values 0..255 (or 256 boolean flags), got {values.dtype} {values.shape}")
    table = np.zeros(256, dtype=bool)
    table[values.astype(np.int64)] = True
    return table


def rle_absorb(row_start: torch.Tensor, runs: torch.Tensor, n_regions: torch.Tensor, run_region: torch.Tensor, regions: torch.Tensor, H: int,
               W: int, min_area: int, out_row_start: torch.Tensor, out_runs: torch.Tensor, n_absorbed: torch.Tensor,
               target: Optional[torch.Tensor] = None, protect=None, pair_capacity: Optional[int] = None,
               workspace: Optional[torch.Tensor] = None):
    """The small regions of a row-run code absorbed into their neighbours (include/arseg_hip.h, arseg_rle_absorb_fwd): ``row_start`` int32
    [N,H+1], ``runs`` 32-bit [N,cap], ``n_regions`` int32 [N], ``run_region`` int32 [N,cap] and ``regions`` int64 [N,rcap,8] as
    ``labels_rle`` + ``rle_regions`` wrote them -> ``out_row_start`` int32 [N,H+1] and ``out_runs`` 32-bit [N,out_cap]: the run code of the
    plane in which every region below ``min_area`` pixels whose value is not in ``protect`` (host values 0..255, or a table of 256 flags) has
    taken the value of the stable neighbour it shares the longest 4-neighbour border with (ties to the smaller region number; none: it
    stays); ``n_absorbed`` int32 [N] (the regions absorbed; -1: the run code overflowed, or the regions are missing or more than rcap;
    -2: more than ``pair_capacity`` neighbour pairs; either way nothing else of the frame is touched) and, when given, ``target`` int32
    [N,tcap] (-1 stable, -2 small and left alone, else the region it went into).  ``pair_capacity``: the slots of the pair table (default
    ``3 * cap``, which cannot overflow).  ``workspace``: a device tensor of at least ``arseg_rle_absorb_workspace_bytes(N, cap, rcap, H,
    pair_capacity)`` bytes, 8-byte aligned (default: the stream's shared workspace).  With every buffer given nothing is allocated and
    nothing synchronises: capturable in a HIP graph.  Returns (out_row_start, out_runs, target, n_absorbed)."""
    what = "rle_absorb"
    H, W = _frame_dims(what, H, W)
    min_area = int(min_area)
    if min_area < 1:
        raise ValueError(f"{what}: min_area must be at least 1, got {min_area}")
    N, cap, dev = _run_side(what, "", H, row_start, runs, n_regions, run_region)
    rcap = _dense(what, "regions", regions, torch.int64, (N, None, 8), dev)
    if rcap == 0:
        raise ValueError(f"{what}: the record buffer holds no region (capacity 0)")
    _dense(what, "out_row_start", out_row_start, torch.int32, (N, H + 1), dev)
    out_cap = _dense(what, "out_runs", out_runs, _RUN_DTYPES, (N, None), dev)
    if out_cap == 0:
        raise ValueError(f"{what}: the output run buffer holds no run (capacity 0)")
    _dense(what, "n_absorbed", n_absorbed, torch.int32, (N,), dev)
    tcap = 0 if target is None else _dense(what, "target", target, torch.int32, (N, None), dev)
    protect_c = None if protect is None else _host_u8(protect_table(protect, what), 256, "protect")
    pcap = 3 * cap if pair_capacity is None else int(pair_capacity)
    if pcap < 1:
        raise ValueError(f"{what}: pair_capacity must be at least 1, got {pair_capacity!r}")
    lib = _lib.load()
    workspace, ws_bytes = _own_workspace(what, workspace, lib.arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, pcap), dev, 8)
    launch(what, lib.arseg_rle_absorb_fwd, _ptr(row_start), _ptr(runs), _ptr(n_regions), _ptr(run_region), cap, _ptr(regions), rcap, N, H, W,
           min_area, protect_c, _ptr(out_row_start), _ptr(out_runs), out_cap, _ptr(target if tcap else None), tcap, _ptr(n_absorbed), pcap,
           _ptr(workspace), ws_bytes, _stream(),
           nbytes=32 * N * pcap + 12 * N * (H + 1))          # the table cleared and read (+ about 40 bytes per run, known on the device only)
    return out_row_start, out_runs, target, n_absorbed


def rle_contours(row_start: torch.Tensor, runs: torch.Tensor, n_regions: torch.Tensor, run_region: torch.Tensor, H: int, W: int,
                 counts: torch.Tensor, loops: Optional[torch.Tensor] = None, verts: Optional[torch.Tensor] = None, connectivity: int = 8,
                 workspace: Optional[torch.Tensor] = None):
    """The outlines of the regions of a row-run code as closed polygon loops (include/arseg_hip.h, arseg_rle_contours_fwd): ``row_start``
    int32 [N,H+1], ``runs`` 32-bit [N,cap], ``n_regions`` int32 [N] and ``run_region`` int32 [N,cap] as ``labels_rle`` + ``rle_regions``
    wrote them, ``connectivity`` the value the regions were labelled with -> ``counts`` int32 [N,2] (the loops and vertices of each frame,
    exact whatever the capacities; -1, -1: the run code overflowed or the regions are missing, nothing else of the frame is touched) and,
    when given, ``loops`` int32 [N,lcap,4] (``region, first, count, hole`` per loop) and ``verts`` 32-bit [N,vcap] (the corners, ``y << 16 |
    x``), exact below the counts and untouched from there on.  ``lcap = cap`` and ``vcap = 4 * cap`` cannot overflow.  ``workspace``: a
    device tensor of at least ``arseg_rle_contours_workspace_bytes(N, cap)`` bytes (default: the stream's shared workspace).  With every
    buffer given nothing is allocated and nothing synchronises: capturable in a HIP graph.  Returns (counts, loops, verts)."""
    what = "rle_contours"
    H, W = _frame_dims(what, H, W, 65535)          # a vertex is y << 16 | x
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity is 4 or 8, got {connectivity!r}")
    N, cap, dev = _run_side(what, "", H, row_start, runs, n_regions, run_region)
    if cap > 1 << 29:
        raise ValueError(f"{what}: at most 2^29 runs per frame, got a capacity of {cap}")
    _dense(what, "counts", counts, torch.int32, (N, 2), dev)
    lcap = 0 if loops is None else _dense(what, "loops", loops, torch.int32, (N, None, 4), dev)
    vcap = 0 if verts is None else _dense(what, "verts", verts, _RUN_DTYPES, (N, None), dev)
    lib = _lib.load()
    workspace, ws_bytes = _own_workspace(what, workspace, lib.arseg_rle_contours_workspace_bytes(N, cap), dev, 4)
    launch(what, lib.arseg_rle_contours_fwd, _ptr(row_start), _ptr(runs), _ptr(n_regions), _ptr(run_region), cap, N, H, W, int(connectivity),
           _ptr(counts), _ptr(loops if lcap else None), lcap, _ptr(verts if vcap else None), vcap, _ptr(workspace), ws_bytes, _stream(),
           nbytes=4 * N * (H + 1))          # (+ about 80 bytes per run and round of jumping, known on the device only)
    return counts, loops, verts


def tolerance_q(tolerance, what="contours_simplify"):
    """A tolerance in pixels, a non-negative multiple of 0.25 -> ``tol2_q``: sixteen times its square (an integer)."""
    quarters = float(tolerance) * 4.0
    if not (0.0 <= quarters <= 32768.0) or quarters != int(quarters):          # 32768 quarters: tol2_q = 1 << 30, the entry point's limit
        raise ValueError(f"{what}: tolerance must be a non-negative multiple of 0.25 pixels (at most 8192), got {tolerance!r}")
    return int(quarters) ** 2


def contours_simplify(counts: torch.Tensor, loops: Optional[torch.Tensor], verts: Optional[torch.Tensor], H: int, W: int, tolerance,
                      counts_out: torch.Tensor, loops_out: Optional[torch.Tensor] = None, verts_out: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None):
    """Region outlines simplified to ``tolerance`` pixels (include/arseg_hip.h, arseg_contours_simplify_fwd): ``counts`` int32 [N,2],
    ``loops`` int32 [N,lcap,4] and ``verts`` 32-bit [N,vcap] as ``rle_contours`` wrote them -> ``counts_out`` int32 [N,2] (the loops and
    the kept vertices of each frame, exact whatever the capacity; -1, -1: the source frame was refused or overflowed, nothing else of the
    frame is touched), ``loops_out`` int32 [N,lcap,4] (``region, first', count', hole``; required with loops) and, when given,
    ``verts_out`` 32-bit [N,vcap_out], exact below the counts and untouched from there on.  ``tolerance``: a non-negative multiple of
    0.25.  Per loop Douglas-Peucker on the two chains between its first vertex and the vertex farthest from it; a loop that would keep
    fewer than 3 vertices is left whole.  ``workspace``: a device tensor of at least ``arseg_contours_simplify_workspace_bytes(N, lcap,
    vcap)`` bytes (default: the stream's shared workspace).  With every buffer given nothing is allocated and nothing synchronises:
    capturable in a HIP graph.  Returns (counts_out, loops_out, verts_out)."""
    what = "contours_simplify"
    H, W = _frame_dims(what, H, W, 16384)
    tol2_q = tolerance_q(tolerance, what)
    N = _dense(what, "counts", counts, torch.int32, (None, 2))
    dev = counts.device
    if N < 1:
        raise _lib.ArsegError(f"{what}: counts must hold at least one frame, got {tuple(counts.shape)}")
    _dense(what, "counts_out", counts_out, torch.int32, (N, 2), dev)
    lcap = 0
    if loops is not None:
        lcap = _dense(what, "loops", loops, torch.int32, (N, None, 4), dev)
        if loops_out is None:
            raise _lib.ArsegError(f"{what}: loops_out is required with loops")
        _dense(what, "loops_out", loops_out, torch.int32, (N, lcap, 4), dev)
    vcap = 0 if verts is None else _dense(what, "verts", verts, _RUN_DTYPES, (N, None), dev)
    vcap_out = 0 if verts_out is None else _dense(what, "verts_out", verts_out, _RUN_DTYPES, (N, None), dev)
    lib = _lib.load()
    nbytes = lib.arseg_contours_simplify_workspace_bytes(N, lcap, vcap)
    workspace, ws_bytes = _own_workspace(what, workspace, max(nbytes, 16) if workspace is None else nbytes, dev, 4)
    launch(what, lib.arseg_contours_simplify_fwd, _ptr(counts), _ptr(loops if lcap else None), lcap, _ptr(verts if vcap else None), vcap, N, H, W,
           tol2_q, _ptr(counts_out), _ptr(loops_out if lcap else None), _ptr(verts_out if vcap_out else None), vcap_out, _ptr(workspace),
           ws_bytes, _stream(),
           nbytes=16 * N)          # (+ about 16 bytes per loop and some 30 per vertex, known on the device only)
    return counts_out, loops_out, verts_out


def contours_simplify_shared(row_start: torch.Tensor, runs: torch.Tensor, counts: torch.Tensor, loops: Optional[torch.Tensor],
                             verts: Optional[torch.Tensor], H: int, W: int, tolerance, counts_out: torch.Tensor,
                             loops_out: Optional[torch.Tensor] = None, verts_out: Optional[torch.Tensor] = None,
                             workspace: Optional[torch.Tensor] = None):
    """Region outlines simplified to ``tolerance`` pixels with shared borders (include/arseg_hip.h, arseg_contours_simplify_shared_fwd):
    ``row_start`` int32 [N,H+1] and ``runs`` 32-bit [N,cap] (the run code the outlines were traced from), ``counts`` int32 [N,2], ``loops``
    int32 [N,lcap,4] and ``verts`` 32-bit [N,vcap] as ``rle_contours`` wrote them -> ``counts_out`` int32 [N,2] (the loops and the kept
    vertices of each frame, exact whatever the capacity; -1, -1: the source frame was refused or overflowed, or its run code overflowed,
    nothing else of the frame is touched), ``loops_out`` int32 [N,lcap,4] (``region, first', count', hole``; required with loops) and,
    when given, ``verts_out`` 32-bit [N,vcap_out], exact below the counts and untouched from there on; ``vcap_out = vcap + 2 * cap``
    cannot overflow.  ``tolerance``: a non-negative multiple of 0.25.  The loops are cut at every junction of three or more regions (and
    at the frame's corners) and every arc is simplified by a rule that is the same in both directions of travel, so neighbours keep the
    same vertices of their common border.  ``workspace``: a device tensor of at least
    ``arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap)`` bytes (default: the stream's shared workspace).  With every
    buffer given nothing is allocated and nothing synchronises: capturable in a HIP graph.  Returns (counts_out, loops_out, verts_out)."""
    what = "contours_simplify_shared"
    H, W = _frame_dims(what, H, W, 16384)
    tol2_q = tolerance_q(tolerance, what)
    N = _dense(what, "row_start", row_start, torch.int32, (None, H + 1))
    dev = row_start.device
    cap = _dense(what, "runs", runs, _RUN_DTYPES, (N, None), dev)
    if cap == 0 or cap > 1 << 29:
        raise ValueError(f"{what}: between 1 and 2^29 runs per frame, got a capacity of {cap}")
    _dense(what, "counts", counts, torch.int32, (N, 2), dev)
    _dense(what, "counts_out", counts_out, torch.int32, (N, 2), dev)
    lcap = 0
    if loops is not None:
        lcap = _dense(what, "loops", loops, torch.int32, (N, None, 4), dev)
        if loops_out is None:
            raise _lib.ArsegError(f"{what}: loops_out is required with loops")
        _dense(what, "loops_out", loops_out, torch.int32, (N, lcap, 4), dev)
    vcap = 0 if verts is None else _dense(what, "verts", verts, _RUN_DTYPES, (N, None), dev)
    vcap_out = 0 if verts_out is None else _dense(what, "verts_out", verts_out, _RUN_DTYPES, (N, None), dev)
    lib = _lib.load()
    workspace, ws_bytes = _own_workspace(what, workspace, lib.arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap), dev, 4)
    launch(what, lib.arseg_contours_simplify_shared_fwd, _ptr(row_start), _ptr(runs), cap, _ptr(counts), _ptr(loops if lcap else None), lcap,
           _ptr(verts if vcap else None), vcap, N, H, W, tol2_q, _ptr(counts_out), _ptr(loops_out if lcap else None),
           _ptr(verts_out if vcap_out else None), vcap_out, _ptr(workspace), ws_bytes, _stream(),
           nbytes=16 * N)          # (+ about 36 bytes per loop and some 60 per vertex, known on the device only)
    return counts_out, loops_out, verts_out


def contours_fill(counts: torch.Tensor, loops: Optional[torch.Tensor], verts: Optional[torch.Tensor], n_regions: torch.Tensor,
                  records: Optional[torch.Tensor], H: int, W: int, labels_out: Optional[torch.Tensor], counts_out: torch.Tensor,
                  background: int = 255, ref_labels: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                  event_capacity: Optional[int] = None, workspace: Optional[torch.Tensor] = None):
    """Region polygons rasterised back to a label plane (include/arseg_hip.h, arseg_contours_fill_fwd): ``counts`` int32 [N,2], ``loops``
    int32 [N,lcap,4] and ``verts`` 32-bit [N,vcap] as ``rle_contours``, ``contours_simplify`` or ``contours_simplify_shared`` wrote them,
    ``n_regions`` int32 [N] and ``records`` int64 [N,rcap,8] of ``rle_regions`` (a region's value is read) -> ``labels_out`` uint8 [N,H,W]
    (rows contiguous, any pitch / image stride): every region's loops filled by the even-odd rule on the pixel centres, the larger region
    number on top, ``background`` where no region covers; ``counts_out`` int32 [N] (the edge-row crossings the frame needs, exact whatever
    the capacity; -1: the source frame was refused or overflowed, or its regions are missing or more than rcap -- nothing else of it is
    touched; above ``event_capacity``: nothing else of it is written) and, when given, ``stats`` int64 [N,FILL_NSTATS]: ``gaps, excess,
    changed`` and 256 each of ``ref_area, fill_area, both`` against ``ref_labels`` (uint8 [N,H,W], rows contiguous; None: ``changed``,
    ``ref_area`` and ``both`` stay 0).  ``event_capacity``: the crossing slots per frame; twice the run code's capacity cannot overflow
    for outlines that come from it (default: half the vertex capacity, which is that with ``rle_contours``' default of 4 vertices per
    run).  ``labels_out=None`` with ``event_capacity=0``: the sizing pass.
    ``workspace``: a device tensor of at least ``arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, event_capacity)`` bytes, 8-byte
    aligned (default: the stream's shared workspace).  With every buffer given nothing is allocated and nothing synchronises: capturable
    in a HIP graph.  Returns (labels_out, counts_out, stats)."""
    what = "contours_fill"
    H, W = _frame_dims(what, H, W, 16384)
    background = int(background)
    if not 0 <= background <= 255:
        raise ValueError(f"{what}: background is a byte, got {background}")
    if event_capacity is not None and int(event_capacity) < 0:
        raise ValueError(f"{what}: event_capacity must not be negative, got {event_capacity!r}")
    if labels_out is None and (event_capacity is None or int(event_capacity) > 0):
        raise ValueError(f"{what}: labels_out is required (None with event_capacity=0 is the sizing pass)")
    N = _dense(what, "counts", counts, torch.int32, (None, 2))
    dev = counts.device
    if N < 1:
        raise _lib.ArsegError(f"{what}: counts must hold at least one frame, got {tuple(counts.shape)}")
    _dense(what, "counts_out", counts_out, torch.int32, (N,), dev)
    _dense(what, "n_regions", n_regions, torch.int32, (N,), dev)
    lcap = 0 if loops is None else _dense(what, "loops", loops, torch.int32, (N, None, 4), dev)
    vcap = 0 if verts is None else _dense(what, "verts", verts, _RUN_DTYPES, (N, None), dev)
    rcap = 0 if records is None else _dense(what, "records", records, torch.int64, (N, None, 8), dev)
    ecap = vcap // 2 if event_capacity is None else int(event_capacity)
    pitch, ns = _out_plane(what, "labels_out", labels_out, N, H, W, dev)
    ref_pitch, ref_ns = _out_plane(what, "ref_labels", ref_labels, N, H, W, dev)
    if stats is not None:
        _dense(what, "stats", stats, torch.int64, (N, _lib.FILL_NSTATS), dev)
    lib = _lib.load()
    workspace, ws_bytes = _own_workspace(what, workspace, lib.arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, ecap), dev, 8)
    launch(what, lib.arseg_contours_fill_fwd, _ptr(counts), _ptr(loops if lcap else None), lcap, _ptr(verts if vcap else None), vcap,
           _ptr(n_regions), _ptr(records if rcap else None), rcap, N, H, W, background, _ptr(ref_labels), ref_pitch, ref_ns, _ptr(labels_out),
           pitch, ns, _ptr(counts_out), _ptr(stats), ecap, _ptr(workspace), ws_bytes, _stream(),
           nbytes=(0 if labels_out is None else N * H * W) + (0 if ref_labels is None else N * H * W) + 16 * N * (H + 1))          # (+ 16 bytes per crossing)
    return labels_out, counts_out, stats
