"""What a deployed segmenter hands on, straight from the head logits (the mirror of ``ingest`` on the way out).

* ``labels8``: the 8-bit mask plane, optionally mapped from train ids to the dataset's label ids.
* ``overlay``: the frame with the classes painted over it, in the plane format the decoder delivered (``ingest.DecodedFrames``: RGB8, NV12 or
  I420) -- the input of a display or a hardware encoder.  ``out=frames`` paints in place.

* ``confidence``: how much to trust the mask -- an 8-bit plane of the softmax's top-1 probability (or its margin over the runner-up) per
  pixel, the label plane next to it and per-frame statistics (sum of the codes, uncertain pixels, pixels per class), one launch of
  ``ops.segment_confidence`` (csrc/confidence.hip) and one pass over the logits; ``DriftMonitor`` turns the statistics into "refresh the
  keyframe" reports on a stream without ground truth.
* ``consistency``: whether the mask agrees with the keyframe's mask fetched through the accumulated motion ``mv_q`` -- an 8-bit change plane
  (0 agree / 255 differ / 128 not compared), the label plane and per-frame counters (compared / outside / void, per-class areas and
  intersections), one launch of ``ops.segment_consistency`` (csrc/consistency.hip); ``consistency_of_planes`` takes label planes instead
  of logits, ``tc_table`` turns the counters into agreement and temporal-consistency mIoU, ``ConsistencyMonitor`` into refresh reports.
* ``stabilise``: the label plane with the keyframe prior applied -- a pixel whose class differs from the keyframe's class at the
  motion-compensated position keeps the keyframe's where its own margin is below a threshold and the link is trustworthy; the label plane,
  an 8-bit hold plane (0 agree / 255 held / 192 own / 128 no prior) and per-frame counters, one launch of ``ops.segment_stabilise``
  (csrc/stabilise.hip); ``hold_bonus`` decays the threshold with the keyframe distance, ``hold_table`` reads the counters.

* ``rle`` / ``rle_of_planes``: the mask as run-length codes -- per frame the rows' run offsets and one 32-bit word ``(x_first << 8) | value``
  per run, counted, scanned and compacted on the GPU (``ops.labels_rle``, csrc/rle.hip) without a host synchronisation, so a few KB per
  frame cross the host link instead of a byte per pixel; ``RleFrames.decode`` is the inverse on the GPU, ``rle_decode_numpy`` on a host.
* ``regions``: the objects of each frame -- for every connected region of one value its value, area, bounding box and centroid, labelled on the
  GPU from the run code alone (``ops.rle_regions``, csrc/regions.hip: a lock-free union-find over the runs), numbered in the raster order of
  their first pixel; ``RegionFrames.to_host`` brings the records over, ``regions_numpy`` computes the same records from a run code on a host.
* ``links``: which region of the keyframe every region of a frame came from, and how much of it, through the accumulated motion ``mv_q``
  (``ops.region_links``, csrc/links.hip: one pass over the field, the pairs counted in a hash table on the GPU); ``LinkFrames.to_host`` brings
  the links over, ``links_numpy`` computes them on a host, ``TrackIds`` turns them into ids that last over a stream.
* ``absorb``: the specks of a mask removed where it is cheap -- every region below ``min_area`` pixels takes the value of the neighbour it
  shares the longest border with, on the run code and on the GPU (``ops.rle_absorb``, csrc/absorb.hip) -> a new ``RleFrames`` for the bus,
  the overlay and the next ``regions`` / ``links``; ``absorb_numpy`` is the same pass on a host.

* ``fill``: the polygons back to a mask -- every region's loops (``contours``, ``simplify`` or ``simplify_shared``) filled on the GPU by the
  even-odd rule on the pixel centres, the larger region number on top (``ops.contours_fill``, csrc/fill.hip) -> ``FilledFrames``: the plane
  a consumer of the polygons draws, and per frame what the simplification did to the mask (``fidelity()``: uncovered and doubly covered
  pixels, changed pixels, IoU per value); ``fill_numpy`` is the same fill on a host.

``labels8`` and ``overlay`` are one launch of ``ops.segment_egress`` (csrc/egress.hip): the bilinear resize and the argmax are the evaluator tail's own, so the
labels equal ``ops.argmax_confusion``'s ``pred`` bit for bit, and neither int32 labels nor a float frame are ever written.  The painting is
integer arithmetic, written out in include/arseg_hip.h (arseg_segment_egress_fwd).  Not covered: 10-bit, 4:2:2 or 4:4:4 destinations, text,
legends or contours, the encoder itself.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ingest, ops

# Presentation colours (RGB), one per train id; any [n_cls,3] uint8 table serves.
CAMVID_PALETTE = ((135, 206, 235), (128, 0, 0), (192, 192, 128), (128, 64, 128), (0, 0, 192), (0, 160, 0), (192, 128, 128), (64, 64, 128),
                  (64, 0, 128), (255, 160, 0), (0, 128, 192), (0, 0, 0))
CITYSCAPES_PALETTE = ((120, 60, 130), (240, 40, 230), (72, 72, 72), (100, 100, 160), (190, 150, 150), (150, 150, 150), (255, 170, 30),
                      (220, 220, 0), (100, 140, 40), (150, 250, 150), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 140), (0, 0, 70),
                      (0, 60, 100), (0, 80, 100), (0, 0, 230), (120, 10, 30))

_MATRIX = {enum: key for key, enum in ingest._COLOUR.items()}          # enum arseg_colour -> ("bt601" | "bt709", full_range)


class Palette(object):
    """Colours and blend weights of an overlay: ``colours_u8`` [n_cls,3] RGB, ``alpha`` one float or n_cls floats in 0..1 (0 leaves the frame,
    1 replaces it).  The kernel's weights are ``a_k = clip(rint(alpha_k * 256), 0, 256)``."""

    def __init__(self, colours_u8, alpha=0.5):
        c = np.asarray(colours_u8)
        if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1 or not np.issubdtype(c.dtype, np.integer) or c.min() < 0 or c.max() > 255:
            raise ValueError(f"Palette: colours must be [n_cls,3] integers in 0..255, got {c.dtype} {c.shape}")
        self.colours = np.ascontiguousarray(c.astype(np.uint8))
        a = np.asarray(alpha, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(len(self.colours), float(a))
        if a.shape != (len(self.colours),) or np.isnan(a).any():
            raise ValueError(f"Palette: alpha must be one float or {len(self.colours)} floats, got shape {a.shape}")
        self.weights = np.clip(np.rint(a * 256.0), 0, 256).astype(np.uint16)

    def __len__(self):
        return len(self.colours)

    def codes(self, src_format, colour=_lib.COLOUR_BT709_LIMITED) -> np.ndarray:
        """The [n_cls,3] uint8 table in the destination's codes: RGB8 -> the colours; NV12 / I420 -> (Y, Cb, Cr) of each colour under the
        frame's ``colour`` enum, by ``ingest.rgb_to_nv12``'s arithmetic (a 2x2 image of one colour: the box average of equal values)."""
        if src_format == _lib.SRC_RGB8:
            return self.colours.copy()
        if src_format not in (_lib.SRC_NV12, _lib.SRC_I420):
            raise ValueError(f"Palette.codes: RGB8, NV12 or I420 destinations only (10-bit formats are not covered), got format {src_format!r}")
        if colour not in _MATRIX:
            raise ValueError(f"Palette.codes: unknown colour enum {colour!r}")
        matrix, full = _MATRIX[colour]
        y, uv = ingest.rgb_to_nv12(np.broadcast_to(self.colours[:, None, None, :], (len(self.colours), 2, 2, 3)), matrix, full)
        return np.ascontiguousarray(np.concatenate([y[:, :1, 0], uv[:, 0, 0, :]], axis=1))


def _check_logits(logits):
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise ValueError("expected head logits as an fp32 tensor [N,n_cls,h,w]")
    return logits.contiguous()


def _plane_if_true(x, N, H, W, device):
    """True -> a fresh uint8 [N,H,W] plane on ``device``; the caller's buffer or None stays what it is."""
    return torch.empty((N, int(H), int(W)), dtype=torch.uint8, device=device) if x is True else x


def labels8(logits, H, W, lut=None, out=None, align_corners=True) -> torch.Tensor:
    """Head logits [N,n_cls,h,w] -> uint8 labels [N,H,W]: ``ops.argmax_confusion``'s pred (same resize, same argmax), as bytes, through
    ``lut`` (n_cls integers 0..255, e.g. train id -> label id; a list or an array) when given.  ``out``: the caller's buffer (nothing is allocated then)."""
    logits = _check_logits(logits)
    if out is None:
        out = torch.empty((logits.shape[0], int(H), int(W)), dtype=torch.uint8, device=logits.device)
    ops.segment_egress(logits, H, W, align_corners=align_corners, lut=lut, labels_out=out)
    return out


def overlay(logits, frames, palette, out=None, labels_out=None, lut=None, align_corners=True):
    """Head logits [N,n_cls,h,w] + the decoder's frames -> (the painted frames, labels8 | None), one launch.  ``frames``: an 8-bit
    ``ingest.DecodedFrames`` (RGB8, NV12, I420); the labels have its H x W.  The result has the format, colour, mean and std of ``frames``;
    ``out``: a DecodedFrames of the same format and size to write into (``out=frames`` paints in place), default freshly allocated.
    ``labels_out``: a uint8 [N,H,W] buffer, or True to have one allocated; None = no label plane."""
    if not isinstance(frames, ingest.DecodedFrames):
        raise ValueError(f"overlay paints over ingest.DecodedFrames (8-bit RGB8 / NV12 / I420), got {type(frames).__name__}")
    if frames.src_format not in (_lib.SRC_RGB8, _lib.SRC_NV12, _lib.SRC_I420):
        raise ValueError("overlay: 10-bit sources (P010, I010) are not covered; RGB8, NV12 and I420 are")
    if not isinstance(palette, Palette):
        palette = Palette(palette)
    logits = _check_logits(logits)
    n_cls = logits.shape[1]
    if len(palette) < n_cls:
        raise ValueError(f"overlay: the palette holds {len(palette)} colours, the logits {n_cls} classes")
    if out is None:
        out = frames._with([torch.empty(p.shape, dtype=p.dtype, device=p.device) for p in frames.planes])
    elif not isinstance(out, ingest.DecodedFrames) or out.src_format != frames.src_format or out.shape != frames.shape:
        raise ValueError("overlay: out must be DecodedFrames of the source's format and size")
    labels_out = _plane_if_true(labels_out, frames.N, frames.H, frames.W, logits.device)
    ops.segment_egress(logits, frames.H, frames.W, align_corners=align_corners, lut=lut, labels_out=labels_out, src=frames, dst=out,
                       palette=palette.codes(frames.src_format, frames.colour)[:n_cls], weights=palette.weights[:n_cls])
    if out is not frames and (out.colour, out.mean, out.std) != (frames.colour, frames.mean, frames.std):
        out = frames._with(out.planes)
    return out, labels_out


def confidence(logits, H, W, kind="top1", low=128, out=None, labels_out=None, lut=None, stats=None, align_corners=True):
    """Head logits [N,n_cls,h,w] -> (conf8 uint8 [N,H,W], labels8 | None, stats | None), one launch and one pass over the logits.

    ``conf8`` = ``floor(255 c + 0.5)`` per output pixel, c from the fp32 softmax over the classes of the resized logits (the resize and the
    class k* are ``ops.argmax_confusion``'s): ``kind="top1"`` the probability of k*, ``kind="margin"`` that minus the runner-up's; 0 where c
    is NaN (a NaN logit, a +inf maximum, all classes -inf).  Log-probability outputs give the same codes (softmax of a log-softmax).
    ``out``: the caller's plane (default freshly allocated).  ``labels_out``: a uint8 [N,H,W] buffer, or True to have one allocated; None =
    no label plane; values as ``labels8`` (through ``lut`` when given).  ``stats``: an int64 [N, _lib.CONF_NSTATS] tensor to accumulate
    into, or True for a zeroed one; None = no statistics.  Row n: [0] += sum of the frame's codes, [1] += pixels with a code below ``low``
    (0..256), [2 + k] += pixels of class k (not mapped through ``lut``) -- integers, so two runs are bit-equal; ``DriftMonitor`` reads rows
    of it.  Everything is included in the one launch; with ``out``, ``labels_out`` and ``stats`` given nothing is allocated."""
    logits = _check_logits(logits)
    N = logits.shape[0]
    out = _plane_if_true(True if out is None else out, N, H, W, logits.device)
    labels_out = _plane_if_true(labels_out, N, H, W, logits.device)
    if stats is True:
        stats = torch.zeros((N, _lib.CONF_NSTATS), dtype=torch.int64, device=logits.device)
    ops.segment_confidence(logits, H, W, kind=kind, low=low, align_corners=align_corners, lut=lut, conf_out=out, labels_out=labels_out, stats=stats)
    return out, labels_out, stats


class DriftMonitor(object):
    """Reports when a stream's confidence says the keyframe should be refreshed early (after a scene cut, or when the motion chain has
    drifted).  Pure Python on rows of ``confidence``'s ``stats`` (a tensor row, an array or a list: [sum of codes, low pixels, ...]); it only
    reports -- acting on the report (the keyframe schedule) is the caller's.

    ``rel_drop``: report when a frame's mean code has fallen below ``rel_drop`` x the mean code of the last keyframe (0 < rel_drop <= 1).
    ``low_share``: report when more than this share of the frame's pixels has a code below the ``low`` the statistics were taken with
    (0 <= low_share <= 1).  Both are required: neither has a value that is right for every network, dataset and ``kind``; they are the
    caller's to calibrate on its own streams (e.g. against ``EvalByDistance``'s table where labels exist)."""

    def __init__(self, rel_drop, low_share):
        self.rel_drop, self.low_share = float(rel_drop), float(low_share)
        if not 0.0 < self.rel_drop <= 1.0 or not 0.0 <= self.low_share <= 1.0:
            raise ValueError(f"DriftMonitor: rel_drop in (0, 1] and low_share in [0, 1], got {rel_drop!r}, {low_share!r}")
        self.key_mean = None          # mean code of the last keyframe

    def update(self, stats_row, n_pixels, is_keyframe) -> bool:
        """One frame: ``stats_row`` its row of statistics, ``n_pixels`` = H x W.  A keyframe resets the baseline first (and is itself only
        held to ``low_share``).  True = refresh the keyframe.  Before the first keyframe only ``low_share`` is applied."""
        n_pixels = int(n_pixels)
        if n_pixels <= 0:
            raise ValueError(f"DriftMonitor.update: n_pixels must be positive, got {n_pixels}")
        total, low = int(stats_row[0]), int(stats_row[1])
        mean = total / n_pixels
        if is_keyframe:
            self.key_mean = mean
        dropped = self.key_mean is not None and mean < self.rel_drop * self.key_mean
        return bool(dropped or low / n_pixels > self.low_share)


def _ref_planes(ref_labels, N):
    """[H,W] | [1,H,W] (one plane shared by the N frames) | [N,H,W] -> a 3-d uint8 tensor."""
    if not torch.is_tensor(ref_labels) or ref_labels.dim() not in (2, 3):
        raise ValueError("expected the reference's train-id plane as a uint8 tensor [H,W], [1,H,W] or [N,H,W]")
    return ref_labels[None] if ref_labels.dim() == 2 else ref_labels


def consistency(logits, ref_labels, mv_q, H, W, change_out=None, labels_out=None, lut=None, stats=True, align_corners=True):
    """Head logits [N,n_cls,h,w] + a reference mask + the motion back to it -> (change8 | None, labels8 | None, stats | None), one launch and
    one pass over the logits (``ops.segment_consistency``, csrc/consistency.hip).

    ``ref_labels``: uint8 TRAIN IDS (not mapped through ``lut``), [H,W] or [1,H,W] (one plane shared by the N frames: the GOP's keyframe,
    ``labels8(forward_keyframe(...)[0], H, W)``) or [N,H,W]; a value >= n_cls is void.  ``mv_q``: int16 [N,H,W,2], quarter pels accumulated
    back to the reference frame (``ingest.MotionChain.mv_q()``, ``ops.merge_motion``).  Pixel (x, y) with class k* (``ops.argmax_confusion``'s
    pred) is compared with ``ref[y + round(mvy / 4), x + round(mvx / 4)]`` (halves to even, no clamp): ``change8`` is 0 where they agree, 255
    where they differ, 128 where the target lies off the frame or either side is void.
    ``change_out`` / ``labels_out``: a uint8 [N,H,W] buffer, or True to have one allocated; None = not wanted; labels as ``labels8``
    (through ``lut`` when given).  ``stats``: an int64 [N, _lib.TC_NSTATS] tensor to accumulate into, or True for a zeroed one; None = no
    statistics.  Row n: [0] += compared pixels, [1] += outside, [2] += void, [3 + k] / [35 + k] / [67 + k] += compared pixels of class k in
    the frame / in the reference / in both -- integers, so two runs are bit-equal; ``tc_table`` and ``ConsistencyMonitor`` read rows of it."""
    logits = _check_logits(logits)
    N = logits.shape[0]
    ref_labels = _ref_planes(ref_labels, N)
    change_out = _plane_if_true(change_out, N, H, W, logits.device)
    labels_out = _plane_if_true(labels_out, N, H, W, logits.device)
    if stats is True:
        stats = torch.zeros((N, _lib.TC_NSTATS), dtype=torch.int64, device=logits.device)
    ops.segment_consistency(logits, ref_labels, mv_q, H, W, align_corners=align_corners, lut=lut, labels_out=labels_out, change_out=change_out,
                            stats=stats)
    return change_out, labels_out, stats


def consistency_of_planes(labels, ref_labels, mv_q, n_cls, change_out=None, stats=True, link=None,
                          link_mask=_lib.LINK_INTRA | _lib.LINK_UNCOVERED, unlinked=None):
    """The plane form of ``consistency``: ``labels`` uint8 [N,H,W] in train ids (e.g. earlier ``labels8`` planes; a value >= n_cls is void)
    instead of logits -> (change8 | None, stats | None), one launch of ``ops.labels_consistency``.  With ``ref_labels`` [N,H,W] and a
    per-frame field it serves consecutive-frame consistency.

    ``link`` (uint8 [N,H,W]: the frames' planes of ``ingest.MotionChain(track_links=True).link()``) gates the comparison: a pixel whose link
    byte has a bit of ``link_mask`` (default: an intra block or an uncovered pixel somewhere along its chain, i.e. ``mv_q`` does not lead to
    its counterpart) is *unlinked* -- change8 128, in no counter of ``stats``, counted per frame in ``unlinked`` (an int64 [N] tensor to
    accumulate into, True for a zeroed one, None = not wanted) -- so that disocclusion does not read as drift.  One launch of
    ``ops.labels_consistency_linked``; returns (change8 | None, stats | None, unlinked | None).  ``link=None``: the path and the results
    above, ``link_mask`` and ``unlinked`` unused."""
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise ValueError("expected the label planes as a uint8 tensor [N,H,W]")
    N, H, W = labels.shape
    ref_labels = _ref_planes(ref_labels, N)
    change_out = _plane_if_true(change_out, N, H, W, labels.device)
    if stats is True:
        stats = torch.zeros((N, _lib.TC_NSTATS), dtype=torch.int64, device=labels.device)
    if link is None:
        ops.labels_consistency(labels, ref_labels, mv_q, n_cls, change_out=change_out, stats=stats)
        return change_out, stats
    if unlinked is True:
        unlinked = torch.zeros((N,), dtype=torch.int64, device=labels.device)
    ops.labels_consistency_linked(labels, ref_labels, mv_q, n_cls, link, link_mask, change_out=change_out, stats=stats, unlinked=unlinked)
    return change_out, stats, unlinked


def tc_table(stats, n_cls):
    """Rows of ``consistency``'s statistics (a tensor, an array or lists, [N, _lib.TC_NSTATS]) -> {"agreement": [N], "tc_miou": [N],
    "compared_share": [N]} as float64 numpy arrays.  agreement = sum_k inter_k / compared; tc_miou = the mean over the classes with a
    non-zero union of inter_k / (cur_k + ref_k - inter_k); compared_share = compared / (compared + outside + void).  A frame with
    compared == 0 yields NaN for agreement and tc_miou (and a compared_share of 0; NaN there only for a row that counted no pixel)."""
    s = np.asarray(stats.cpu() if torch.is_tensor(stats) else stats, dtype=np.int64)
    if s.ndim == 1:
        s = s[None]
    n_cls = int(n_cls)
    if s.ndim != 2 or s.shape[1] != _lib.TC_NSTATS or not 1 <= n_cls <= 32:
        raise ValueError(f"tc_table: expected rows of {_lib.TC_NSTATS} counters and 1..32 classes, got {s.shape}, {n_cls}")
    compared, total = s[:, 0].astype(np.float64), s[:, :3].sum(axis=1).astype(np.float64)
    cur, ref, inter = (s[:, o:o + n_cls].astype(np.float64) for o in (3, 35, 67))
    union = cur + ref - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        agreement = np.where(compared > 0, inter.sum(axis=1) / compared, np.nan)
        iou = np.where(union > 0, inter / union, np.nan)
        seen = (union > 0).sum(axis=1)
        tc = np.where(seen > 0, np.nansum(iou, axis=1) / np.maximum(seen, 1), np.nan)
        share = np.where(total > 0, compared / total, np.nan)
    return {"agreement": agreement, "tc_miou": tc, "compared_share": share}


class ConsistencyMonitor(object):
    """Reports when a frame's mask no longer agrees with the keyframe's mask along the motion chain -- the label-free signal that stays
    informative when the softmax is sharp but wrong (a drifted chain, a scene cut inside a GOP); the sibling of ``DriftMonitor``.  Pure
    Python on rows of ``consistency``'s ``stats``; it only reports -- acting on the report (the keyframe schedule) is the caller's.

    ``min_agreement``: report when the agreement rate sum_k inter_k / compared falls below it (0 <= min_agreement <= 1).
    ``min_compared_share``: report when less than this share of the frame's pixels could be compared at all (the targets lie off the frame
    or on void: the chain has left the picture; 0 <= min_compared_share <= 1).  Both are required: neither has a value that is right for
    every network, dataset and motion source; they are the caller's to calibrate on its own streams (e.g. against ``EvalByDistance``'s
    table where labels exist)."""

    def __init__(self, min_agreement, min_compared_share):
        self.min_agreement, self.min_compared_share = float(min_agreement), float(min_compared_share)
        if not 0.0 <= self.min_agreement <= 1.0 or not 0.0 <= self.min_compared_share <= 1.0:
            raise ValueError(f"ConsistencyMonitor: both thresholds in [0, 1], got {min_agreement!r}, {min_compared_share!r}")

    def update(self, stats_row, n_pixels) -> bool:
        """One non-keyframe: ``stats_row`` its row of statistics, ``n_pixels`` = H x W.  True = refresh the keyframe.  A frame of which
        nothing could be compared is reported whenever ``min_compared_share`` > 0, and never for its (undefined) agreement."""
        n_pixels = int(n_pixels)
        if n_pixels <= 0:
            raise ValueError(f"ConsistencyMonitor.update: n_pixels must be positive, got {n_pixels}")
        compared = int(stats_row[0])
        agree = sum(int(stats_row[67 + k]) for k in range(32))
        too_little = compared / n_pixels < self.min_compared_share
        disagrees = compared > 0 and agree / compared < self.min_agreement
        return bool(too_little or disagrees)


HOLD_OUTCOMES = ("unlinked", "outside", "void", "weak", "agree", "held", "own")          # the order of the contract and of the counters


def stabilise(logits, ref_labels, mv_q, H, W, bonus, link=None, link_mask=_lib.LINK_INTRA | _lib.LINK_UNCOVERED, ref_conf=None, ref_low=0,
              labels_out=True, hold_out=None, stats=True, lut=None, align_corners=True):
    """Head logits [N,n_cls,h,w] + the keyframe's mask + the motion back to it -> (labels8 | None, hold8 | None, stats | None): the labels of
    ``labels8`` with the keyframe prior applied, one launch and one pass over the logits (``ops.segment_stabilise``, csrc/stabilise.hip).

    ``ref_labels`` and ``mv_q`` as ``consistency`` takes them.  A pixel whose own class k* differs from the class ``c_ref`` the keyframe had
    at ``(y + round(mvy / 4), x + round(mvx / 4))`` keeps ``c_ref`` where its decision is marginal: where ``v[k*] - v[c_ref] < bonus`` on the
    resized logits (strict, fp32; false for a NaN).  ``bonus``: the hold threshold in logit units, one float for all frames or an fp32 [N]
    tensor on the device (``hold_bonus`` makes one per keyframe distance); 0 or less holds nothing, and the labels are ``labels8``'s.
    No prior is offered where the target lies off the frame, where the keyframe is void (>= n_cls), where ``link`` (uint8 [N,H,W], the
    planes of ``ingest.MotionChain(track_links=True).link()``) has a bit of ``link_mask``, or where ``ref_conf`` (uint8 [H,W], [1,H,W] or
    [N,H,W]: the keyframe's ``confidence`` plane) is below ``ref_low`` (0..256) at the target.
    ``labels_out`` / ``hold_out``: a uint8 [N,H,W] buffer, or True to have one allocated; None = not wanted.  ``hold8``: 0 agree, 255 held,
    192 own (differs and is kept), 128 no prior.  ``stats``: an int64 [N, _lib.ST_NSTATS] tensor to accumulate into, or True for a zeroed
    one; None = no statistics; ``hold_table`` reads its rows.  With a tensor ``bonus`` and the caller's buffers nothing is allocated and
    nothing synchronises.  The planes feed ``rle_of_planes``, ``regions``, ``links``, ``absorb``, ``contours``, overlays and
    ``consistency_of_planes`` unchanged; with the same gates the latter's agreeing count is ``agree + held`` of ``stats``."""
    logits = _check_logits(logits)
    N = logits.shape[0]
    ref_labels = _ref_planes(ref_labels, N)
    if ref_conf is not None:
        if not torch.is_tensor(ref_conf) or ref_conf.dim() not in (2, 3):
            raise ValueError("expected the reference's confidence plane as a uint8 tensor [H,W], [1,H,W] or [N,H,W]")
        ref_conf = ref_conf[None] if ref_conf.dim() == 2 else ref_conf
    if not torch.is_tensor(bonus):
        bonus = torch.full((N,), float(bonus), dtype=torch.float32, device=logits.device)
    labels_out = _plane_if_true(labels_out, N, H, W, logits.device)
    hold_out = _plane_if_true(hold_out, N, H, W, logits.device)
    if stats is True:
        stats = torch.zeros((N, _lib.ST_NSTATS), dtype=torch.int64, device=logits.device)
    ops.segment_stabilise(logits, ref_labels, mv_q, H, W, bonus, align_corners=align_corners, lut=lut, link=link, link_mask=link_mask,
                          ref_conf=ref_conf, ref_low=ref_low, labels_out=labels_out, hold_out=hold_out, stats=stats)
    return labels_out, hold_out, stats


def hold_bonus(distances, bonus0, half_life, device=None) -> torch.Tensor:
    """The usual decay of the hold threshold with the distance to the keyframe: ``bonus0 * 2 ** (-d / half_life)`` per entry of
    ``distances`` (frames since the keyframe, >= 0), computed in float64 and rounded once -> an fp32 tensor of their shape (on ``device``),
    ``stabilise``'s ``bonus``.  ``bonus0`` >= 0 in logit units, ``half_life`` > 0 in frames; both finite."""
    d = np.asarray(distances, dtype=np.float64)
    bonus0, half_life = float(bonus0), float(half_life)
    if d.ndim > 1 or not np.isfinite(d).all() or (d < 0).any():
        raise ValueError(f"hold_bonus: distances must be finite and >= 0 (a number or a list), got {distances!r}")
    if not np.isfinite(bonus0) or bonus0 < 0 or not np.isfinite(half_life) or half_life <= 0:
        raise ValueError(f"hold_bonus: bonus0 >= 0 and half_life > 0, both finite, got {bonus0!r}, {half_life!r}")
    return torch.from_numpy(np.atleast_1d(bonus0 * np.exp2(-d / half_life)).astype(np.float32)).to(device if device is not None else "cpu")


def hold_table(stats, n_cls):
    """Rows of ``stabilise``'s statistics (a tensor, an array or lists, [N, _lib.ST_NSTATS]) -> {"shares": {outcome: [N]} for the seven
    ``HOLD_OUTCOMES`` (each count over the row's total), "held_of_differing": [N] = held / (held + own), "into": int64 [N, n_cls] (held
    pixels by the keyframe's class they took), "from": int64 [N, n_cls] (by the class they gave up)}; float64 numpy arrays, NaN for 0 / 0."""
    s = np.asarray(stats.cpu() if torch.is_tensor(stats) else stats, dtype=np.int64)
    if s.ndim == 1:
        s = s[None]
    n_cls = int(n_cls)
    if s.ndim != 2 or s.shape[1] != _lib.ST_NSTATS or not 1 <= n_cls <= 32:
        raise ValueError(f"hold_table: expected rows of {_lib.ST_NSTATS} counters and 1..32 classes, got {s.shape}, {n_cls}")
    counts = s[:, :7].astype(np.float64)
    total, differing = counts.sum(axis=1), counts[:, 5] + counts[:, 6]
    with np.errstate(divide="ignore", invalid="ignore"):
        shares = {name: np.where(total > 0, counts[:, i] / total, np.nan) for i, name in enumerate(HOLD_OUTCOMES)}
        held = np.where(differing > 0, counts[:, 5] / differing, np.nan)
    return {"shares": shares, "held_of_differing": held, "into": s[:, 8:8 + n_cls].copy(), "from": s[:, 40:40 + n_cls].copy()}


class RleFrames(object):
    """The row-run code of N planes of H x W (include/arseg_hip.h, arseg_labels_rle_fwd): ``row_start`` int32 [N,H+1] (the exclusive prefix of
    the rows' run counts) and ``runs`` 32-bit [N,capacity] (run i of a frame in (y, x) order: ``(x_first << 8) | value``), both on the device.
    ``labels``: the plane the runs were taken from, where ``rle`` allocated it (else None)."""

    def __init__(self, row_start, runs, H, W, labels=None):
        self.row_start, self.runs, self.H, self.W, self.labels = row_start, runs, int(H), int(W), labels
        if row_start.dim() != 2 or row_start.shape[1] != self.H + 1 or runs.dim() != 2 or runs.shape[0] != row_start.shape[0]:
            raise ValueError(f"RleFrames: row_start [N,{self.H + 1}] and runs [N,capacity], got {tuple(row_start.shape)} and {tuple(runs.shape)}")

    @property
    def N(self):
        return self.row_start.shape[0]

    @property
    def capacity(self):
        return self.runs.shape[1]

    def needed(self) -> torch.Tensor:
        """The runs each frame needs (a device view, int32 [N]): exact whatever the capacity; ``needed() > capacity`` is an overflow."""
        return self.row_start[:, self.H]

    def decode(self, out=None) -> torch.Tensor:
        """The planes back, on the GPU (``ops.rle_decode``): uint8 [N,H,W] into ``out`` (default: a zeroed plane).  The pixels of runs
        beyond the capacity keep what ``out`` held."""
        if out is None:
            out = torch.zeros((self.N, self.H, self.W), dtype=torch.uint8, device=self.runs.device)
        return ops.rle_decode(self.row_start, self.runs, out)

    def to_host(self):
        """[(row_start int32 [H+1], runs uint32 [needed])] per frame as numpy arrays, in two copies: the offsets (with the needed counts),
        then ``runs[:, :max(needed)]`` -- the bytes that cross the link follow the runs, not the capacity.  Raises ``ArsegError`` naming
        the frame, the runs it needs and the capacity when a frame has overflowed."""
        offsets = self.row_start.cpu().numpy()
        needed = offsets[:, self.H]
        for n, k in enumerate(needed):
            if k > self.capacity:
                raise _lib.ArsegError(f"RleFrames.to_host: frame {n} needs {int(k)} runs, the capacity is {self.capacity}")
        words = self.runs[:, :int(needed.max())].cpu().numpy().view(np.uint32)
        return [(offsets[n], words[n, :needed[n]]) for n in range(self.N)]


def rle_of_planes(labels, capacity, out=None) -> RleFrames:
    """uint8 planes [N,H,W] on the GPU (``labels8``, change or confidence planes, any byte values; rows contiguous, any pitch) ->
    ``RleFrames`` with room for ``capacity`` runs per frame, one call of ``ops.labels_rle``.  ``out``: an ``RleFrames`` of the same N, H, W
    to write into (nothing is allocated then; its capacity holds)."""
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise ValueError("expected the planes as a uint8 tensor [N,H,W]")
    N, H, W = labels.shape
    if out is None:
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"rle_of_planes: capacity must not be negative, got {capacity}")
        out = RleFrames(torch.empty((N, H + 1), dtype=torch.int32, device=labels.device),
                        torch.empty((N, capacity), dtype=torch.int32, device=labels.device), H, W)
    elif not isinstance(out, RleFrames) or (out.N, out.H, out.W) != (N, H, W):
        raise ValueError(f"rle_of_planes: out must be RleFrames of {N} frames of {H}x{W}")
    ops.labels_rle(labels, out.row_start, out.runs)
    return out


def rle(logits, H, W, capacity, lut=None, labels_out=None, out=None, align_corners=True) -> RleFrames:
    """Head logits [N,n_cls,h,w] -> the row-run code of their ``labels8`` plane: ``labels8`` into ``labels_out`` (default: a plane the
    returned object keeps as ``.labels``), then the encoder -- two ABI calls, nothing in between comes to the host.  With ``out`` (an
    ``RleFrames``) and ``labels_out`` given nothing is allocated and the pair can be captured in a HIP graph."""
    logits = _check_logits(logits)
    kept = labels_out is None
    plane = labels8(logits, H, W, lut=lut, out=labels_out, align_corners=align_corners)
    frames = rle_of_planes(plane, capacity, out=out)
    frames.labels = plane if kept else frames.labels
    return frames


def _parse_runs(what, row_start, runs, H, W):
    """One frame's run code, checked -> ``rs`` int64 [H+1] and, per counted run, ``x0``, ``x1`` (its columns [x0, x1)), ``val`` and ``row``,
    int64 each.  THE host-side definition of the format: a run ends where the next one of its row begins, or at W."""
    rs = np.asarray(row_start).astype(np.int64)
    words = np.asarray(runs).astype(np.int64) & 0xFFFFFFFF
    if rs.shape != (H + 1,) or rs[0] != 0 or (np.diff(rs) < 1).any() or words.ndim != 1 or len(words) < rs[H]:
        raise ValueError(f"{what}: expected row_start [{H + 1}], rising from 0 by at least one run per row, and the row_start[{H}] runs it counts")
    words = words[:rs[H]]
    x0 = words >> 8
    x1 = np.append(x0[1:], W)
    x1[rs[1:] - 1] = W                                # the last run of a row ends at W
    if (x0[rs[:-1]] != 0).any() or (x1 <= x0).any() or (x1 > W).any():
        raise ValueError(f"{what}: the runs of a row do not start at 0 and increase below W")
    return rs, x0, x1, words & 0xFF, np.repeat(np.arange(H, dtype=np.int64), np.diff(rs))


def _runs_above(row, x0, x1, W, d):
    """The pairs (u, v) of a run u and a run v of the row above that overlaps it, or with ``d`` = 1 touches it across a corner: two searches
    over the whole frame, on keys that order (row, x) globally so that a search for a column of row y - 1 cannot leave that row."""
    K = W + 2
    cur = np.flatnonzero(row > 0)
    first = np.searchsorted(row * K + x1, (row[cur] - 1) * K + x0[cur] - d, side="right")           # the first run above with b1 + d > a0
    last = np.searchsorted(row * K + x0, (row[cur] - 1) * K + x1[cur] + d, side="left") - 1          # the last run above with b0 < a1 + d
    count = last - first + 1
    return np.repeat(cur, count), np.repeat(first, count) + np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)


def rle_decode_numpy(row_start, runs, H, W) -> np.ndarray:
    """The receiving side without a GPU: one frame's ``row_start`` [H+1] and ``runs`` [>= row_start[H]] (as ``RleFrames.to_host`` returns
    them) -> the uint8 plane [H,W]."""
    H, W = int(H), int(W)
    _, x0, x1, val, _ = _parse_runs("rle_decode_numpy", row_start, runs, H, W)
    return np.repeat(val.astype(np.uint8), x1 - x0).reshape(H, W)


REGION_DTYPE = np.dtype([("value", np.int64), ("area", np.int64), ("x_min", np.int64), ("y_min", np.int64), ("x_max", np.int64),
                         ("y_max", np.int64), ("cx", np.float64), ("cy", np.float64)])


def _region_records(rows, min_area=None, values=None) -> np.ndarray:
    """int64 [R,8] rows {value, area, x_min, y_min, x_max, y_max, sum_x, sum_y} -> the structured records (centroids = sums / area),
    filtered on the host; the order (raster order of the regions' first pixels) stays."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 8)
    rec = np.empty(len(rows), dtype=REGION_DTYPE)
    for k, name in enumerate(REGION_DTYPE.names[:6]):
        rec[name] = rows[:, k]
    area = np.maximum(rows[:, 1], 1).astype(np.float64)
    rec["cx"], rec["cy"] = rows[:, 6] / area, rows[:, 7] / area
    keep = np.ones(len(rec), dtype=bool)
    if min_area is not None:
        keep &= rec["area"] >= min_area
    if values is not None:
        keep &= np.isin(rec["value"], np.asarray(list(values) if not np.isscalar(values) else [values]))
    return rec[keep]


class RegionFrames(object):
    """The connected regions of ``frames`` (an ``RleFrames``; include/arseg_hip.h, arseg_rle_regions_fwd), on the device: ``n_regions`` int32
    [N] (-1: the frame's run code overflowed), ``run_region`` int32 [N,frames.capacity] (the region number of every stored run) and
    ``records`` int64 [N,capacity,8]: ``value, area, x_min, y_min, x_max, y_max, sum_x, sum_y`` per region.  ``workspace``: the scratch tensor
    the labelling uses, kept so that a repeated call allocates nothing."""

    def __init__(self, n_regions, run_region, records, frames, connectivity=8, workspace=None):
        self.n_regions, self.run_region, self.records, self.frames = n_regions, run_region, records, frames
        self.connectivity, self.workspace = int(connectivity), workspace
        if not isinstance(frames, RleFrames):
            raise ValueError("RegionFrames: frames must be the RleFrames the regions were taken from")
        N = frames.N
        if tuple(n_regions.shape) != (N,) or tuple(run_region.shape) != (N, frames.capacity) or records.dim() != 3 or \
                records.shape[0] != N or records.shape[2] != 8:
            raise ValueError(f"RegionFrames: n_regions [{N}], run_region [{N},{frames.capacity}] and records [{N},capacity,8], got "
                             f"{tuple(n_regions.shape)}, {tuple(run_region.shape)} and {tuple(records.shape)}")

    @property
    def N(self):
        return self.frames.N

    @property
    def capacity(self):
        return self.records.shape[1]

    def needed(self) -> torch.Tensor:
        """The regions of each frame (a device view, int32 [N]): exact whatever the capacity; ``needed() > capacity`` is an overflow of the
        records, -1 an overflow of the frame's run code."""
        return self.n_regions

    def to_host(self, min_area=None, values=None):
        """Per frame a numpy structured array with the fields ``value, area, x_min, y_min, x_max, y_max, cx, cy`` (bounds inclusive, the
        centroid float64 from the integer sums), in two copies: ``n_regions``, then ``records[:, :max needed]``.  ``min_area`` and
        ``values`` (one value or several) filter on the host.  Raises ``ArsegError`` naming the frame, what it needs and the capacity when
        a frame has more regions than the capacity, or when its run code had overflowed (no regions exist for it)."""
        need = self.n_regions.cpu().numpy()
        for n, k in enumerate(need):
            if k < 0:
                raise _lib.ArsegError(f"RegionFrames.to_host: the run code of frame {n} overflowed (it needs {int(self.frames.needed()[n])} "
                                      f"runs, the capacity is {self.frames.capacity}): it has no regions")
            if k > self.capacity:
                raise _lib.ArsegError(f"RegionFrames.to_host: frame {n} needs {int(k)} regions, the capacity is {self.capacity}")
        rows = self.records[:, :int(need.max())].cpu().numpy()
        return [_region_records(rows[n, :need[n]], min_area, values) for n in range(self.N)]


def regions(frames: RleFrames, region_capacity, connectivity=8, out=None) -> RegionFrames:
    """The connected regions of run-coded frames, on the GPU: one call of ``ops.rle_regions`` -> ``RegionFrames`` with room for
    ``region_capacity`` records per frame.  ``out``: a ``RegionFrames`` of these frames' N and run capacity to write into (its capacity and
    workspace hold; nothing is allocated then, and ``labels8 -> labels_rle -> rle_regions`` can be captured in one HIP graph)."""
    if not isinstance(frames, RleFrames):
        raise ValueError("regions: expected the RleFrames of egress.rle / egress.rle_of_planes")
    if connectivity not in (4, 8):
        raise ValueError(f"regions: connectivity is 4 or 8, got {connectivity!r}")
    N, cap, dev = frames.N, frames.capacity, frames.runs.device
    if out is None:
        region_capacity = int(region_capacity)
        if region_capacity < 0:
            raise ValueError(f"regions: region_capacity must not be negative, got {region_capacity}")
        out = RegionFrames(torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N, cap), dtype=torch.int32, device=dev),
                           torch.empty((N, region_capacity, 8), dtype=torch.int64, device=dev), frames, connectivity,
                           torch.empty((N, max(cap, 1)), dtype=torch.int32, device=dev))
    elif not isinstance(out, RegionFrames) or out.N != N or out.run_region.shape[1] != cap:
        raise ValueError(f"regions: out must be RegionFrames of {N} frames with room for {cap} runs")
    else:
        out.frames, out.connectivity = frames, int(connectivity)
    ops.rle_regions(frames.row_start, frames.runs, frames.H, frames.W, out.n_regions, out.run_region,
                    out.records if out.capacity else None, connectivity=connectivity, workspace=out.workspace)
    return out


def regions_numpy(row_start, runs, H, W, connectivity=8, return_run_region=False):
    """The receiving side without a GPU, and what a CPU consumer of the run code calls: one frame's ``row_start`` [H+1] and ``runs``
    [>= row_start[H]] (as ``RleFrames.to_host`` returns them) -> the records ``RegionFrames.to_host`` gives for that frame (same order, same
    integers); with ``return_run_region`` also the region number of every run, int32 [row_start[H]].  Vectorised: the neighbours of all runs
    by two searches over the whole frame, components by minimum-label propagation with pointer jumping."""
    H, W = int(H), int(W)
    if connectivity not in (4, 8):
        raise ValueError(f"regions_numpy: connectivity is 4 or 8, got {connectivity!r}")
    _, x0, x1, val, row = _parse_runs("regions_numpy", row_start, runs, H, W)
    rows, run_region = _regions_of(x0, x1, val, row, H, W, connectivity)
    rec = _region_records(rows)
    return (rec, run_region.astype(np.int32)) if return_run_region else rec


def _regions_of(x0, x1, val, row, H, W, connectivity):
    """The parsed runs of a frame -> (the int64 [R,8] rows of its regions, the region number of every run)."""
    u, v = _runs_above(row, x0, x1, W, 1 if connectivity == 8 else 0)
    same = val[u] == val[v]
    u, v = u[same], v[same]
    lab = np.arange(len(x0), dtype=np.int64)
    while True:
        m = np.minimum(lab[u], lab[v])
        nxt = lab.copy()
        np.minimum.at(nxt, u, m)
        np.minimum.at(nxt, v, m)
        nxt = np.minimum(nxt, nxt[nxt])
        while True:
            j = nxt[nxt]
            if np.array_equal(j, nxt):
                break
            nxt = j
        if np.array_equal(nxt, lab):
            break
        lab = nxt
    roots, run_region = np.unique(lab, return_inverse=True)
    length = x1 - x0
    R = len(roots)
    rows = np.zeros((R, 8), dtype=np.int64)
    rows[:, 0] = val[roots]
    np.add.at(rows[:, 1], run_region, length)
    rows[:, 2], rows[:, 3] = W, H
    np.minimum.at(rows[:, 2], run_region, x0)
    np.minimum.at(rows[:, 3], run_region, row)
    rows[:, 4] = rows[:, 5] = -1
    np.maximum.at(rows[:, 4], run_region, x1 - 1)
    np.maximum.at(rows[:, 5], run_region, row)
    np.add.at(rows[:, 6], run_region, (x0 + x1 - 1) * length // 2)
    np.add.at(rows[:, 7], run_region, row * length)
    return rows, run_region


LINK_DTYPE = np.dtype([(name, np.int64) for name in ("ref_region", "overlap", "same", "outside", "mutual", "n_ref")])
BACK_DTYPE = np.dtype([(name, np.int64) for name in ("cur_region", "overlap", "covered", "n_cur")])


def _records_of(rows, dtype) -> np.ndarray:
    """int64 [R, fields] rows -> the structured records."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(dtype.names))
    rec = np.empty(len(rows), dtype=dtype)
    for k, name in enumerate(dtype.names):
        rec[name] = rows[:, k]
    return rec


class LinkFrames(object):
    """The links of the regions of ``cur`` (a ``RegionFrames`` of N frames) to the regions of ``ref`` (a ``RegionFrames`` of one frame, shared,
    or of N) along the motion (include/arseg_hip.h, arseg_region_links_fwd), on the device: ``n_pairs`` int32 [N] (-1: a side of the frame has
    no regions, -2: more distinct pairs than ``pair_capacity``), ``links`` int64 [N,cur.capacity,6] (``ref_region, overlap, same, outside,
    mutual, n_ref`` per region) and ``back`` int64 [N,ref.capacity,4] (``cur_region, overlap, covered, n_cur`` per reference region).
    ``workspace``: the tables the linking uses, kept so that a repeated call allocates nothing."""

    def __init__(self, n_pairs, links, back, cur, ref, pair_capacity, workspace=None):
        self.n_pairs, self.links, self.back, self.cur, self.ref = n_pairs, links, back, cur, ref
        self.pair_capacity, self.workspace = int(pair_capacity), workspace
        if not isinstance(cur, RegionFrames) or not isinstance(ref, RegionFrames):
            raise ValueError("LinkFrames: cur and ref must be the RegionFrames the links were taken from")
        N = cur.N
        if ref.N not in (1, N) or (ref.frames.H, ref.frames.W) != (cur.frames.H, cur.frames.W):
            raise ValueError(f"LinkFrames: ref must hold one frame or {N} of {cur.frames.H}x{cur.frames.W}, got {ref.N} of "
                             f"{ref.frames.H}x{ref.frames.W}")
        if tuple(n_pairs.shape) != (N,) or tuple(links.shape) != (N, cur.capacity, 6) or tuple(back.shape) != (N, ref.capacity, 4):
            raise ValueError(f"LinkFrames: n_pairs [{N}], links [{N},{cur.capacity},6] and back [{N},{ref.capacity},4], got "
                             f"{tuple(n_pairs.shape)}, {tuple(links.shape)} and {tuple(back.shape)}")
        if self.pair_capacity < 1:
            raise ValueError(f"LinkFrames: pair_capacity must be at least 1, got {pair_capacity!r}")

    @property
    def N(self):
        return self.cur.N

    def needed(self) -> torch.Tensor:
        """The distinct pairs of each frame (a device view, int32 [N]); -1: the frame could not be linked, -2: more than ``pair_capacity``."""
        return self.n_pairs

    def to_host(self):
        """Per frame ``(links, back)``: two numpy structured arrays with the fields ``ref_region, overlap, same, outside, mutual, n_ref`` (one
        row per region of the frame) and ``cur_region, overlap, covered, n_cur`` (one row per region of its reference).  ``n_pairs`` and the
        region counts come over first, then only the rows in use.  Raises ``ArsegError`` naming the frame when it could not be linked (a run
        code overflowed), when it has more pairs than ``pair_capacity``, or when a side has more regions than its capacity."""
        pairs = self.n_pairs.cpu().numpy()
        R, K = self.cur.n_regions.cpu().numpy(), self.ref.n_regions.cpu().numpy()
        K = np.broadcast_to(K, (self.N,)) if len(K) == 1 else K
        for n in range(self.N):
            if pairs[n] == -1:
                raise _lib.ArsegError(f"LinkFrames.to_host: frame {n} could not be linked: its run code or its reference's overflowed "
                                      f"(regions {int(R[n])}, reference regions {int(K[n])})")
            if pairs[n] == -2:
                raise _lib.ArsegError(f"LinkFrames.to_host: frame {n} has more distinct pairs than the pair capacity {self.pair_capacity}")
            if R[n] > self.cur.capacity:
                raise _lib.ArsegError(f"LinkFrames.to_host: frame {n} needs {int(R[n])} regions, the capacity is {self.cur.capacity}")
            if K[n] > self.ref.capacity:
                raise _lib.ArsegError(f"LinkFrames.to_host: the reference of frame {n} needs {int(K[n])} regions, the capacity is "
                                      f"{self.ref.capacity}")
        links = self.links[:, :int(R.max())].cpu().numpy()
        back = self.back[:, :int(K.max())].cpu().numpy()
        return [(_records_of(links[n, :R[n]], LINK_DTYPE), _records_of(back[n, :K[n]], BACK_DTYPE)) for n in range(self.N)]


def links(cur: RegionFrames, ref: RegionFrames, mv_q=None, pair_capacity=None, out=None) -> LinkFrames:
    """Which region of ``ref`` every region of ``cur`` came from, on the GPU: one call of ``ops.region_links`` -> ``LinkFrames``.  ``ref``: the
    ``RegionFrames`` of one frame (the GOP's keyframe, shared by the N frames) or of N frames; ``mv_q``: int16 [N,H,W,2], quarter pels
    accumulated back to the reference (``ingest.MotionChain.mv_q()``), None: zero motion.  A pixel of region r whose target
    ``(x + round(mvx / 4), y + round(mvy / 4))`` (halves to even, no clamp) lies in a reference run of the same value, of region k, counts
    into the pair (r, k).  ``pair_capacity``: the slots of the pair table, default ``4 * cur.frames.capacity``.  ``out``: a ``LinkFrames``
    of the same N and capacities to write into (its pair capacity and workspace hold; nothing is allocated then, and ``labels8 ->
    labels_rle -> rle_regions -> region_links`` can be captured in one HIP graph)."""
    if not isinstance(cur, RegionFrames) or not isinstance(ref, RegionFrames):
        raise ValueError("links: expected the RegionFrames of egress.regions for both sides")
    N, H, W, dev = cur.N, cur.frames.H, cur.frames.W, cur.frames.runs.device
    if ref.N not in (1, N) or (ref.frames.H, ref.frames.W) != (H, W):
        raise ValueError(f"links: ref must hold one frame (shared) or {N} of {H}x{W}, got {ref.N} of {ref.frames.H}x{ref.frames.W}")
    if out is None:
        pair_capacity = 4 * cur.frames.capacity if pair_capacity is None else int(pair_capacity)
        if pair_capacity < 1:
            raise ValueError(f"links: pair_capacity must be at least 1, got {pair_capacity}")
        _need = _lib.load().arseg_region_links_workspace_bytes(N, pair_capacity)
        if not cur.frames.runs.is_cuda:
            raise _lib.ArsegError("links runs on the GPU only (got CPU tensors); links_numpy is the host form")
        out = LinkFrames(torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N, cur.capacity, 6), dtype=torch.int64, device=dev),
                         torch.empty((N, ref.capacity, 4), dtype=torch.int64, device=dev), cur, ref, pair_capacity,
                         torch.empty((_need // 8,), dtype=torch.int64, device=dev))
    elif not isinstance(out, LinkFrames) or out.N != N or out.links.shape[1] != cur.capacity or out.back.shape[1] != ref.capacity:
        raise ValueError(f"links: out must be LinkFrames of {N} frames with room for {cur.capacity} and {ref.capacity} regions")
    else:
        out.cur, out.ref = cur, ref
    ops.region_links(cur.frames.row_start, cur.frames.runs, cur.n_regions, cur.run_region, ref.frames.row_start, ref.frames.runs,
                     ref.n_regions, ref.run_region, H, W, out.n_pairs, out.links if cur.capacity else None,
                     out.back if ref.capacity else None, mv_q=mv_q, pair_capacity=out.pair_capacity, workspace=out.workspace)
    return out


def _region_planes(what, row_start, runs, run_region, H, W):
    """One frame's run code and run_region -> (value plane, region-id plane), int64 [H,W] each, and the number of regions."""
    rs, x0, x1, val, _ = _parse_runs(what, row_start, runs, H, W)
    rr = np.asarray(run_region).astype(np.int64)
    if rr.ndim != 1 or len(rr) < rs[H] or (rr[:rs[H]] < 0).any():
        raise ValueError(f"{what}: expected the row_start[{H}] region numbers of the runs, none of them negative")
    rr = rr[:rs[H]]
    return np.repeat(val, x1 - x0).reshape(H, W), np.repeat(rr, x1 - x0).reshape(H, W), int(rr.max()) + 1


def links_numpy(cur_row_start, cur_runs, cur_run_region, ref_row_start, ref_runs, ref_run_region, H, W, mv_q=None):
    """The same links on a host without a GPU: one frame's run code and ``run_region`` (as ``RleFrames.to_host`` and ``regions_numpy(...,
    return_run_region=True)`` give them), its reference's, and ``mv_q`` int16 [H,W,2] (None: zero motion) -> the ``(links, back)`` pair of
    structured arrays ``LinkFrames.to_host`` returns for that frame.  Vectorised: both sides decoded to region-id planes, one gather, then
    ``np.unique`` over the pairs."""
    H, W = int(H), int(W)
    val, reg, R = _region_planes("links_numpy", cur_row_start, cur_runs, cur_run_region, H, W)
    rval, rreg, K = _region_planes("links_numpy", ref_row_start, ref_runs, ref_run_region, H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    if mv_q is None:
        tx, ty = xs, ys
    else:
        mv = np.asarray(mv_q)
        if mv.shape != (H, W, 2) or not np.issubdtype(mv.dtype, np.integer):
            raise ValueError(f"links_numpy: mv_q must be integers [{H},{W},2], got {mv.dtype} {mv.shape}")
        mv = mv.astype(np.int64)
        b, r = mv >> 2, mv & 3                           # v = 4 b + r: halves go to the even neighbour
        step = np.where(r < 2, b, np.where(r > 2, b + 1, b + (b & 1)))
        tx, ty = xs + step[..., 0], ys + step[..., 1]
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    cx, cy = np.where(inside, tx, 0), np.where(inside, ty, 0)
    hit = inside & (rval[cy, cx] == val)
    key, count = np.unique(reg[hit] * K + rreg[cy, cx][hit], return_counts=True)
    pr, pk = key // K, key % K
    rows = np.zeros((R, 6), dtype=np.int64)
    rows[:, 0] = -1
    back = np.zeros((K, 4), dtype=np.int64)
    back[:, 0] = -1
    rows[:, 3] = np.bincount(reg[~inside], minlength=R)
    if len(key):
        rows[:, 2], rows[:, 5] = np.bincount(pr, weights=count, minlength=R).astype(np.int64), np.bincount(pr, minlength=R)
        back[:, 2], back[:, 3] = np.bincount(pk, weights=count, minlength=K).astype(np.int64), np.bincount(pk, minlength=K)
        # the largest count first, then the smaller partner: the first entry of each group wins
        order = np.lexsort((pk, -count, pr))
        first = order[np.r_[True, np.diff(pr[order]) != 0]]
        rows[pr[first], 0], rows[pr[first], 1] = pk[first], count[first]
        order = np.lexsort((pr, -count, pk))
        first = order[np.r_[True, np.diff(pk[order]) != 0]]
        back[pk[first], 0], back[pk[first], 1] = pr[first], count[first]
        linked = rows[:, 0] >= 0
        rows[linked, 4] = back[rows[linked, 0], 0] == np.flatnonzero(linked)
    return _records_of(rows, LINK_DTYPE), _records_of(back, BACK_DTYPE)


class AbsorbedFrames(RleFrames):
    """The run code of ``source.frames`` (``source``: a ``RegionFrames``) with the small regions absorbed into their neighbours
    (include/arseg_hip.h, arseg_rle_absorb_fwd), on the device: an ``RleFrames`` with ``target`` int32 [N,source.capacity] (per region of the
    source -1: stable, -2: small and left alone, else the region it went into) and ``n_absorbed`` int32 [N] (-1: the frame could not be
    processed, -2: more neighbour pairs than ``pair_capacity``; the frame's code is not written then).  It carries no regions: ``regions``
    labels it.  ``workspace``: the tables the pass uses, kept so that a repeated call allocates nothing."""

    def __init__(self, row_start, runs, H, W, target, n_absorbed, source, pair_capacity, workspace=None):
        super().__init__(row_start, runs, H, W)
        self.target, self.n_absorbed, self.source = target, n_absorbed, source
        self.pair_capacity, self.workspace = int(pair_capacity), workspace
        if not isinstance(source, RegionFrames) or (source.N, source.frames.H, source.frames.W) != (self.N, self.H, self.W):
            raise ValueError(f"AbsorbedFrames: source must be the RegionFrames of {self.N} frames of {self.H}x{self.W} the code was made from")
        if tuple(n_absorbed.shape) != (self.N,) or target.dim() != 2 or target.shape[0] != self.N:
            raise ValueError(f"AbsorbedFrames: n_absorbed [{self.N}] and target [{self.N},capacity], got {tuple(n_absorbed.shape)} and "
                             f"{tuple(target.shape)}")
        if self.pair_capacity < 1:
            raise ValueError(f"AbsorbedFrames: pair_capacity must be at least 1, got {pair_capacity!r}")

    def _absorbed(self, what):
        """n_absorbed on the host, after raising ``ArsegError`` for a frame that was not written."""
        done = self.n_absorbed.cpu().numpy()
        for n, k in enumerate(done):
            if k == -1:
                raise _lib.ArsegError(f"AbsorbedFrames.{what}: frame {n} could not be processed: its run code overflowed, or its regions are "
                                      f"missing or more than the capacity {self.source.capacity} (regions {int(self.source.n_regions[n])})")
            if k == -2:
                raise _lib.ArsegError(f"AbsorbedFrames.{what}: frame {n} has more neighbour pairs than the pair capacity {self.pair_capacity}")
        return done

    def to_host(self):
        """``RleFrames.to_host`` of the new code; raises ``ArsegError`` naming the frame when it could not be processed (-1) or had more
        neighbour pairs than ``pair_capacity`` (-2)."""
        self._absorbed("to_host")
        return super().to_host()

    def targets_to_host(self):
        """Per frame the target of every region of the source, int32 [R]; the same errors as ``to_host``, and one for a target capacity
        below a frame's regions."""
        self._absorbed("targets_to_host")
        R = self.source.n_regions.cpu().numpy()
        for n, k in enumerate(R):
            if k > self.target.shape[1]:
                raise _lib.ArsegError(f"AbsorbedFrames.targets_to_host: frame {n} has {int(k)} regions, the target capacity is {self.target.shape[1]}")
        rows = self.target[:, :int(R.max())].cpu().numpy()
        return [rows[n, :R[n]] for n in range(self.N)]


def absorb(regions: RegionFrames, min_area, protect=None, pair_capacity=None, out=None) -> AbsorbedFrames:
    """The run code of ``regions.frames`` with every region below ``min_area`` pixels absorbed into the neighbour it shares the longest
    border with, on the GPU: one call of ``ops.rle_absorb`` -> ``AbsorbedFrames`` (an ``RleFrames`` with ``.target`` and ``.n_absorbed``).
    ``protect``: values (0..255) whose regions are never absorbed, whatever their area.  A small region goes into the STABLE neighbour
    (``area >= min_area`` or protected) with the most 4-neighbour pixel pairs along their border, ties to the smaller region number; one
    without a stable neighbour stays.  One pass: a second one is ``absorb(regions(result, ...), ...)``.  ``pair_capacity``: the slots of the
    pair table, default ``3 * regions.frames.capacity`` (which cannot overflow).  ``out``: an ``AbsorbedFrames`` of the same N, H, W to write
    into (its capacities, pair capacity and workspace hold; nothing is allocated then, and ``labels8 -> labels_rle -> rle_regions ->
    rle_absorb -> rle_regions`` can be captured in one HIP graph)."""
    if not isinstance(regions, RegionFrames):
        raise ValueError("absorb: expected the RegionFrames of egress.regions")
    src = regions.frames
    N, H, W, cap, dev = src.N, src.H, src.W, src.capacity, src.runs.device
    if out is None:
        pair_capacity = 3 * cap if pair_capacity is None else int(pair_capacity)
        if pair_capacity < 1:
            raise ValueError(f"absorb: pair_capacity must be at least 1, got {pair_capacity}")
        if not src.runs.is_cuda:
            raise _lib.ArsegError("absorb runs on the GPU only (got CPU tensors); absorb_numpy is the host form")
        _need = _lib.load().arseg_rle_absorb_workspace_bytes(N, cap, regions.capacity, H, pair_capacity)
        out = AbsorbedFrames(torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.empty((N, cap), dtype=torch.int32, device=dev), H, W,
                             torch.empty((N, regions.capacity), dtype=torch.int32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev),
                             regions, pair_capacity, torch.empty((max(_need // 8, 1),), dtype=torch.int64, device=dev))
    elif not isinstance(out, AbsorbedFrames) or (out.N, out.H, out.W) != (N, H, W):
        raise ValueError(f"absorb: out must be AbsorbedFrames of {N} frames of {H}x{W}")
    else:
        out.source = regions
    ops.rle_absorb(src.row_start, src.runs, regions.n_regions, regions.run_region, regions.records, H, W, min_area, out.row_start, out.runs,
                   out.n_absorbed, target=out.target if out.target.shape[1] else None, protect=protect, pair_capacity=out.pair_capacity,
                   workspace=out.workspace)
    return out


def absorb_numpy(row_start, runs, H, W, min_area, protect=None, connectivity=8):
    """The same pass on a host without a GPU: one frame's ``row_start`` [H+1] and ``runs`` [>= row_start[H]] (as ``RleFrames.to_host``
    returns them) -> ``(row_start int32 [H+1], runs uint32, target int32 [R])`` as ``AbsorbedFrames.to_host`` and ``targets_to_host`` give
    them for that frame, the regions being those of ``regions_numpy`` at ``connectivity``.  Vectorised over the runs: the borders from the
    neighbouring run pairs (one search over the frame for the row above), summed per pair of regions with ``np.unique``."""
    H, W, min_area = int(H), int(W), int(min_area)
    if min_area < 1:
        raise ValueError(f"absorb_numpy: min_area must be at least 1, got {min_area}")
    if connectivity not in (4, 8):
        raise ValueError(f"absorb_numpy: connectivity is 4 or 8, got {connectivity!r}")
    _, x0, x1, val, row = _parse_runs("absorb_numpy", row_start, runs, H, W)
    rows, rr = _regions_of(x0, x1, val, row, H, W, connectivity)
    rec, R = _region_records(rows), len(rows)
    stable = rec["area"] >= min_area
    if protect is not None:
        stable |= ops.egress.protect_table(protect, "absorb_numpy")[rec["value"]]
    # neighbouring runs: (i, i + 1) of one row with one pixel pair; a run and the runs above it that overlap it, with the overlap's length
    left = np.flatnonzero(row[:-1] == row[1:])
    u, v = _runs_above(row, x0, x1, W, 0)
    a = np.concatenate([rr[left], rr[left + 1], rr[u], rr[v]])
    b = np.concatenate([rr[left + 1], rr[left], rr[v], rr[u]])
    w = np.concatenate([np.ones(2 * len(left), dtype=np.int64), np.tile(np.minimum(x1[u], x1[v]) - np.maximum(x0[u], x0[v]), 2)])
    voting = (a != b) & ~stable[a] & stable[b]
    key, inverse = np.unique(a[voting] * R + b[voting], return_inverse=True)
    border = np.bincount(inverse.reshape(-1), weights=w[voting], minlength=len(key)).astype(np.int64)
    pa, pb = key // R, key % R
    target = np.where(stable, -1, -2).astype(np.int32)
    if len(key):
        order = np.lexsort((pb, -border, pa))                # the longest border first, then the smaller region: the first of each group wins
        best = order[np.r_[True, np.diff(pa[order]) != 0]]
        target[pa[best]] = pb[best]
    goes = target[rr]
    new = np.where(goes >= 0, rec["value"][np.maximum(goes, 0)], val)
    keep = np.r_[True, (new[1:] != new[:-1]) | (row[1:] != row[:-1])]
    out_start = np.concatenate(([0], np.cumsum(np.bincount(row[keep], minlength=H)))).astype(np.int32)
    return out_start, ((x0[keep] << 8) | new[keep]).astype(np.uint32), target


class ContourFrames(object):
    """The outlines of the regions of ``source`` (a ``RegionFrames``; include/arseg_hip.h, arseg_rle_contours_fwd), on the device: ``counts``
    int32 [N,2] (the loops and the vertices of each frame, exact whatever the capacities; -1, -1: the frame could not be processed),
    ``loops`` int32 [N,loop_capacity,4] (``region, first, count, hole`` per loop) and ``verts`` 32-bit [N,vertex_capacity] (the corners of
    the loops one after the other, ``y << 16 | x``).  ``workspace``: the scratch the pass uses, kept so that a repeated call allocates
    nothing."""

    def __init__(self, counts, loops, verts, source, workspace=None):
        self.counts, self.loops, self.verts, self.source, self.workspace = counts, loops, verts, source, workspace
        if not isinstance(source, RegionFrames):
            raise ValueError("ContourFrames: source must be the RegionFrames the outlines were traced from")
        N = source.N
        if tuple(counts.shape) != (N, 2) or loops.dim() != 3 or loops.shape[0] != N or loops.shape[2] != 4 or verts.dim() != 2 or \
                verts.shape[0] != N:
            raise ValueError(f"ContourFrames: counts [{N},2], loops [{N},capacity,4] and verts [{N},capacity], got {tuple(counts.shape)}, "
                             f"{tuple(loops.shape)} and {tuple(verts.shape)}")

    @property
    def N(self):
        return self.source.N

    @property
    def loop_capacity(self):
        return self.loops.shape[1]

    @property
    def vertex_capacity(self):
        return self.verts.shape[1]

    def needed(self) -> torch.Tensor:
        """The loops and vertices each frame needs (a device view, int32 [N,2]): exact whatever the capacities; a value above its capacity
        is an overflow, -1 a frame that could not be processed."""
        return self.counts

    def to_host(self):
        """Per frame a list of ``(region, hole, int32 [k,2] array of (x, y))``, one entry per loop in the contract's order (outer loops
        clockwise on the screen, holes counter-clockwise), in three copies: the counts, then the loops and vertices up to the largest
        need.  Raises ``ArsegError`` naming the frame when it could not be processed or needs more loops or vertices than the capacity."""
        need = self.counts.cpu().numpy()
        for n, (L, V) in enumerate(need):
            if L < 0:
                raise _lib.ArsegError(f"ContourFrames.to_host: frame {n} could not be processed: its run code overflowed or it has no regions "
                                      f"(regions {int(self.source.n_regions[n])})")
            if L > self.loop_capacity or V > self.vertex_capacity:
                raise _lib.ArsegError(f"ContourFrames.to_host: frame {n} needs {int(L)} loops and {int(V)} vertices, the capacities are "
                                      f"{self.loop_capacity} and {self.vertex_capacity}")
        rows = self.loops[:, :int(need[:, 0].max())].cpu().numpy()
        words = self.verts[:, :int(need[:, 1].max())].cpu().numpy().view(np.uint32)
        return [_polygons(rows[n, :need[n, 0]], words[n, :need[n, 1]]) for n in range(self.N)]


def _polygons(loops, verts):
    """One frame's loop records and vertex words -> [(region, hole, int32 [k,2] of (x, y))]."""
    return [(int(r), int(hole), np.stack([verts[first:first + count] & 0xFFFF, verts[first:first + count] >> 16], axis=1).astype(np.int32))
            for r, first, count, hole in loops]


def contours(regions: RegionFrames, loop_capacity=None, vertex_capacity=None, out=None) -> ContourFrames:
    """The outlines of the regions as closed polygon loops, traced on the GPU from the run code: one call of ``ops.rle_contours`` ->
    ``ContourFrames``.  A vertex is a corner of the pixel grid; every loop has its region on the right hand (outer loops clockwise on the
    screen, holes counter-clockwise), holds corners only and begins at its smallest vertex in (y, x) order; where a region touches itself
    across a corner the loop joins the two pixels at ``regions.connectivity`` 8 and parts them at 4.  The capacities default to the bounds
    that cannot overflow: one loop and four vertices per run.  ``out``: a ``ContourFrames`` of the same N to write into (its capacities
    and workspace hold; nothing is allocated then, and ``labels8 -> labels_rle -> rle_regions -> rle_contours`` can be captured in one HIP
    graph)."""
    if not isinstance(regions, RegionFrames):
        raise ValueError("contours: expected the RegionFrames of egress.regions")
    src = regions.frames
    N, H, W, cap, dev = src.N, src.H, src.W, src.capacity, src.runs.device
    if out is None:
        loop_capacity = cap if loop_capacity is None else int(loop_capacity)
        vertex_capacity = 4 * cap if vertex_capacity is None else int(vertex_capacity)
        if loop_capacity < 0 or vertex_capacity < 0:
            raise ValueError(f"contours: the capacities must not be negative, got {loop_capacity} and {vertex_capacity}")
        if not src.runs.is_cuda:
            raise _lib.ArsegError("contours runs on the GPU only (got CPU tensors); contours_numpy is the host form")
        _need = _lib.load().arseg_rle_contours_workspace_bytes(N, cap)
        out = ContourFrames(torch.empty((N, 2), dtype=torch.int32, device=dev), torch.empty((N, loop_capacity, 4), dtype=torch.int32, device=dev),
                            torch.empty((N, vertex_capacity), dtype=torch.int32, device=dev), regions,
                            torch.empty((max(_need // 16, 1), 4), dtype=torch.int32, device=dev))
    elif not isinstance(out, ContourFrames) or out.N != N:
        raise ValueError(f"contours: out must be ContourFrames of {N} frames")
    else:
        out.source = regions
    ops.rle_contours(src.row_start, src.runs, regions.n_regions, regions.run_region, H, W, out.counts,
                     loops=out.loops if out.loop_capacity else None, verts=out.verts if out.vertex_capacity else None,
                     connectivity=regions.connectivity, workspace=out.workspace)
    return out


def contours_numpy(row_start, runs, H, W, connectivity=8):
    """The same pass on a host without a GPU: one frame's ``row_start`` [H+1] and ``runs`` [>= row_start[H]] (as ``RleFrames.to_host``
    returns them) -> ``(counts int32 [2], loops int32 [L,4], verts uint32 [V])`` as arseg_rle_contours_fwd leaves them with room for
    everything, the regions being those of ``regions_numpy`` at ``connectivity``.  Every run gives two vertical edges (its left end
    travelled upwards, its right end downwards); the edge that follows an edge along its loop is found from the neighbouring row, and the
    cycles of that permutation are the loops."""
    H, W = int(H), int(W)
    if H > 65535 or W > 65535:
        raise ValueError(f"contours_numpy: H and W at most 65535 (a vertex is y << 16 | x), got {H}x{W}")
    if connectivity not in (4, 8):
        raise ValueError(f"contours_numpy: connectivity is 4 or 8, got {connectivity!r}")
    rs, starts, x1, val, row = _parse_runs("contours_numpy", row_start, runs, H, W)
    _, rr = _regions_of(starts, x1, val, row, H, W, connectivity)
    eight = connectivity == 8
    n = len(starts)
    rs, x0, x1, val, row = rs.tolist(), starts.tolist(), x1.tolist(), val.tolist(), row.tolist()
    succ, end = [0] * (2 * n), [0] * (2 * n)                  # the edge after edge e = 2 * run + side, and the corner where it starts

    def cover(y, x):                                          # the run of row y that covers column x
        return rs[y] + int(np.searchsorted(starts[rs[y]:rs[y + 1]], x, side="right")) - 1

    def east(t, Y, v, j, stop):                               # along the top of run t (row Y) to the first run >= j above with value v
        while j < stop and (x0[j] <= x1[t] if eight else x0[j] < x1[t]):
            if val[j] == v:
                return 2 * j, (Y << 16) | x0[j]
            j += 1
        return 2 * t + 1, (Y << 16) | x1[t]

    def west(t, Y, v, k, stop):                               # along the bottom of run t (row Y - 1) to the last run <= k below with value v
        while k >= stop and (x1[k] >= x0[t] if eight else x1[k] > x0[t]):
            if val[k] == v:
                return 2 * k + 1, (Y << 16) | x1[k]
            k -= 1
        return 2 * t, (Y << 16) | x0[t]

    for y in range(H):
        for i in range(rs[y], rs[y + 1]):
            a0, a1, v = x0[i], x1[i], val[i]
            if y == 0:                                        # the left end, arriving at (a0, y)
                succ[2 * i], end[2 * i] = east(i, y, v, 0, 0)
            else:
                p = cover(y - 1, a0)
                ur = val[p] == v
                ul = a0 > 0 and (ur if x0[p] < a0 else val[p - 1] == v)
                if ur and not ul:
                    succ[2 * i], end[2 * i] = 2 * p, (y << 16) | a0
                elif ur or (eight and ul):
                    succ[2 * i], end[2 * i] = west(p if ur else p - 1, y, v, i - 1, rs[y])
                else:
                    succ[2 * i], end[2 * i] = east(i, y, v, p + 1, rs[y])
            e = 2 * i + 1
            if y == H - 1:                                    # the right end, arriving at (a1, y + 1)
                succ[e], end[e] = west(i, y + 1, v, -1, 0)
            else:
                p = cover(y + 1, a1 - 1)
                bl = val[p] == v
                br = a1 < W and (bl if x1[p] > a1 else val[p + 1] == v)
                if bl and not br:
                    succ[e], end[e] = 2 * p + 1, ((y + 1) << 16) | a1
                elif bl or (eight and br):
                    succ[e], end[e] = east(p if bl else p + 1, y + 1, v, i + 1, rs[y + 1])
                else:
                    succ[e], end[e] = west(i, y + 1, v, p, rs[y + 1])
    loops, verts, seen = [], [], [False] * (2 * n)
    for lead in range(2 * n):                                 # the smallest edge of every cycle, in rising order
        if seen[lead]:
            continue
        pts, e = [], lead
        while not seen[e]:
            seen[e] = True
            i = e >> 1
            own = ((row[i] + 1) << 16 | x1[i]) if e & 1 else (row[i] << 16 | x0[i])
            if end[e] != own:
                pts += [own, end[e]]
            e = succ[e]
        if lead & 1:                                          # a hole begins where its smallest edge starts
            pts = pts[-1:] + pts[:-1]
        loops.append((rr[lead >> 1], len(verts), len(pts), lead & 1))
        verts += pts
    return (np.array([len(loops), len(verts)], dtype=np.int32), np.array(loops, dtype=np.int32).reshape(-1, 4),
            np.array(verts, dtype=np.uint32))


class SimplifiedContours(ContourFrames):
    """``contours`` (a ``ContourFrames``) simplified to ``tolerance`` pixels (include/arseg_hip.h, arseg_contours_simplify_fwd), on the
    device: a ``ContourFrames`` itself -- ``counts``, ``loops``, ``verts``, ``needed()`` and ``to_host()`` mean what they mean there, the
    vertices being the kept ones -- whose ``source`` is the input's."""

    def __init__(self, counts, loops, verts, contours, tolerance, workspace=None):
        if not isinstance(contours, ContourFrames):
            raise ValueError("SimplifiedContours: contours must be the ContourFrames that were simplified")
        super().__init__(counts, loops, verts, contours.source, workspace)
        self.contours, self.tolerance = contours, tolerance
        if loops.shape[1] != contours.loop_capacity:
            raise ValueError(f"SimplifiedContours: loops must have the input's capacity {contours.loop_capacity}, got {loops.shape[1]}")


def simplify(contours: ContourFrames, tolerance, vertex_capacity=None, out=None) -> SimplifiedContours:
    """The outlines with the vertices dropped that lie within ``tolerance`` pixels (a non-negative multiple of 0.25) of the polygon that
    remains, on the GPU: one call of ``ops.contours_simplify`` -> ``SimplifiedContours``.  Per loop Douglas-Peucker on the two chains
    between its first vertex and the vertex farthest from it; a loop that would keep fewer than 3 vertices is left whole; loops, their
    order, first vertices, regions and hole marks stay.  ``vertex_capacity`` defaults to the input's, which cannot overflow.  ``out``: a
    ``SimplifiedContours`` of the same N and loop capacity to write into (its vertex capacity and workspace hold; nothing is allocated
    then, and the call can be captured in one HIP graph behind ``rle_contours``).  Each loop is simplified on its own: a border shared by
    two regions is simplified twice, and the two results may differ by up to the tolerance (``simplify_shared`` simplifies it once)."""
    if not isinstance(contours, ContourFrames):
        raise ValueError("simplify: expected the ContourFrames of egress.contours")
    ops.tolerance_q(tolerance, "simplify")
    N, lcap, vcap, dev = contours.N, contours.loop_capacity, contours.vertex_capacity, contours.counts.device
    if out is None:
        vertex_capacity = vcap if vertex_capacity is None else int(vertex_capacity)
        if vertex_capacity < 0:
            raise ValueError(f"simplify: the capacity must not be negative, got {vertex_capacity}")
        if not contours.counts.is_cuda:
            raise _lib.ArsegError("simplify runs on the GPU only (got CPU tensors); simplify_numpy is the host form")
        _need = _lib.load().arseg_contours_simplify_workspace_bytes(N, lcap, vcap)
        out = SimplifiedContours(torch.empty((N, 2), dtype=torch.int32, device=dev), torch.empty((N, lcap, 4), dtype=torch.int32, device=dev),
                                 torch.empty((N, vertex_capacity), dtype=torch.int32, device=dev), contours, tolerance,
                                 torch.empty((max(_need // 16, 1), 4), dtype=torch.int32, device=dev))
    elif not isinstance(out, SimplifiedContours) or out.N != N or out.loop_capacity != lcap or out is contours:
        raise ValueError(f"simplify: out must be SimplifiedContours of {N} frames with a loop capacity of {lcap}")
    else:
        out.contours, out.source, out.tolerance = contours, contours.source, tolerance
    frame = contours.source.frames
    ops.contours_simplify(contours.counts, contours.loops if lcap else None, contours.verts if vcap else None, frame.H, frame.W, tolerance,
                          out.counts, loops_out=out.loops if lcap else None, verts_out=out.verts if out.vertex_capacity else None,
                          workspace=out.workspace)
    return out


def simplify_numpy(counts, loops, verts, tolerance):
    """The same pass on a host without a GPU: one frame's ``(counts [2], loops [>= L,4], verts [>= V])`` (as ``contours_numpy`` returns
    them) -> the same three arrays of the simplified outlines, as arseg_contours_simplify_fwd leaves them with room for everything.  The
    recursion runs on an explicit stack of segments, the distances of a segment's interior in one vectorised step."""
    tol = ops.tolerance_q(tolerance, "simplify_numpy")
    L, V = int(counts[0]), int(counts[1])
    if L < 0 or V < 0 or L > len(loops) or V > len(verts):
        raise ValueError(f"simplify_numpy: the frame holds {len(loops)} loops and {len(verts)} vertices, its counts say {L} and {V}")
    words = np.asarray(verts)[:V].astype(np.int64) & 0xFFFFFFFF
    xs, ys = words & 0xFFFF, words >> 16
    if V and (xs.max() > 16384 or ys.max() > 16384):
        raise ValueError("simplify_numpy: H and W at most 16384")
    records, kept_words = np.array(np.asarray(loops)[:L], dtype=np.int32).reshape(-1, 4), []
    at = 0
    for k, (_, first, count, _) in enumerate(records.tolist()):
        if first < 0 or count < 0 or first + count > V:
            raise ValueError(f"simplify_numpy: loop {k} lies outside the frame's {V} vertices")
        x, y = np.append(xs[first:first + count], xs[first:first + 1]), np.append(ys[first:first + count], ys[first:first + 1])
        keep = np.zeros(count, dtype=bool)
        if count:
            far = int(np.argmax((x[:count] - x[0]) ** 2 + (y[:count] - y[0]) ** 2))          # argmax: the first of a tie
            keep[[0, far]] = True
            todo = [(0, far), (far, count)]
            while todo:
                a, b = todo.pop()
                if b - a < 2:
                    continue
                ex, ey = int(x[b] - x[a]), int(y[b] - y[a])
                c = np.abs(ex * (y[a + 1:b] - y[a]) - ey * (x[a + 1:b] - x[a]))
                i = int(np.argmax(c))
                if 16 * int(c[i]) ** 2 > tol * (ex * ex + ey * ey):
                    keep[a + 1 + i] = True
                    todo += [(a, a + 1 + i), (a + 1 + i, b)]
            if keep.sum() < 3:
                keep[:] = True
        records[k, 1:3] = (at, int(keep.sum()))
        at += int(keep.sum())
        kept_words.append(words[first:first + count][keep])
    out = np.concatenate(kept_words).astype(np.uint32) if kept_words else np.zeros(0, dtype=np.uint32)
    return np.array([L, at], dtype=np.int32), records, out


class SharedContours(SimplifiedContours):
    """``contours`` simplified to ``tolerance`` pixels with shared borders (include/arseg_hip.h, arseg_contours_simplify_shared_fwd), on
    the device: a ``SimplifiedContours`` whose loops were cut where three regions meet and simplified arc by arc, so that two
    neighbouring polygons keep the same vertices of their common border and leave no gap or overlap between them.  A loop may hold more
    vertices than its source (the junctions inside its straight edges are vertices now), and a region thinner than the tolerance may
    come out degenerate -- two vertices, or all of them on one line: its neighbours close over it."""

    def to_host(self, drop_degenerate=False):
        """``ContourFrames.to_host``; with ``drop_degenerate`` the loops whose kept vertices span no area are left out (their neighbours
        cover them)."""
        frames = super().to_host()
        if not drop_degenerate:
            return frames
        return [[loop for loop in frame if _area2(loop[2]) != 0] for frame in frames]


def _area2(pts):
    """Twice the signed area of a closed polygon int [k,2]."""
    p = np.asarray(pts, dtype=np.int64)
    q = np.roll(p, -1, axis=0)
    return int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


def simplify_shared(contours: ContourFrames, tolerance, vertex_capacity=None, out=None) -> SharedContours:
    """``simplify`` for neighbours that must fit: the outlines within ``tolerance`` pixels (a non-negative multiple of 0.25), every border
    between two regions simplified once, on the GPU: one call of ``ops.contours_simplify_shared`` -> ``SharedContours``.  The run code is
    ``contours.source.frames``'.  Every loop gets the junctions inside its straight edges as vertices, is cut at every junction (a grid
    corner where three or four regions, or the frame's corner, meet) and each arc goes through Douglas-Peucker with ties decided by the
    vertex, not by the direction of travel; a closed arc that would keep fewer than 3 vertices stays whole; loops, their order, regions
    and hole marks stay.  ``vertex_capacity`` defaults to the input's plus twice the run code's capacity, which cannot overflow.
    ``out``: a ``SharedContours`` of the same N and loop capacity to write into (its vertex capacity and workspace hold; nothing is
    allocated then, and the call can be captured in one HIP graph behind ``rle_contours``).  Raises as ``simplify`` does."""
    if not isinstance(contours, ContourFrames):
        raise ValueError("simplify_shared: expected the ContourFrames of egress.contours")
    ops.tolerance_q(tolerance, "simplify_shared")
    frame = contours.source.frames
    N, lcap, vcap, dev = contours.N, contours.loop_capacity, contours.vertex_capacity, contours.counts.device
    if out is None:
        vertex_capacity = vcap + 2 * frame.capacity if vertex_capacity is None else int(vertex_capacity)
        if vertex_capacity < 0:
            raise ValueError(f"simplify_shared: the capacity must not be negative, got {vertex_capacity}")
        if not contours.counts.is_cuda:
            raise _lib.ArsegError("simplify_shared runs on the GPU only (got CPU tensors); simplify_shared_numpy is the host form")
        _need = _lib.load().arseg_contours_simplify_shared_workspace_bytes(N, frame.capacity, lcap, vcap)
        out = SharedContours(torch.empty((N, 2), dtype=torch.int32, device=dev), torch.empty((N, lcap, 4), dtype=torch.int32, device=dev),
                             torch.empty((N, vertex_capacity), dtype=torch.int32, device=dev), contours, tolerance,
                             torch.empty((max(_need // 16, 1), 4), dtype=torch.int32, device=dev))
    elif not isinstance(out, SharedContours) or out.N != N or out.loop_capacity != lcap or out is contours:
        raise ValueError(f"simplify_shared: out must be SharedContours of {N} frames with a loop capacity of {lcap}")
    else:
        out.contours, out.source, out.tolerance = contours, contours.source, tolerance
    ops.contours_simplify_shared(frame.row_start, frame.runs, contours.counts, contours.loops if lcap else None,
                                 contours.verts if vcap else None, frame.H, frame.W, tolerance, out.counts,
                                 loops_out=out.loops if lcap else None, verts_out=out.verts if out.vertex_capacity else None,
                                 workspace=out.workspace)
    return out


def simplify_shared_numpy(row_start, runs, H, W, counts, loops, verts, tolerance):
    """The same pass on a host without a GPU: one frame's run code (as ``RleFrames.to_host`` returns it) and its ``(counts [2], loops
    [>= L,4], verts [>= V])`` (as ``contours_numpy`` returns them) -> the three arrays of the outlines simplified with shared borders, as
    arseg_contours_simplify_shared_fwd leaves them with room for everything.  The junctions are a map of the grid corners computed from
    the decoded plane in one vectorised step; an edge takes its inside junctions from a slice of that map; the recursion of an arc runs
    on an explicit stack of segments."""
    tol = ops.tolerance_q(tolerance, "simplify_shared_numpy")
    H, W = int(H), int(W)
    if not (0 < H <= 16384 and 0 < W <= 16384):
        raise ValueError(f"simplify_shared_numpy: H and W positive and at most 16384, got {H}x{W}")
    L, V = int(counts[0]), int(counts[1])
    if L < 0 or V < 0 or L > len(loops) or V > len(verts):
        raise ValueError(f"simplify_shared_numpy: the frame holds {len(loops)} loops and {len(verts)} vertices, its counts say {L} and {V}")
    padded = np.full((H + 2, W + 2), -1, dtype=np.int16)                     # -1: outside the frame
    padded[1:-1, 1:-1] = rle_decode_numpy(row_start, runs, H, W)
    a, b, c, d = padded[:-1, :-1], padded[:-1, 1:], padded[1:, :-1], padded[1:, 1:]          # the four pixels of corner (x, y) at [y, x]
    junction = ((a != b).astype(np.int8) + (c != d) + (a != c) + (b != d)) >= 3
    junction[[0, 0, H, H], [0, W, 0, W]] = True
    words = np.asarray(verts)[:V].astype(np.int64) & 0xFFFFFFFF
    if V and ((words & 0xFFFF).max() > W or (words >> 16).max() > H):
        raise ValueError(f"simplify_shared_numpy: a vertex lies outside the {H}x{W} frame")
    records, kept_words = np.array(np.asarray(loops)[:L], dtype=np.int32).reshape(-1, 4), []
    at = 0
    for k, (_, first, count, _) in enumerate(records.tolist()):
        if first < 0 or count < 0 or first + count > V:
            raise ValueError(f"simplify_shared_numpy: loop {k} lies outside the frame's {V} vertices")
        w = words[first:first + count]
        pieces = []
        for w0, w1 in zip(w.tolist(), np.roll(w, -1).tolist()):             # the expanded loop: each corner and the junctions inside its edge
            x0, y0, x1, y1 = w0 & 0xFFFF, w0 >> 16, w1 & 0xFFFF, w1 >> 16
            pieces.append(np.array([w0], dtype=np.int64))
            if y0 == y1:
                xs = np.flatnonzero(junction[y0, min(x0, x1) + 1:max(x0, x1)]) + min(x0, x1) + 1
                pieces.append((y0 << 16) | (xs if x1 > x0 else xs[::-1]))
            elif x0 == x1:
                ys = np.flatnonzero(junction[min(y0, y1) + 1:max(y0, y1), x0]) + min(y0, y1) + 1
                pieces.append(((ys if y1 > y0 else ys[::-1]) << 16) | x0)
            else:
                raise ValueError(f"simplify_shared_numpy: loop {k} has an edge along neither axis")
        e = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int64)
        n = len(e)
        keep = junction[e >> 16, e & 0xFFFF].copy() if n else np.zeros(0, dtype=bool)
        cuts = np.flatnonzero(keep)
        rot = int(cuts[0]) if len(cuts) else 0
        e2 = np.concatenate([e[rot:], e[:rot + 1]]) if n else e                 # from the first junction passage, closed
        x, y = e2 & 0xFFFF, e2 >> 16
        ends = np.append(cuts - rot, n) if len(cuts) else np.array([0, n])
        stay = np.zeros(n + 1, dtype=bool)

        def chain(lo, hi):
            todo = [(lo, hi)]
            while todo:
                p, q = todo.pop()
                if q - p < 2:
                    continue
                ex, ey = int(x[q] - x[p]), int(y[q] - y[p])
                c = np.abs(ex * (y[p + 1:q] - y[p]) - ey * (x[p + 1:q] - x[p]))
                tie = np.flatnonzero(c == c.max())
                i = p + 1 + int(tie[np.argmin(e2[p + 1:q][tie])])           # the smallest vertex word of a tie
                if 16 * int(c.max()) ** 2 > tol * (ex * ex + ey * ey):
                    stay[i] = True
                    todo += [(p, i), (i, q)]

        for lo, hi in zip(ends[:-1].tolist(), ends[1:].tolist()):
            stay[lo] = True
            if e2[lo] != e2[hi]:
                chain(lo, hi)
                continue
            far = (x[lo:hi] - x[lo]) ** 2 + (y[lo:hi] - y[lo]) ** 2
            tie = np.flatnonzero(far == far.max())
            a1 = lo + int(tie[np.argmin(e2[lo:hi][tie])])
            stay[a1] = True
            chain(lo, a1)
            chain(a1, hi)
            if stay[lo:hi].sum() < 3:
                stay[lo:hi] = True
        keep = np.roll(stay[:n], rot)
        records[k, 1:3] = (at, int(keep.sum()))
        at += int(keep.sum())
        kept_words.append(e[keep])
    out = np.concatenate(kept_words).astype(np.uint32) if kept_words else np.zeros(0, dtype=np.uint32)
    return np.array([L, at], dtype=np.int32), records, out


class FilledFrames(object):
    """``contours`` (any ``ContourFrames``) filled back into label planes (include/arseg_hip.h, arseg_contours_fill_fwd), on the device:
    ``labels`` uint8 [N,H,W] (every region's loops filled by the even-odd rule on the pixel centres, the larger region number on top, the
    background value where no region covers), ``counts`` int32 [N] (the edge-row crossings each frame needs; -1: the frame could not be
    processed) and ``stats`` int64 [N,3 + 3 * 256] (``gaps, excess, changed, ref_area[256], fill_area[256], both[256]`` against the
    reference plane the call was given).  ``workspace``: the scratch the pass uses, kept so that a repeated call allocates nothing."""

    def __init__(self, labels, counts, stats, contours, event_capacity, background=255, workspace=None):
        self.labels, self.counts, self.stats, self.contours, self.workspace = labels, counts, stats, contours, workspace
        self.event_capacity, self.background = int(event_capacity), int(background)
        if not isinstance(contours, ContourFrames):
            raise ValueError("FilledFrames: contours must be the ContourFrames that were filled")
        N = contours.N
        if labels.dim() != 3 or labels.shape[0] != N or tuple(counts.shape) != (N,) or tuple(stats.shape) != (N, _lib.FILL_NSTATS):
            raise ValueError(f"FilledFrames: labels [{N},H,W], counts [{N}] and stats [{N},{_lib.FILL_NSTATS}], got {tuple(labels.shape)}, "
                             f"{tuple(counts.shape)} and {tuple(stats.shape)}")

    @property
    def N(self):
        return self.contours.N

    def needed(self) -> torch.Tensor:
        """The crossings each frame needs (a device view, int32 [N]): exact whatever the capacity; a value above ``event_capacity`` is an
        overflow (the frame's plane and stats were not written), -1 a frame that could not be processed."""
        return self.counts

    def rle(self, capacity, out=None) -> RleFrames:
        """The filled planes as run codes (``rle_of_planes``): the mask re-enters the chain -- ``regions``, ``links``, ``absorb``."""
        frames = rle_of_planes(self.labels, capacity, out=out)
        frames.labels = self.labels
        return frames

    def fidelity(self):
        """What the polygons did to the mask, per frame a dict: ``gaps`` (pixels no polygon covers), ``excess`` (coverings beyond the first,
        summed over the pixels), ``changed`` (pixels whose value differs from the reference; gaps count), ``iou`` (value -> both / (ref_area
        + fill_area - both) for the values present on either side) and ``miou`` (their mean; None without any), in one copy of ``counts``
        and ``stats``.  Without a reference ``changed`` is 0 and the areas are those of the fill alone.  Raises ``ArsegError`` naming a
        frame that was refused or needs more crossings than the capacity."""
        both = torch.cat([self.counts.to(torch.int64)[:, None], self.stats], dim=1).cpu().numpy()
        out = []
        for n, row in enumerate(both):
            if row[0] < 0:
                raise _lib.ArsegError(f"FilledFrames.fidelity: frame {n} could not be processed: its outlines were refused or overflowed, or "
                                      f"its regions are missing")
            if row[0] > self.event_capacity:
                raise _lib.ArsegError(f"FilledFrames.fidelity: frame {n} needs {int(row[0])} crossings, the capacity is {self.event_capacity}")
            ref_area, fill_area, inter = row[4:260], row[260:516], row[516:772]
            union = ref_area + fill_area - inter
            iou = {int(v): float(inter[v]) / float(union[v]) for v in np.flatnonzero(union)}
            out.append({"gaps": int(row[1]), "excess": int(row[2]), "changed": int(row[3]), "iou": iou,
                        "miou": float(np.mean(list(iou.values()))) if iou else None})
        return out


def fill(contours: ContourFrames, background=255, ref=None, event_capacity=None, out=None) -> FilledFrames:
    """The polygons back to masks, on the GPU: one call of ``ops.contours_fill`` -> ``FilledFrames``.  ``contours``: any
    ``ContourFrames`` -- exact outlines, ``SimplifiedContours`` or ``SharedContours``; a region's value comes from
    ``contours.source.records``.  A pixel belongs to a region when its centre lies inside the region's loops by the even-odd rule (a centre
    on an edge goes to the polygon on the right of the edge); where several regions cover it the largest region number wins, where none
    does it gets ``background``.  ``ref``: the mask to compare with -- None, a uint8 [N,H,W] device plane, or True: the plane the run code
    was taken from (``contours.source.frames.labels``) when it is kept, else that run code decoded.  ``event_capacity`` defaults to twice
    the run code's capacity, which cannot overflow for outlines that come from it.  ``out``: a ``FilledFrames`` of the same N, H, W to
    write into (its capacity and workspace hold; nothing is allocated then, and the call can be captured in one HIP graph behind
    ``rle_contours`` and the simplify passes)."""
    if not isinstance(contours, ContourFrames):
        raise ValueError("fill: expected the ContourFrames of egress.contours, egress.simplify or egress.simplify_shared")
    background = int(background)
    if not 0 <= background <= 255:
        raise ValueError(f"fill: background is a byte, got {background}")
    found = contours.source
    frame = found.frames
    N, H, W, lcap, vcap, dev = contours.N, frame.H, frame.W, contours.loop_capacity, contours.vertex_capacity, contours.counts.device
    if out is None:
        event_capacity = 2 * frame.capacity if event_capacity is None else int(event_capacity)
        if event_capacity < 0:
            raise ValueError(f"fill: the capacity must not be negative, got {event_capacity}")
        if not contours.counts.is_cuda:
            raise _lib.ArsegError("fill runs on the GPU only (got CPU tensors); fill_numpy is the host form")
        _need = _lib.load().arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, event_capacity)
        out = FilledFrames(torch.empty((N, H, W), dtype=torch.uint8, device=dev), torch.empty((N,), dtype=torch.int32, device=dev),
                           torch.zeros((N, _lib.FILL_NSTATS), dtype=torch.int64, device=dev), contours, event_capacity, background,
                           torch.empty((max(_need // 16, 1), 2), dtype=torch.int64, device=dev))
    elif not isinstance(out, FilledFrames) or out.N != N or tuple(out.labels.shape) != (N, H, W):
        raise ValueError(f"fill: out must be FilledFrames of {N} frames of {H}x{W}")
    else:
        out.contours, out.background = contours, background
    if ref is True:
        ref = frame.labels if frame.labels is not None else frame.decode()
    ops.contours_fill(contours.counts, contours.loops if lcap else None, contours.verts if vcap else None, found.n_regions,
                      found.records if found.capacity else None, H, W, out.labels, out.counts, background=background, ref_labels=ref,
                      stats=out.stats, event_capacity=out.event_capacity, workspace=out.workspace)
    return out


def fill_numpy(counts, loops, verts, values, H, W, background=255):
    """The same fill on a host without a GPU: one frame's ``(counts [2], loops [>= L,4], verts [>= V])`` (as ``contours_numpy``,
    ``simplify_numpy`` or ``simplify_shared_numpy`` return them) and ``values`` (the value of every region, e.g. ``regions_numpy``'s
    ``value`` field) -> ``(plane uint8 [H,W], gaps, excess)``.  All edges at once: the rows an edge crosses are laid out by ``np.repeat``,
    the crossing columns come from the contract's formula, one sort by (region, row, column) pairs them into spans, and the spans are
    painted in rising region number."""
    H, W, background = int(H), int(W), int(background)
    if not (0 < H <= 16384 and 0 < W <= 16384) or not 0 <= background <= 255:
        raise ValueError(f"fill_numpy: H and W positive and at most 16384 and background a byte, got {H}x{W} and {background}")
    L, V = int(counts[0]), int(counts[1])
    if L < 0 or V < 0 or L > len(loops) or V > len(verts):
        raise ValueError(f"fill_numpy: the frame holds {len(loops)} loops and {len(verts)} vertices, its counts say {L} and {V}")
    values = np.asarray(values).astype(np.int64).reshape(-1)
    rec = np.asarray(loops)[:L].astype(np.int64).reshape(-1, 4)
    region, first, count = rec[:, 0], rec[:, 1], rec[:, 2]
    if L and (first.min() < 0 or count.min() < 0 or (first + count).max() > V):
        raise ValueError(f"fill_numpy: a loop lies outside the frame's {V} vertices")
    if L and (region.min() < 0 or region.max() >= len(values)):
        raise ValueError(f"fill_numpy: a loop names a region outside the {len(values)} values")
    words = np.asarray(verts)[:V].astype(np.int64) & 0xFFFFFFFF
    if V and ((words & 0xFFFF).max() > W or (words >> 16).max() > H):
        raise ValueError(f"fill_numpy: a vertex lies outside the {H}x{W} frame")
    plane = np.full((H, W), background, dtype=np.uint8)
    # every vertex with its successor along its loop
    start = np.repeat(first, count)
    at = start + np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
    nxt = np.where(at + 1 < start + np.repeat(count, count), at + 1, start)
    xa, ya, xb, yb, r = words[at] & 0xFFFF, words[at] >> 16, words[nxt] & 0xFFFF, words[nxt] >> 16, np.repeat(region, count)
    swap = ya > yb
    xa, xb, ya, yb = np.where(swap, xb, xa), np.where(swap, xa, xb), np.minimum(ya, yb), np.maximum(ya, yb)
    dy = yb - ya                                                   # 0: a horizontal edge crosses no row
    e = np.repeat(np.arange(len(dy)), dy)
    y = ya[e] + np.arange(dy.sum()) - np.repeat(np.cumsum(dy) - dy, dy)
    num = 2 * xa[e] * dy[e] + (2 * y + 1 - 2 * ya[e]) * (xb[e] - xa[e]) - dy[e]
    xs = np.clip(-((-num) // (2 * dy[e])), 0, W)                   # the ceiling, for either sign
    order = np.lexsort((xs, y, r[e]))
    c0, c1, row, owner = xs[order][0::2], xs[order][1::2], y[order][0::2], r[e][order][0::2]
    if len(xs) % 2 or (row != y[order][1::2]).any() or (owner != r[e][order][1::2]).any():
        raise ValueError("fill_numpy: a region crosses a row an odd number of times: its loops are not closed")
    length = c1 - c0
    where = np.repeat(row * W + c0, length) + np.arange(length.sum()) - np.repeat(np.cumsum(length) - length, length)
    plane.reshape(-1)[where] = np.repeat(values[owner] & 0xFF, length).astype(np.uint8)          # in rising region number: the last one stays
    covered = np.bincount(where, minlength=H * W)
    return plane, int((covered == 0).sum()), int((covered - np.minimum(covered, 1)).sum())


class TrackIds(object):
    """Persistent ids for the regions of a stream, from the links alone.  Pure Python on the ``links`` arrays of ``LinkFrames.to_host`` /
    ``links_numpy``; it has no thresholds -- what to do with a short-lived id is the caller's business.

    A region whose link is mutual (it is the largest part of the reference region it mostly came from) inherits that region's id.  Every
    other region gets the next fresh id, and its parent is the id of the reference region it mostly came from (a split or a merge), or -1."""

    def __init__(self):
        self.next_id = 0
        self.key_ids = None          # ids of the current keyframe's regions
        self.last_ids = None         # ids of the most recent frame's regions (a keyframe included)

    def _fresh(self, count):
        ids = np.arange(self.next_id, self.next_id + count, dtype=np.int64)
        self.next_id += count
        return ids

    def _assign(self, links, ref_ids, what):
        ref = np.asarray(links["ref_region"], dtype=np.int64)
        mutual = np.asarray(links["mutual"], dtype=np.int64) == 1
        if len(ref) and ref.max() >= len(ref_ids):
            raise ValueError(f"{what}: the links name reference region {int(ref.max())}, the reference has {len(ref_ids)} regions")
        ids = np.full(len(ref), -1, dtype=np.int64)
        ids[mutual] = ref_ids[ref[mutual]]
        ids[~mutual] = self._fresh(int((~mutual).sum()))
        parents = np.full(len(ref), -1, dtype=np.int64)
        born = ~mutual & (ref >= 0)
        parents[born] = ref_ids[ref[born]]
        return ids, parents

    def keyframe(self, n_regions, links=None):
        """A keyframe with ``n_regions`` regions -> their ids, int64 [n_regions].  ``links``: the links of this keyframe's regions against the
        previous frame's regions, made with ``mv_q=None`` (zero motion): ids survive the GOP boundary through them.  Without: all fresh."""
        n_regions = int(n_regions)
        if links is None:
            ids = self._fresh(n_regions)
        else:
            if self.last_ids is None:
                raise ValueError("TrackIds.keyframe: links given, but there is no previous frame")
            if len(links) != n_regions:
                raise ValueError(f"TrackIds.keyframe: {n_regions} regions, {len(links)} links")
            ids, _ = self._assign(links, self.last_ids, "TrackIds.keyframe")
        self.key_ids = self.last_ids = ids
        return ids

    def frame(self, links):
        """A non-keyframe's links against the current keyframe -> (ids, parents), int64 [regions] each."""
        if self.key_ids is None:
            raise ValueError("TrackIds.frame: no keyframe yet")
        ids, parents = self._assign(links, self.key_ids, "TrackIds.frame")
        self.last_ids = ids
        return ids, parents
