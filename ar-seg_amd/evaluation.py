"""Hot-path pieces of the reference's ``evaluation.py`` on libarseg_hip.so.

* ``warpFeature``      -- evaluation.py:61-87
* ``resize_flow``      -- the MV resize block, evaluation.py:176-180
* ``EvalConstRes`` / ``EvalAlterRes`` -- evaluation.py:90-144 / 148-215, same call signatures
  (``dl`` is any iterable of the reference's sample tuples).  Networks may be bare modules or
  wrapped in ``nn.DataParallel`` (the reference addresses ``net.module`` on the hot path).
* ``EvalByDistance`` / ``EvalTable`` / ``table_filename`` -- the reference's result table (mIoU at keyframe distance
  0 .. GOP-1 and their mean, evaluation.py:272-303, 308-386, 406-439) from ONE pass: one confusion matrix per distance.
* ``EvalByBand`` / ``BandTable`` / ``label_bands_numpy`` -- the same table split by the distance to the ground truth's label boundaries
  (trimap bands; no reference counterpart), from the same one pass.
* ``EvalByBoundary`` / ``BoundaryTable`` / ``boundary_iou_numpy`` -- Boundary IoU per keyframe distance (the ground truth's band
  intersected with the prediction's; no reference counterpart), from the same one pass.
* ``EvalByContour`` / ``ContourTable`` / ``contour_f_numpy`` -- the contour F-measure per keyframe distance (precision and recall of
  the class contours within a pixel tolerance, the F of DAVIS's J & F; no reference counterpart), from the same one pass.
* ``EvalByCalibration`` / ``CalibrationTable`` / ``calibration_numpy`` -- the reliability table of the 8-bit confidence code per
  keyframe distance (pixels and right pixels per predicted class and code: ECE, MCE, risk-coverage, the threshold for a target
  precision; no reference counterpart), from the same one pass.
* ``alter_res_step_fast`` -- the same non-keyframe step on the kernel-native layouts (int16 MVs in,
  MV resize + warp + CReFF + head fused), used by the GOP runner and bench.py.

The CLI / dataset walking of the reference (evaluation.py:218-439) needs the datasets and
checkpoints and is out of scope.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ops


def _unwrap(net):
    return net.module if hasattr(net, "module") else net


def warpFeature(feature, flow):
    """feature [B,C,H,W] (NCHW-contiguous or channels_last), flow [B,H,W,2] float32/float64 in feature pixels."""
    if ops.is16(feature):                  # 16-bit keyframe feature through the NCHW interface: warp in fp32
        feature = ops.cast(feature, torch.float32)
    if ops.is_nhwc_view(feature) and not feature.is_contiguous():
        return ops.as_nchw(ops.warp(ops.to_nhwc(feature), flow, _lib.NHWC))
    return ops.warp(feature.contiguous(), flow, _lib.NCHW)


def resize_flow(flow, Hp, Wp):
    """evaluation.py:176-180 for a flow [B,H,W,2]: both components are scaled by Hp/H, then bilinear(align_corners=True), in fp64.
    int16 input = the on-disk quarter-pel representation (``flow = int16 / 4``, dataset/camvid.py:625); float32 / float64 input =
    pixels, any values (what the reference's DataLoader hands over).  No host synchronisation."""
    if flow.dtype == torch.int16:
        return ops.mv_resize(flow, Hp, Wp)
    return ops.flow_resize(flow, Hp, Wp)


def _downscale_hw(H, W, scale):
    return int(H * scale), int(W * scale)


class EvalConstRes(object):
    """evaluation.py:90-144."""

    def __init__(self, scale=0.5, ignore_label=255):
        self.ignore_label = ignore_label
        self.scale = scale

    def __call__(self, net, dl, n_classes):
        return _range_safe(lambda: self._run(net, dl, n_classes), dl, n_classes)

    def _run(self, net, dl, n_classes):
        hist = torch.zeros((n_classes, n_classes), dtype=torch.int64, device="cuda")
        for imgs, label, *_ in dl:
            label = label.cuda()
            imgs = imgs.cuda()
            N, C, H, W = imgs.shape
            h, w = _downscale_hw(H, W, self.scale)
            if (h, w) != (H, W):
                imgs = _resize_frames(imgs, h, w)
            logits = net(imgs)[0]
            _, hist = ops.argmax_confusion(logits, label, label.shape[-2], label.shape[-1], hist, self.ignore_label, want_pred=False)
        return hist


def _range_safe_hist(run, dl, reset=None):
    """Runs an evaluation pass (``run()`` returns this rank's confusion matrix); if the split-fp16 convs met an activation outside their
    operand range (the sticky device word of ops.range_tripped -- read once, after the pass, which ends in a host read anyway), the pass is
    repeated on the fp32 matrix-core back end.  With torch.distributed initialised the decision is COLLECTIVE (max of the ranks' flags: a
    rank that did not trip repeats as well, so every rank issues the same collectives); the caller all-reduces the histogram once, from
    the final pass only (evaluation.py:134-135).  A one-shot iterator cannot be replayed: that raises instead of returning a possibly
    clamped result.  Returns the final pass's histogram of this rank."""
    ops.range_tripped()                      # clear what earlier launches left
    hist = run()
    tripped = bool(ops.range_tripped())
    multi = dist.is_available() and dist.is_initialized()
    if multi:
        flag = torch.tensor([1.0 if tripped else 0.0], device=hist.device)
        dist.all_reduce(flag, dist.ReduceOp.MAX)
        tripped = bool(flag.item() > 0)
    if tripped:
        if hasattr(dl, "__next__") or not hasattr(dl, "__iter__"):          # an iterator, not a re-iterable loader
            raise _lib.ArsegError("an activation left the split-fp16 operand range (|x| > 65504) and the data iterator cannot be replayed: "
                                  "evaluate with ops.set_conv_math('f32')")
        if reset is not None:
            reset()                          # per-pass counters start again
        prev = ops.set_conv_math("f32")
        try:
            hist = run()
        finally:
            ops.set_conv_math(prev)
    return hist


def _range_safe(run, dl, n_classes, reset=None):
    return _miou(_range_safe_hist(run, dl, reset), n_classes)


def _resize_frames(imgs, h, w):
    """F.interpolate(imgs, (h,w), bilinear, align_corners=True) on NCHW frames (evaluation.py:115-117)."""
    return ops.resize_nchw(imgs, h, w, _lib.BILINEAR, True)


def _same_frames(a, b):
    """torch.equal for float frames; ingest.DecodedFrames compare their planes (both on the GPU, one host read as before)."""
    if torch.is_tensor(a) and torch.is_tensor(b):
        return torch.equal(a, b)
    return type(a) is type(b) and not torch.is_tensor(a) and a.equal(b)


def _miou(hist, n_classes):
    hist = hist.float()
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(hist, dist.ReduceOp.SUM)                     # evaluation.py:134-135
    ious = hist.diag() / (hist.sum(dim=0) + hist.sum(dim=1) - hist.diag())
    return ious.mean().item()


class EvalAlterRes(object):
    """evaluation.py:148-215: keyframe through the HR net, non-keyframe through the LR net + CReFF.

    ``cache_keyframe`` (extension): the reference recomputes the HR forward of the keyframe for
    every sample (evaluation.py:173) although the 11 non-keyframes of a GOP share it; with the flag set the keyframe feature is
    kept while consecutive samples carry the same reference frame (compared on the GPU).  The result is unchanged -- the HR
    forward is deterministic -- only ~10/11 of the HR forwards disappear when the loader is GOP ordered.  ``hr_forwards``
    counts the ones executed."""

    def __init__(self, scale=0.5, ignore_label=255, cache_keyframe=False):
        self.ignore_label = ignore_label
        self.scale = scale
        self.cache_keyframe = cache_keyframe
        self.hr_forwards = 0

    def __call__(self, highres_net, net, dl, n_classes):
        first = self.hr_forwards

        def reset():
            self.hr_forwards = first

        return _range_safe(lambda: self._run(highres_net, net, dl, n_classes), dl, n_classes, reset)

    def _run(self, highres_net, net, dl, n_classes):
        hist = torch.zeros((n_classes, n_classes), dtype=torch.int64, device="cuda")
        lr_net = _unwrap(net)
        cache = [None, None]
        for imgs, label, _, ref_imgs, flow in dl:
            label = label.cuda()
            out = self._logits(highres_net, lr_net, imgs, ref_imgs, flow, cache)
            _, hist = ops.argmax_confusion(out, label, label.shape[-2], label.shape[-1], hist, self.ignore_label, want_pred=False)
        return hist

    def _logits(self, highres_net, lr_net, imgs, ref_imgs, flow, cache):
        """The loop body up to the logits.  ``cache`` = [reference frames, their HR feature] of the previous sample."""
        imgs = imgs.cuda()
        flow = flow.cuda()
        ref_imgs = ref_imgs.cuda()
        last_ref, last_p = cache
        if self.cache_keyframe and last_ref is not None and last_ref.shape == ref_imgs.shape and _same_frames(last_ref, ref_imgs):
            highres_ref_p = last_p
        else:
            highres_ref_p = highres_net(ref_imgs)[-1]                                     # :173-174
            self.hr_forwards += 1
            cache[0], cache[1] = ref_imgs, highres_ref_p
        flow = resize_flow(flow, highres_ref_p.shape[-2], highres_ref_p.shape[-1])       # :177-180
        highres_ref_p = warpFeature(highres_ref_p, flow)                                 # :183
        N, C, H, W = imgs.shape
        h, w = _downscale_hw(H, W, self.scale)
        if torch.is_tensor(imgs):
            imgs = _resize_frames(imgs, h, w)                                            # :186-188
            out_p = lr_net.forward_phase1(imgs)[-1]                                      # :190-191
        else:                                                                            # 8-bit decoder frames: downscale fused into the ingest
            out_p = ops.as_nchw(lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1])
        out, _ = lr_net.forward_phase2(out_p, highres_ref_p)                             # :193
        return out


class EvalByDistance(EvalAlterRes):
    """The reference's result table from one pass: the mIoU at every keyframe distance d = 0 .. gop-1 (its CLI runs one evaluation per
    distance, evaluation.py:317-376).  ``dl`` yields the reference's sample tuples, of any distance and in any order:

    * ``(imgs, label, _)``: keyframe samples -- through the HR net at scale 1.0 and counted at d = 0 (evaluation.py:358-363);
    * ``(imgs, label, _, ref_imgs, flow, dist)``: EvalAlterRes' sample with the distance(s) appended, an int or an int tensor [N] with
      values 1 .. gop-1 -- EvalAlterRes' loop body, counted at ``dist`` (frames of one batch may differ).

    One [gop, n_cls, n_cls] histogram, all-reduced once under torch.distributed; the operand-range fallback of the other evaluators.
    Returns an ``EvalTable``.  ``cache_keyframe`` / ``hr_forwards`` as in EvalAlterRes (the keyframe feature of non-keyframe samples)."""

    def __init__(self, scale=0.5, ignore_label=255, gop=12, cache_keyframe=False):
        super().__init__(scale, ignore_label, cache_keyframe)
        if gop < 1:
            raise ValueError(f"gop must be positive, got {gop}")
        self.gop = gop

    def __call__(self, highres_net, net, dl, n_classes):
        first = self.hr_forwards

        def reset():
            self.hr_forwards = first

        hist = _range_safe_hist(lambda: self._run(highres_net, net, dl, n_classes), dl, reset)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(hist, dist.ReduceOp.SUM)                 # integer counts: exact
        return EvalTable(hist)

    def _groups(self, d, N):
        if torch.is_tensor(d) and d.is_cuda:                 # stays on the device: no host read (ids outside 0 .. gop-1 count nowhere)
            return d.reshape(-1).to(torch.int32)
        ds = [int(v) for v in d.reshape(-1).tolist()] if torch.is_tensor(d) else [int(d)] * N
        if len(ds) == 1 and N > 1:
            ds = ds * N
        if any(not 1 <= v < self.gop for v in ds):
            raise ValueError(f"keyframe distance of a non-keyframe sample must be in 1 .. {self.gop - 1}, got {ds}")
        return ds

    def _run(self, highres_net, net, dl, n_classes):
        hist = torch.zeros((self.gop, n_classes, n_classes), dtype=torch.int64, device="cuda")
        lr_net = _unwrap(net)
        cache = [None, None]
        for sample in dl:
            label = sample[1].cuda()
            N = label.shape[0]
            if len(sample) == 3:
                out = highres_net(sample[0].cuda())[0]                # EvalConstRes(scale=1.0), evaluation.py:363
                groups = [0] * N
            elif len(sample) == 6:
                imgs, _, _, ref_imgs, flow, d = sample
                out = self._logits(highres_net, lr_net, imgs, ref_imgs, flow, cache)
                groups = self._groups(d, N)
            else:
                raise ValueError(f"EvalByDistance takes (imgs, label, _) or (imgs, label, _, ref_imgs, flow, dist) samples, got {len(sample)} elements")
            _, hist = ops.argmax_confusion_grouped(out, label, groups, self.gop, label.shape[-2], label.shape[-1], hist, self.ignore_label,
                                                   want_pred=False)
        return hist


def table_filename(dataset, backbone, mode, scale, gop, bitrate):
    """File name of the reference's result tables (evaluation.py:299-301 "HR", :382-384 "AR", :435-437 "LR")."""
    if mode not in ("HR", "AR", "LR"):
        raise ValueError(f"mode must be 'HR', 'AR' or 'LR', got {mode!r}")
    tag = "1.0x" if mode == "HR" else f"AR-{scale}x" if mode == "AR" else f"{scale}x"
    return f"{dataset}-{backbone}-{tag}-resolution-exp-GOP{gop}-{bitrate}-evaluation.txt"


def _ious(hist):
    """evaluation.py:136 on one confusion matrix, in float32 (a class absent from label and prediction: 0 / 0 = NaN)."""
    hist = hist.float()
    return hist.diag() / (hist.sum(dim=0) + hist.sum(dim=1) - hist.diag())


class EvalTable(object):
    """mIoU per group (keyframe distance) from a [G, n_cls, n_cls] confusion histogram -- the 13 numbers of the reference's result files
    at G = 12.  Plain torch / numpy; works on CPU tensors.

    ``hist`` the histogram; ``iou`` float32 [G, n_cls]; ``miou`` G Python floats, each what EvalConstRes / EvalAlterRes return on that
    group's samples alone (same float32 arithmetic, NaN where a class is absent from both label and prediction); ``mean`` their float64
    mean as the reference takes it (np.array(mIoU_list).mean(), evaluation.py:298)."""

    def __init__(self, hist):
        hist = torch.as_tensor(hist)
        if hist.dim() != 3 or hist.shape[1] != hist.shape[2]:
            raise ValueError(f"EvalTable takes a [G, n_cls, n_cls] histogram, got {tuple(hist.shape)}")
        self.hist = hist
        ious = [_ious(h) for h in hist]
        self.miou = [i.mean().item() for i in ious]          # on the histogram's device, as _miou does
        self.iou = torch.stack(ious).cpu()

    @property
    def mean(self):
        return np.array(self.miou).mean()

    def as_array(self):
        """The G values and their mean: what the reference writes (evaluation.py:298-303)."""
        return np.array(list(self.miou) + [self.mean])

    def pooled(self, groups=None):
        """mIoU of the summed histogram (``groups``: only these; default all) -- what EvalAlterRes reports for the same samples."""
        if self.hist is None:
            raise ValueError("a table read from a file holds the mIoU values only, not the histogram")
        h = self.hist if groups is None else self.hist[list(groups)]
        return _ious(h.sum(dim=0)).mean().item()

    def save(self, path):
        np.savetxt(path, self.as_array())

    @classmethod
    def load(cls, path):
        """A table written by ``save`` or by the reference: the floats only (``hist`` and ``iou`` are None)."""
        vals = np.atleast_1d(np.loadtxt(path))
        if vals.ndim != 1 or vals.size < 2:
            raise ValueError(f"{path}: expected G mIoU values and their mean, one per line")
        t = cls.__new__(cls)
        t.hist, t.iou, t.miou = None, None, [float(v) for v in vals[:-1]]
        return t


def label_bands_numpy(label, radii, n_cls, ignore_label=255):
    """The host form of ``ops.label_bands``' band plane (include/arseg_hip.h, arseg_label_bands_fwd), numpy only: ``label`` an integer
    array [..., H, W] -> uint8 of the same shape, the band of every pixel (``len(radii)``: interior).  A 3 x 3 minimum and a 3 x 3 maximum
    filter with edge replication, iterated: after r rounds they are the extremes of the clipped (2r+1) x (2r+1) window, and the distance
    of a pixel is the first r at which the two differ."""
    rad = ops.band_radii(radii)
    lab = np.asarray(label)
    if lab.ndim < 2 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"label_bands_numpy takes an integer array [..., H, W], got {lab.dtype} {lab.shape}")
    lab = lab.astype(np.int64)
    lo = np.where((lab >= 0) & (lab < n_cls) & (lab != ignore_label), lab, 255).astype(np.uint8)
    hi = lo

    def spread(a, pick):
        for axis in (-2, -1):
            p = np.concatenate([np.take(a, [0], axis), a, np.take(a, [-1], axis)], axis)
            n = a.shape[axis]
            a = pick(pick(np.take(p, range(0, n), axis), np.take(p, range(1, n + 1), axis)), np.take(p, range(2, n + 2), axis))
        return a

    dist = np.full(lab.shape, rad[-1] + 1, np.int64)
    for r in range(1, rad[-1] + 1):
        lo, hi = spread(lo, np.minimum), spread(hi, np.maximum)
        dist = np.where((dist > r) & (lo != hi), r, dist)
    return np.searchsorted(np.asarray(rad), dist, side="left").astype(np.uint8)


def alter_res_batch_bands(lr_net, ref_ps, imgs, mv_qs, labels, radii, scale=0.5, hist=None, ignore_label=255, groups=None, n_groups=1):
    """``alter_res_batch_pred``'s sibling for the errors' place: the same phases and tail (its pred, without a label), then
    ``ops.label_bands`` of that pred against ``labels`` (int64 [B,H,W]) -> (pred int32 [B,H,W], hist int64
    [n_groups, len(radii) + 1, n_cls, n_cls], accumulated when given).  ``groups`` / ``n_groups`` as ``ops.label_bands`` takes them.
    Nothing comes to the host in between."""
    pred, _ = alter_res_batch_pred(lr_net, ref_ps, imgs, mv_qs, scale=scale)
    n_cls = hist.shape[-1] if hist is not None else _unwrap(lr_net).final_conv.out_channels
    _, hist = ops.label_bands(labels, radii, pred=pred, groups=groups, n_groups=n_groups, n_cls=n_cls, hist=hist, ignore_label=ignore_label)
    return pred, hist


class BandTable(object):
    """mIoU per keyframe distance and boundary band from a [G, n_bands + 1, n_cls, n_cls] histogram (``EvalByBand``): ``hist`` and
    ``radii``; ``band(k)`` the pixels whose distance to a label boundary is in (radii[k-1], radii[k]], ``trimap(k)`` those within
    radii[k] (the bands 0 .. k summed), ``interior()`` those beyond the last radius and ``total()`` all of them -- ``EvalByDistance``'s
    histogram on the same samples --, each an ``EvalTable``.  Plain torch / numpy; works on CPU tensors."""

    def __init__(self, hist, radii):
        hist = torch.as_tensor(hist)
        self.radii = ops.band_radii(radii)
        if hist.dim() != 4 or hist.shape[1] != len(self.radii) + 1 or hist.shape[2] != hist.shape[3]:
            raise ValueError(f"BandTable takes a [G, {len(self.radii) + 1}, n_cls, n_cls] histogram, got {tuple(hist.shape)}")
        self.hist = hist

    def _need_hist(self):
        if self.hist is None:
            raise ValueError("a table read from a file holds the mIoU values only, not the histogram")

    def band(self, k):
        self._need_hist()
        if not 0 <= k < len(self.radii):
            raise IndexError(f"band {k} of {len(self.radii)}")
        return EvalTable(self.hist[:, k])

    def trimap(self, k):
        self._need_hist()
        if not 0 <= k < len(self.radii):
            raise IndexError(f"trimap {k} of {len(self.radii)}")
        return EvalTable(self.hist[:, :k + 1].sum(dim=1))

    def interior(self):
        self._need_hist()
        return EvalTable(self.hist[:, -1])

    def total(self):
        self._need_hist()
        return EvalTable(self.hist.sum(dim=1))

    def as_array(self):
        """[n_bands + 2, G + 1]: the trimaps of width radii[0], radii[1], ..., the interior, the total; each row the G values and their
        mean, as ``EvalTable.as_array``."""
        if self.hist is None:
            return self._array
        rows = [self.trimap(k) for k in range(len(self.radii))] + [self.interior(), self.total()]
        return np.stack([t.as_array() for t in rows])

    def save(self, path):
        np.savetxt(path, self.as_array(), header="radii " + " ".join(str(r) for r in self.radii))

    @classmethod
    def load(cls, path):
        """A table written by ``save``: the radii and the floats only (``hist`` is None; ``as_array`` gives them back)."""
        with open(path) as f:
            head = f.readline().split()
        if head[:2] != ["#", "radii"]:
            raise ValueError(f"{path}: not a BandTable file (no radii line)")
        t = cls.__new__(cls)
        t.radii = ops.band_radii(head[2:])
        vals = np.atleast_2d(np.loadtxt(path))
        if vals.shape[0] != len(t.radii) + 2 or vals.shape[1] < 2:
            raise ValueError(f"{path}: expected {len(t.radii) + 2} rows of G mIoU values and their mean, got {vals.shape}")
        t.hist, t._array = None, vals
        return t


class EvalByBand(EvalByDistance):
    """``EvalByDistance`` with the place of the errors: the same samples, keyframe handling (d = 0 through the HR net) and operand-range
    fallback, one pass, and per keyframe distance one confusion matrix per band of distance to the ground truth's label boundaries
    (``radii``, in pixels; include/arseg_hip.h, arseg_label_bands_fwd).  One [gop, len(radii) + 1, n_cls, n_cls] histogram, all-reduced
    once under torch.distributed.  Returns a ``BandTable``, whose ``total()`` is ``EvalByDistance``'s table on the same samples."""

    def __init__(self, scale=0.5, ignore_label=255, gop=12, cache_keyframe=False, radii=(1, 2, 4, 8)):
        super().__init__(scale, ignore_label, gop, cache_keyframe)
        self.radii = ops.band_radii(radii)

    def __call__(self, highres_net, net, dl, n_classes):
        first = self.hr_forwards

        def reset():
            self.hr_forwards = first

        hist = _range_safe_hist(lambda: self._run(highres_net, net, dl, n_classes), dl, reset)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(hist, dist.ReduceOp.SUM)                 # integer counts: exact
        return BandTable(hist, self.radii)

    def _run(self, highres_net, net, dl, n_classes):
        hist = torch.zeros((self.gop, len(self.radii) + 1, n_classes, n_classes), dtype=torch.int64, device="cuda")
        lr_net = _unwrap(net)
        cache = [None, None]
        for sample in dl:
            label = sample[1].cuda()
            N = label.shape[0]
            if len(sample) == 3:
                out = highres_net(sample[0].cuda())[0]
                groups = [0] * N
            elif len(sample) == 6:
                imgs, _, _, ref_imgs, flow, d = sample
                out = self._logits(highres_net, lr_net, imgs, ref_imgs, flow, cache)
                groups = self._groups(d, N)
            else:
                raise ValueError(f"EvalByBand takes (imgs, label, _) or (imgs, label, _, ref_imgs, flow, dist) samples, got {len(sample)} elements")
            pred, _ = ops.argmax_confusion_grouped(out, None, groups, self.gop, label.shape[-2], label.shape[-1])
            ops.label_bands(label, self.radii, pred=pred, groups=groups, n_groups=self.gop, n_cls=n_classes, hist=hist,
                            ignore_label=self.ignore_label)
        return hist


def boundary_iou_numpy(label, pred, radii, n_cls, ignore_label=255, border=True):
    """The host form of ``ops.boundary_iou``'s counts (include/arseg_hip.h, arseg_boundary_iou_fwd), numpy only and written the paper's
    way: ``label`` and ``pred`` integer arrays [..., H, W] -> int64 [3, len(radii) + 1, n_cls], the frames summed.  Per class the mask
    of the ground truth and that of the prediction, each minus its d-fold 3 x 3 erosion (zero-padded with ``border``, edge-replicated
    without), restricted to the pixels that count, give the inner bands of width d = radii[k] and their intersection; differences of
    consecutive widths give the disjoint bands, the whole masks the last one."""
    rad = ops.boundary_radii(radii)
    lab, prd = np.asarray(label), np.asarray(pred)
    if lab.ndim < 2 or lab.shape != prd.shape or not np.issubdtype(lab.dtype, np.integer) or not np.issubdtype(prd.dtype, np.integer):
        raise ValueError(f"boundary_iou_numpy takes two integer arrays [..., H, W] of one shape, got {lab.dtype} {lab.shape} and {prd.dtype} {prd.shape}")
    lab, prd = lab.astype(np.int64), prd.astype(np.int64)
    lab = np.where((lab >= 0) & (lab < n_cls) & (lab != ignore_label), lab, 255)
    prd = np.where((prd >= 0) & (prd < n_cls), prd, 255)
    counting = (lab != 255) & (prd != 255)

    def erode(m):
        for axis in (-2, -1):
            n = m.shape[axis]
            first, last = np.take(m, [0], axis), np.take(m, [-1], axis)
            if border:
                first, last = np.zeros_like(first), np.zeros_like(last)
            p = np.concatenate([first, m, last], axis)
            m = np.take(p, range(0, n), axis) & np.take(p, range(1, n + 1), axis) & np.take(p, range(2, n + 2), axis)
        return m

    def sizes(g, p):
        g, p = g & counting, p & counting
        return np.array([g.sum(), p.sum(), (g & p).sum()], np.int64)

    out = np.zeros((3, len(rad) + 1, n_cls), np.int64)
    for c in range(n_cls):
        g, p = lab == c, prd == c
        eg, ep, d, before = g, p, 0, np.zeros(3, np.int64)
        for k, r in enumerate(rad):
            while d < r:
                eg, ep, d = erode(eg), erode(ep), d + 1
            within = sizes(g & ~eg, p & ~ep)
            out[:, k, c], before = within - before, within
        out[:, len(rad), c] = sizes(g, p) - before
    return out


def alter_res_batch_boundary(lr_net, ref_ps, imgs, mv_qs, labels, radii, scale=0.5, counts=None, ignore_label=255, groups=None, n_groups=1,
                             border=True):
    """``alter_res_batch_pred``'s sibling for Boundary IoU: the same phases and tail (its pred, without a label), then
    ``ops.boundary_iou`` of that pred against ``labels`` (int64 [B,H,W]) -> (pred int32 [B,H,W], counts int64
    [n_groups, 3, len(radii) + 1, n_cls], accumulated when given).  ``groups`` / ``n_groups`` as ``ops.boundary_iou`` takes them.
    Nothing comes to the host in between."""
    pred, _ = alter_res_batch_pred(lr_net, ref_ps, imgs, mv_qs, scale=scale)
    n_cls = counts.shape[-1] if counts is not None else _unwrap(lr_net).final_conv.out_channels
    counts, _, _ = ops.boundary_iou(labels, pred, radii, groups=groups, n_groups=n_groups, n_cls=n_cls, counts=counts, ignore_label=ignore_label,
                                    border=border)
    return pred, counts


class BoundaryTable(object):
    """Boundary IoU per keyframe distance from a [G, 3, n_bands + 1, n_cls] tensor of counts (``EvalByBoundary``, ``ops.boundary_iou``):
    ``counts``, ``radii`` and ``border``.  ``boundary_iou(k)`` float32 [G, n_cls], the Boundary IoU at width radii[k] (the bands 0 .. k
    summed; I / (G + P - I) in ``EvalTable``'s float32 arithmetic, 0 / 0 = NaN); ``iou()`` all bands summed -- ``EvalByDistance``'s
    ``EvalTable.iou`` on the same samples; ``miou(k)`` the G class means as Python floats (``k=None``: of ``iou()``) and ``mean(k)`` their
    float64 mean as ``EvalTable`` takes it.  Plain torch / numpy; works on CPU tensors."""

    def __init__(self, counts, radii, border=True):
        counts = torch.as_tensor(counts)
        self.radii = ops.boundary_radii(radii)
        self.border = bool(border)
        if counts.dim() != 4 or counts.shape[1] != 3 or counts.shape[2] != len(self.radii) + 1:
            raise ValueError(f"BoundaryTable takes [G, 3, {len(self.radii) + 1}, n_cls] counts, got {tuple(counts.shape)}")
        self.counts = counts

    def _need_counts(self):
        if self.counts is None:
            raise ValueError("a table read from a file holds the mean values only, not the counts")

    def _ratio(self, upto):
        c = self.counts[:, :, :upto].sum(dim=2).float()
        return c[:, 2] / (c[:, 0] + c[:, 1] - c[:, 2])

    def boundary_iou(self, k):
        self._need_counts()
        if not 0 <= k < len(self.radii):
            raise IndexError(f"radius {k} of {len(self.radii)}")
        return self._ratio(k + 1).cpu()

    def iou(self):
        self._need_counts()
        return self._ratio(len(self.radii) + 1).cpu()

    def miou(self, k=None):
        self._need_counts()
        if k is not None and not 0 <= k < len(self.radii):
            raise IndexError(f"radius {k} of {len(self.radii)}")
        ious = self._ratio(len(self.radii) + 1 if k is None else k + 1)
        return [i.mean().item() for i in ious]               # on the counts' device, as EvalTable does

    def mean(self, k=None):
        return np.array(self.miou(k)).mean()

    def as_array(self):
        """[n_bands + 1, G + 1]: the mean Boundary IoU at radii[0], radii[1], ..., then the plain mIoU; each row the G values and their
        mean, as ``EvalTable.as_array``."""
        if self.counts is None:
            return self._array
        rows = [self.miou(k) for k in range(len(self.radii))] + [self.miou()]
        return np.stack([np.array(list(r) + [np.array(r).mean()]) for r in rows])

    def save(self, path):
        np.savetxt(path, self.as_array(), header="radii " + " ".join(str(r) for r in self.radii) + f" border {int(self.border)}")

    @classmethod
    def load(cls, path):
        """A table written by ``save``: the radii, the border flag and the floats only (``counts`` is None; ``as_array`` gives them back)."""
        with open(path) as f:
            head = f.readline().split()
        if head[:2] != ["#", "radii"] or len(head) < 5 or head[-2] != "border" or head[-1] not in ("0", "1"):
            raise ValueError(f"{path}: not a BoundaryTable file (no radii ... border line)")
        t = cls.__new__(cls)
        t.radii, t.border = ops.boundary_radii(head[2:-2]), head[-1] == "1"
        vals = np.atleast_2d(np.loadtxt(path))
        if vals.shape[0] != len(t.radii) + 1 or vals.shape[1] < 2:
            raise ValueError(f"{path}: expected {len(t.radii) + 1} rows of G mean values and their mean, got {vals.shape}")
        t.counts, t._array = None, vals
        return t


class EvalByBoundary(EvalByDistance):
    """``EvalByDistance`` with Boundary IoU (Cheng et al., CVPR 2021): the same samples, keyframe handling (d = 0 through the HR net) and
    operand-range fallback, one pass, and per keyframe distance the counts of ``ops.boundary_iou`` (include/arseg_hip.h,
    arseg_boundary_iou_fwd).  ``radii`` in pixels; None takes ``ops.boundary_radius`` of the first label's size, the paper's 2 % of the
    diagonal.  One [gop, 3, len(radii) + 1, n_cls] tensor, all-reduced once under torch.distributed.  Returns a ``BoundaryTable``, whose
    ``iou()`` is ``EvalByDistance``'s table on the same samples."""

    def __init__(self, scale=0.5, ignore_label=255, gop=12, cache_keyframe=False, radii=None, border=True):
        super().__init__(scale, ignore_label, gop, cache_keyframe)
        self.radii = None if radii is None else ops.boundary_radii(radii)
        self.border = bool(border)

    def __call__(self, highres_net, net, dl, n_classes):
        first = self.hr_forwards
        used = [self.radii]

        def reset():
            self.hr_forwards = first

        counts = _range_safe_hist(lambda: self._run(highres_net, net, dl, n_classes, used), dl, reset)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(counts, dist.ReduceOp.SUM)               # integer counts: exact
        return BoundaryTable(counts, used[0], self.border)

    def _run(self, highres_net, net, dl, n_classes, used):
        counts = None
        lr_net = _unwrap(net)
        cache = [None, None]
        for sample in dl:
            label = sample[1].cuda()
            N = label.shape[0]
            if counts is None:
                if used[0] is None:
                    used[0] = ops.boundary_radii((ops.boundary_radius(label.shape[-2], label.shape[-1]),))    # above 64: refused
                counts = torch.zeros((self.gop, 3, len(used[0]) + 1, n_classes), dtype=torch.int64, device="cuda")
            if len(sample) == 3:
                out = highres_net(sample[0].cuda())[0]
                groups = [0] * N
            elif len(sample) == 6:
                imgs, _, _, ref_imgs, flow, d = sample
                out = self._logits(highres_net, lr_net, imgs, ref_imgs, flow, cache)
                groups = self._groups(d, N)
            else:
                raise ValueError(f"EvalByBoundary takes (imgs, label, _) or (imgs, label, _, ref_imgs, flow, dist) samples, got {len(sample)} elements")
            pred, _ = ops.argmax_confusion_grouped(out, None, groups, self.gop, label.shape[-2], label.shape[-1])
            ops.boundary_iou(label, pred, used[0], groups=groups, n_groups=self.gop, n_cls=n_classes, counts=counts,
                             ignore_label=self.ignore_label, border=self.border)
        if counts is None:
            raise ValueError("EvalByBoundary: the loader gave no sample")
        return counts


def contour_f_numpy(label, pred, radii, n_cls, ignore_label=255):
    """The host form of ``ops.contour_f``'s counts (include/arseg_hip.h, arseg_contour_f_fwd), numpy only and written the published way
    (the dilation of DAVIS's F-measure, the distance threshold of bfscore): ``label`` and ``pred`` integer arrays [..., H, W] -> int64
    [2, len(radii) + 1, n_cls], the frames summed.  Per class the contour map of each plane (the class's pixels with another class among
    their 8 neighbours), dilated by the disc dx^2 + dy^2 <= r^2 through shifted ORs and ANDed with the other plane's contours, gives the
    contour pixels matched within r; differences of consecutive radii give the disjoint bands, the whole contour the last one."""
    rad = ops.contour_radii(radii)
    lab, prd = np.asarray(label), np.asarray(pred)
    if lab.ndim < 2 or lab.shape != prd.shape or not np.issubdtype(lab.dtype, np.integer) or not np.issubdtype(prd.dtype, np.integer):
        raise ValueError(f"contour_f_numpy takes two integer arrays [..., H, W] of one shape, got {lab.dtype} {lab.shape} and {prd.dtype} {prd.shape}")
    lab, prd = lab.astype(np.int64), prd.astype(np.int64)
    lab = np.where((lab >= 0) & (lab < n_cls) & (lab != ignore_label), lab, 255)
    prd = np.where((prd >= 0) & (prd < n_cls), prd, 255)
    counting = (lab != 255) & (prd != 255)
    H, W = lab.shape[-2:]

    def shifted(m, dy, dx):
        """m moved by (dy, dx): out[y, x] = m[y - dy, x - dx], False where that is outside the image."""
        out = np.zeros_like(m)
        if abs(dy) < H and abs(dx) < W:
            out[..., max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = m[..., max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
        return out

    def contour(plane, c):
        other = (plane != c) & (plane != 255)
        near = np.zeros_like(other)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near |= shifted(other, dy, dx)
        return (plane == c) & near

    def dilated(m, r):
        out = np.zeros_like(m)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy * dy + dx * dx <= r * r:
                    out |= shifted(m, dy, dx)
        return out

    out = np.zeros((2, len(rad) + 1, n_cls), np.int64)
    for c in range(n_cls):
        cg, cp = contour(lab, c), contour(prd, c)
        if not cg.any() and not cp.any():
            continue
        before = np.zeros(2, np.int64)
        for k, r in enumerate(rad):
            within = np.array([(cg & dilated(cp, r) & counting).sum(), (cp & dilated(cg, r) & counting).sum()], np.int64)
            out[:, k, c], before = within - before, within
        out[:, len(rad), c] = np.array([(cg & counting).sum(), (cp & counting).sum()], np.int64) - before
    return out


def alter_res_batch_contour(lr_net, ref_ps, imgs, mv_qs, labels, radii, scale=0.5, counts=None, ignore_label=255, groups=None, n_groups=1):
    """``alter_res_batch_pred``'s sibling for the contour F-measure: the same phases and tail (its pred, without a label), then
    ``ops.contour_f`` of that pred against ``labels`` (int64 [B,H,W]) -> (pred int32 [B,H,W], counts int64
    [n_groups, 2, len(radii) + 1, n_cls], accumulated when given).  ``groups`` / ``n_groups`` as ``ops.contour_f`` takes them.
    Nothing comes to the host in between."""
    pred, _ = alter_res_batch_pred(lr_net, ref_ps, imgs, mv_qs, scale=scale)
    n_cls = counts.shape[-1] if counts is not None else _unwrap(lr_net).final_conv.out_channels
    counts, _, _ = ops.contour_f(labels, pred, radii, groups=groups, n_groups=n_groups, n_cls=n_cls, counts=counts, ignore_label=ignore_label)
    return pred, counts


class ContourTable(object):
    """Contour precision, recall and F per keyframe distance from a [G, 2, n_bands + 1, n_cls] tensor of counts (``EvalByContour``,
    ``ops.contour_f``): ``counts`` and ``radii``.  ``recall(k)`` / ``precision(k)`` float32 [G, n_cls]: the contour pixels of the ground
    truth / of the prediction matched within radii[k] (the bands 0 .. k summed) over all of them, in ``EvalTable``'s float32 arithmetic,
    0 / 0 = NaN (the class has no contour on that plane); ``f(k)`` = 2 P R / (P + R), NaN where P or R is, 0 where P + R == 0;
    ``mean_f(k)`` the G class means as Python floats and ``mean(k)`` their float64 mean as ``EvalTable`` takes it.  The means are plain
    means, as the sibling tables': a group's ``mean_f(k)`` is NaN as soon as ONE class has no contour on either plane in that group, and
    then so are ``mean(k)`` and that entry of every row of ``as_array()`` -- with rare classes at a keyframe distance, read ``f(k)`` and
    average the classes that are there (``torch.nanmean(table.f(k), dim=1)``).  Plain torch / numpy; works on CPU tensors."""

    def __init__(self, counts, radii):
        counts = torch.as_tensor(counts)
        self.radii = ops.contour_radii(radii)
        if counts.dim() != 4 or counts.shape[1] != 2 or counts.shape[2] != len(self.radii) + 1:
            raise ValueError(f"ContourTable takes [G, 2, {len(self.radii) + 1}, n_cls] counts, got {tuple(counts.shape)}")
        self.counts = counts

    def _ratio(self, row, k):
        if self.counts is None:
            raise ValueError("a table read from a file holds the mean values only, not the counts")
        if not 0 <= k < len(self.radii):
            raise IndexError(f"radius {k} of {len(self.radii)}")
        c = self.counts[:, row]
        return c[:, :k + 1].sum(dim=1).float() / c.sum(dim=1).float()

    def _f(self, k):
        p, r = self._ratio(1, k), self._ratio(0, k)
        f = 2 * p * r / (p + r)
        return torch.where((p + r) == 0, torch.zeros_like(f), f)             # 0 / 0 here is "nothing matched", not "no contour"

    def precision(self, k):
        return self._ratio(1, k).cpu()

    def recall(self, k):
        return self._ratio(0, k).cpu()

    def f(self, k):
        return self._f(k).cpu()

    def mean_f(self, k):
        return [f.mean().item() for f in self._f(k)]                          # on the counts' device, as EvalTable does

    def mean(self, k):
        return np.array(self.mean_f(k)).mean()

    def as_array(self):
        """[n_bands, G + 1]: the mean F at radii[0], radii[1], ...; each row the G values and their mean, as ``EvalTable.as_array``."""
        if self.counts is None:
            return self._array
        rows = [self.mean_f(k) for k in range(len(self.radii))]
        return np.stack([np.array(list(r) + [np.array(r).mean()]) for r in rows])

    def save(self, path):
        np.savetxt(path, self.as_array(), header="contour radii " + " ".join(str(r) for r in self.radii))

    @classmethod
    def load(cls, path):
        """A table written by ``save``: the radii and the floats only (``counts`` is None; ``as_array`` gives them back)."""
        with open(path) as f:
            head = f.readline().split()
        if head[:3] != ["#", "contour", "radii"] or len(head) < 4:
            raise ValueError(f"{path}: not a ContourTable file (no contour radii line)")
        t = cls.__new__(cls)
        t.radii = ops.contour_radii(head[3:])
        vals = np.atleast_2d(np.loadtxt(path))
        if vals.shape[0] != len(t.radii) or vals.shape[1] < 2:
            raise ValueError(f"{path}: expected {len(t.radii)} rows of G mean values and their mean, got {vals.shape}")
        t.counts, t._array = None, vals
        return t


class EvalByContour(EvalByDistance):
    """``EvalByDistance`` with the contour F-measure: the same samples, keyframe handling (d = 0 through the HR net) and operand-range
    fallback, one pass, and per keyframe distance the counts of ``ops.contour_f`` (include/arseg_hip.h, arseg_contour_f_fwd).  ``radii``
    in pixels; None takes ``ops.contour_radius`` of the first label's size, DAVIS's 0.8 % of the diagonal.  One
    [gop, 2, len(radii) + 1, n_cls] tensor, all-reduced once under torch.distributed.  Returns a ``ContourTable``."""

    def __init__(self, scale=0.5, ignore_label=255, gop=12, cache_keyframe=False, radii=None):
        super().__init__(scale, ignore_label, gop, cache_keyframe)
        self.radii = None if radii is None else ops.contour_radii(radii)

    def __call__(self, highres_net, net, dl, n_classes):
        first = self.hr_forwards
        used = [self.radii]

        def reset():
            self.hr_forwards = first

        counts = _range_safe_hist(lambda: self._run(highres_net, net, dl, n_classes, used), dl, reset)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(counts, dist.ReduceOp.SUM)               # integer counts: exact
        return ContourTable(counts, used[0])

    def _run(self, highres_net, net, dl, n_classes, used):
        counts = None
        lr_net = _unwrap(net)
        cache = [None, None]
        for sample in dl:
            label = sample[1].cuda()
            N = label.shape[0]
            if counts is None:
                if used[0] is None:
                    used[0] = ops.contour_radii((ops.contour_radius(label.shape[-2], label.shape[-1]),))      # above 32: refused
                counts = torch.zeros((self.gop, 2, len(used[0]) + 1, n_classes), dtype=torch.int64, device="cuda")
            if len(sample) == 3:
                out = highres_net(sample[0].cuda())[0]
                groups = [0] * N
            elif len(sample) == 6:
                imgs, _, _, ref_imgs, flow, d = sample
                out = self._logits(highres_net, lr_net, imgs, ref_imgs, flow, cache)
                groups = self._groups(d, N)
            else:
                raise ValueError(f"EvalByContour takes (imgs, label, _) or (imgs, label, _, ref_imgs, flow, dist) samples, got {len(sample)} elements")
            pred, _ = ops.argmax_confusion_grouped(out, None, groups, self.gop, label.shape[-2], label.shape[-1])
            ops.contour_f(label, pred, used[0], groups=groups, n_groups=self.gop, n_cls=n_classes, counts=counts, ignore_label=self.ignore_label)
        if counts is None:
            raise ValueError("EvalByContour: the loader gave no sample")
        return counts


_CAL_KINDS = ("top1", "margin")


def calibration_numpy(logits, label, H, W, n_cls, groups=None, n_groups=1, ignore_label=255, kind="top1", align_corners=True):
    """The host form of ``ops.calibration`` (include/arseg_hip.h, arseg_calibration_fwd), written from the contract in float64 with numpy
    and torch on the CPU: fp32 ``logits`` [N,n_cls,h,w] -> F.interpolate(bilinear, ``align_corners``) -> per pixel the class k* (the first
    maximum; a NaN counts as the maximum) and the code q = floor(255 c + 0.5) of the softmax's top-1 probability (``kind="top1"``) or of
    its margin over the runner-up (``"margin"``), 0 where c is NaN; ``label`` an integer array [N,H,W] -> int64 [n_groups, n_cls, 256, 2]:
    the pixels with 0 <= label < n_cls and label != ``ignore_label`` of the frames of group g at [g][k*][q][0], those with label == k*
    at [g][k*][q][1].  ``groups``: one id per frame (a frame whose id is outside [0, n_groups) counts nowhere), None with one group.
    float64 decides a pixel within fp32 rounding of a tie or of a code boundary its own way: the GPU tests hold the kernel to the
    confidence launch's planes, and those to this arithmetic under tests/confidence_oracle.py's rule."""
    import torch.nn.functional as F

    x = np.asarray(logits)
    lab = np.asarray(label)
    H, W = int(H), int(W)
    if kind not in _CAL_KINDS:
        raise ValueError(f"calibration_numpy: kind is 'top1' or 'margin', got {kind!r}")
    if x.ndim != 4 or x.shape[1] != n_cls or not 1 <= n_cls <= 32:
        raise ValueError(f"calibration_numpy takes logits [N, n_cls, h, w] with 1..32 classes, got {x.shape} for n_cls = {n_cls}")
    if lab.shape != (x.shape[0], H, W) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"calibration_numpy takes integer labels {(x.shape[0], H, W)}, got {lab.dtype} {lab.shape}")
    if n_groups < 1 or (groups is None and n_groups != 1):
        raise ValueError(f"calibration_numpy: groups=None needs n_groups == 1, got {n_groups}")
    ids = [0] * x.shape[0] if groups is None else [int(g) for g in groups]
    if len(ids) != x.shape[0]:
        raise ValueError(f"groups names {len(ids)} frames, the batch has {x.shape[0]}")
    v = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).double()
    if tuple(v.shape[-2:]) != (H, W):
        v = F.interpolate(v, size=(H, W), mode="bilinear", align_corners=bool(align_corners))
    v = v.numpy()
    isn = np.isnan(v)
    k = np.where(isn.any(axis=1), isn.argmax(axis=1), np.where(isn, -np.inf, v).argmax(axis=1))
    with np.errstate(all="ignore"):
        e = np.exp(v - v.max(axis=1, keepdims=True))
        p = np.sort(e / e.sum(axis=1, keepdims=True), axis=1)                  # a NaN anywhere makes the whole pixel NaN
        c = p[:, -1] - (p[:, -2] if kind == "margin" and n_cls > 1 else 0.0)
        q = np.where(np.isnan(c), 0.0, np.floor(255.0 * c + 0.5)).astype(np.int64)
    lab = lab.astype(np.int64)
    counting = (lab >= 0) & (lab < n_cls) & (lab != ignore_label)
    out = np.zeros((n_groups, n_cls * 256 * 2), np.int64)
    for n, g in enumerate(ids):
        if 0 <= g < n_groups:
            m = counting[n]
            key = (k[n][m] * 256 + q[n][m]) * 2
            out[g] += np.bincount(key, minlength=n_cls * 512) + np.bincount(key[lab[n][m] == k[n][m]] + 1, minlength=n_cls * 512)
    return out.reshape(n_groups, n_cls, 256, 2)


class CalibrationTable(object):
    """Calibration of the 8-bit confidence code per keyframe distance from a [G, n_cls, 256, 2] tensor of counts (``EvalByCalibration``,
    ``ops.calibration``): ``cal[g][k][q]`` = (pixels predicted k with code q, those of them that were right); ``kind`` the confidence the
    codes stand for ("top1" or "margin").  Everything here is arithmetic on those integers: sums in int64, ratios in ``EvalTable``'s
    float32, 0 / 0 = NaN (a group, class or bin without pixels).  The confidence of a pixel is its code / 255: the codes are the
    confidence rounded to 8 bits, so the mean confidence of a bin is within 0.5 / 255 of the fp32 one, and so are ECE and MCE (the bin a
    pixel falls into is decided by its code: ``bin(q) = q * n_bins // 256``).  Plain torch / numpy; works on CPU tensors.

    ``counts(per_class=False)`` int64 [G, 256, 2] (or the [G, n_cls, 256, 2] tensor itself); ``accuracy()`` / ``confidence()`` float32
    [G]; ``reliability(n_bins)`` -> (confidence, accuracy, weight), each [G, n_bins]; ``ece`` / ``mce`` / ``classwise_ece`` [G];
    ``risk_coverage()`` -> (coverage, selective accuracy), each [G, 256], entry t keeping the pixels with q >= t; ``accuracy_below(low)``
    [G]: the accuracy of the pixels ``egress.DriftMonitor``'s ``low`` flags (q < low); ``threshold_for(accuracy)`` int64 [G]: the
    smallest t whose kept pixels reach that accuracy, 256 if none does; ``pooled()`` the table of all groups together."""

    def __init__(self, cal, kind="top1"):
        cal = torch.as_tensor(cal)
        if cal.dim() != 4 or cal.shape[2] != 256 or cal.shape[3] != 2 or cal.dtype.is_floating_point:
            raise ValueError(f"CalibrationTable takes integer [G, n_cls, 256, 2] counts, got {cal.dtype} {tuple(cal.shape)}")
        if kind not in _CAL_KINDS:
            raise ValueError(f"CalibrationTable: kind is 'top1' or 'margin', got {kind!r}")
        self.cal = cal.long()
        self.kind = kind

    def counts(self, per_class=False):
        return self.cal if per_class else self.cal.sum(dim=1)

    @staticmethod
    def _codes(c):
        return torch.arange(256, dtype=torch.int64, device=c.device)

    def accuracy(self):
        c = self.counts()
        return (c[..., 1].sum(dim=-1).float() / c[..., 0].sum(dim=-1).float()).cpu()

    def confidence(self):
        n = self.counts()[..., 0]
        return ((n * self._codes(n)).sum(dim=-1).float() / (255 * n.sum(dim=-1)).float()).cpu()

    @staticmethod
    def _n_bins(n_bins):
        n_bins = int(n_bins)
        if not 1 <= n_bins <= 256:
            raise ValueError(f"n_bins must be in 1..256, got {n_bins}")
        return n_bins

    def _binned(self, c, n_bins):
        """counts [..., 256, 2] -> (confidence, accuracy, weight) [..., n_bins]"""
        q = self._codes(c)
        index = (q * n_bins // 256).expand(c.shape[:-1])
        zero = torch.zeros(c.shape[:-2] + (n_bins,), dtype=torch.int64, device=c.device)
        n = zero.scatter_add(-1, index, c[..., 0])
        right = zero.scatter_add(-1, index, c[..., 1])
        qn = zero.scatter_add(-1, index, c[..., 0] * q)
        return qn.float() / (255 * n).float(), right.float() / n.float(), n.float() / n.sum(dim=-1, keepdim=True).float()

    def reliability(self, n_bins=15):
        return tuple(t.cpu() for t in self._binned(self.counts(), self._n_bins(n_bins)))

    @staticmethod
    def _ece(conf, acc, weight):
        gap = torch.where(weight > 0, (acc - conf).abs() * weight, torch.zeros_like(weight))          # an empty bin: NaN x 0
        return torch.where(weight.isnan().any(dim=-1), torch.full_like(gap[..., 0], float("nan")), gap.sum(dim=-1))

    def ece(self, n_bins=15):
        return self._ece(*self._binned(self.counts(), self._n_bins(n_bins))).cpu()

    def mce(self, n_bins=15):
        conf, acc, weight = self._binned(self.counts(), self._n_bins(n_bins))
        gap = torch.where(weight > 0, (acc - conf).abs(), torch.full_like(weight, -1.0)).max(dim=-1).values
        return torch.where(gap < 0, torch.full_like(gap, float("nan")), gap).cpu()

    def classwise_ece(self, n_bins=15):
        """The mean over the predicted classes present in a group of the ECE within the pixels predicted that class."""
        per = self._ece(*self._binned(self.cal, self._n_bins(n_bins)))                                  # [G, n_cls], NaN: class not predicted
        there = ~per.isnan()
        return (torch.where(there, per, torch.zeros_like(per)).sum(dim=1) / there.sum(dim=1).float()).cpu()

    def risk_coverage(self):
        c = self.counts()
        kept = c.flip(-2).cumsum(dim=-2).flip(-2)                                                       # [G, 256, 2]: q >= t
        return (kept[..., 0].float() / c[..., 0].sum(dim=-1, keepdim=True).float()).cpu(), (kept[..., 1].float() / kept[..., 0].float()).cpu()

    def accuracy_below(self, low):
        low = int(low)
        if not 0 <= low <= 256:
            raise ValueError(f"low is a code threshold in 0..256, got {low}")
        c = self.counts()[:, :low].sum(dim=1)
        return (c[:, 1].float() / c[:, 0].float()).cpu()

    def threshold_for(self, accuracy):
        _, sel = self.risk_coverage()
        ok = sel >= float(accuracy)                                                                     # NaN (nothing kept) compares False
        first = torch.where(ok, self._codes(ok).expand_as(ok), torch.full_like(ok, 256, dtype=torch.int64))
        return first.min(dim=-1).values

    def pooled(self):
        return CalibrationTable(self.cal.sum(dim=0, keepdim=True), self.kind)

    def save(self, path):
        """The counts and the kind as .npz (the integers, so every figure can be recomputed)."""
        with open(path, "wb") as f:
            np.savez_compressed(f, cal=self.cal.cpu().numpy(), kind=np.array(self.kind))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if "cal" not in z or "kind" not in z:
                raise ValueError(f"{path}: not a CalibrationTable file (no cal / kind arrays)")
            return cls(torch.from_numpy(z["cal"]), str(z["kind"]))


class EvalByCalibration(EvalByDistance):
    """``EvalByDistance`` with the reliability table of the confidence code: the same samples, keyframe handling (d = 0 through the HR net)
    and operand-range fallback, one pass, and per keyframe distance the counts of ``ops.calibration`` (include/arseg_hip.h,
    arseg_calibration_fwd) from the logits the distance evaluator's tail would have taken -- does a code of 200 at distance 9 mean what it
    means at distance 1?  ``kind``: "top1" or "margin".  One [gop, n_cls, 256, 2] tensor, all-reduced once under torch.distributed.
    Returns a ``CalibrationTable``."""

    def __init__(self, scale=0.5, ignore_label=255, gop=12, cache_keyframe=False, kind="top1"):
        super().__init__(scale, ignore_label, gop, cache_keyframe)
        if kind not in _CAL_KINDS:
            raise ValueError(f"EvalByCalibration: kind is 'top1' or 'margin', got {kind!r}")
        self.kind = kind

    def __call__(self, highres_net, net, dl, n_classes):
        first = self.hr_forwards

        def reset():
            self.hr_forwards = first

        cal = _range_safe_hist(lambda: self._run(highres_net, net, dl, n_classes), dl, reset)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(cal, dist.ReduceOp.SUM)                  # integer counts: exact
        return CalibrationTable(cal, self.kind)

    def _run(self, highres_net, net, dl, n_classes):
        cal = torch.zeros((self.gop, n_classes, 256, 2), dtype=torch.int64, device="cuda")
        lr_net = _unwrap(net)
        cache = [None, None]
        for sample in dl:
            label = sample[1].cuda()
            N = label.shape[0]
            if len(sample) == 3:
                out = highres_net(sample[0].cuda())[0]
                groups = [0] * N
            elif len(sample) == 6:
                imgs, _, _, ref_imgs, flow, d = sample
                out = self._logits(highres_net, lr_net, imgs, ref_imgs, flow, cache)
                groups = self._groups(d, N)
            else:
                raise ValueError(f"EvalByCalibration takes (imgs, label, _) or (imgs, label, _, ref_imgs, flow, dist) samples, got {len(sample)} elements")
            ops.calibration(out.contiguous(), label, label.shape[-2], label.shape[-1], groups=groups, n_groups=self.gop, cal=cal, ignore_label=self.ignore_label,
                            kind=self.kind)
        return cal


def alter_res_step_fast(lr_net, ref_p_nhwc, img, mv_q, scale=0.5):
    """One non-keyframe on the kernel-native layouts.

    ref_p_nhwc: keyframe feature, NHWC [N,Hp,Wp,C] (unwarped); img: NCHW frame; mv_q: int16 quarter-pel [N,H,W,2].
    Returns (logits NCHW, p in C8 layout).  Same arithmetic as EvalAlterRes' loop body; the frame downscale is fused
    into the NHWC4 ingest, the MV resize into the warp, and everything after the backbone into one CReFF kernel.
    """
    lr_net = _unwrap(lr_net)
    N, C, H, W = img.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(img, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]     # a3 + phase 1
    return lr_net.phase2_warp(feat, [ref_p_nhwc[i] for i in range(N)], mv_q)      # a2 + a1 + CReFF + head


def alter_res_batch_fast(lr_net, ref_ps, imgs, mv_qs, scale=0.5):
    """B non-keyframes in one pass (they have no dependence on each other, evaluation.py:161-193, so the LR backbone
    and CReFF run batched: large GEMM M, one launch sequence for the whole batch).

    ref_ps: sequence of B un-warped keyframe features, NHWC [Hp,Wp,C] each (frames of one GOP share theirs);
    imgs: [B,3,H,W]; mv_qs: int16 [B,H,W,2].  Returns (logits [B,n_cls,H',W'], p C8 [B,C/8,Hp,Wp,8]).
    """
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    sub = ops.config.lr_subbatch
    if 0 < sub < B:                       # optional: bound the working set (Winograd V / M tensors) per pass
        outs = [alter_res_batch_fast(lr_net, ref_ps[i:i + sub], imgs[i:i + sub], mv_qs[i:i + sub], scale) for i in range(0, B, sub)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]     # a3 + phase 1, batched
    return lr_net.phase2_warp(feat, list(ref_ps), mv_qs)               # a2 + a1 (each frame has its own MV map) + CReFF + head


def alter_res_phase1(lr_net, imgs, scale=0.5):
    """First half of ``alter_res_batch_fast``: frame downscale + ingest + LR backbone (evaluation.py:186-191).  Independent of the
    keyframe feature -- the multi-GPU runner overlaps it with the exchange of ``ref_p`` (arseg_amd/gop.py)."""
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    return lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]


def alter_res_phase2(lr_net, feat, ref_ps, mv_qs):
    """Second half: MV resize + warp + CReFF + head on the phase-1 feature (evaluation.py:176-183,193) -> logits."""
    return _unwrap(lr_net).phase2_warp(feat, list(ref_ps), mv_qs)[0]


def alter_res_batch_pred(lr_net, ref_ps, imgs, mv_qs, scale=0.5, labels=None, hist=None, ignore_label=255, groups=None, n_groups=None):
    """B non-keyframes through backbone + warp + CReFF + head and the evaluator tail (evaluation.py:201-209) in one go:
    -> (pred int32 [B,H,W], hist int64 [n_cls,n_cls] | None).  For BiSeNet the head's 1/8-resolution logits go straight into
    the argmax (x8 upsample fused); the other networks' logits are resized (align_corners=True,
    the identity for PSPNet) inside the same argmax kernel.  ``groups`` (one id per frame, e.g. the keyframe distances
    ``range(1, 12)`` of a GOP; see ops.argmax_confusion_grouped) with ``n_groups``: hist is [n_groups,n_cls,n_cls], frame b counts into
    hist[groups[b]]; pred is unchanged."""
    if groups is not None and n_groups is None:
        raise ValueError("groups needs n_groups (the number of histograms)")
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")                       # BiSeNetOutput: head -> nn.Upsample(x8, align_corners=False)
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):               # label size differs from 8x the head: two resizes, not fusable
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    if groups is not None:
        return ops.argmax_confusion_grouped(lo, labels, groups, n_groups, H, W, hist, ignore_label, align_corners=not fused_up)
    return ops.argmax_confusion(lo, labels, H, W, hist, ignore_label, align_corners=not fused_up)


def alter_res_batch_render(lr_net, ref_ps, imgs, mv_qs, scale=0.5, palette=None, lut=None, labels_out=None, out=None):
    """The deployment sibling of ``alter_res_batch_pred``: the same phase 1 and phase 2, then the egress launch instead of the evaluator
    tail -> (labels uint8 [B,H,W], painted frames | None).  The labels equal ``alter_res_batch_pred``'s pred (the same route decision:
    BiSeNet's 1/8-resolution head logits with align_corners=False when the frame is exactly 8x the head, align_corners=True otherwise),
    as bytes and through ``lut`` (n_cls integers 0..255) when given.  ``palette`` (``egress.Palette`` or an [n_cls,3] colour table): also paint the classes over
    ``imgs``, which must then be 8-bit ``ingest.DecodedFrames`` (RGB8, NV12, I420); ``out`` the frames to write into (``out=imgs``: in
    place).  ``labels_out`` / ``out``: the caller's buffers; with both given nothing frame-sized is allocated.  A GOP's keyframe goes
    through ``egress.overlay(net.forward_keyframe(key)[0], key, palette)``.  ``out`` without ``palette`` is a ValueError (nothing would be
    painted into it)."""
    from . import egress
    if palette is None and out is not None:
        raise ValueError("alter_res_batch_render: out= needs a palette (without one only the labels are written)")
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    if palette is None:
        return egress.labels8(lo, H, W, lut=lut, out=labels_out, align_corners=not fused_up), None
    painted, labels = egress.overlay(lo, imgs, palette, out=out, labels_out=True if labels_out is None else labels_out, lut=lut,
                                     align_corners=not fused_up)
    return labels, painted


def alter_res_batch_confidence(lr_net, ref_ps, imgs, mv_qs, scale=0.5, kind="top1", low=128, lut=None, out=None, labels_out=True, stats=True):
    """``alter_res_batch_render``'s sibling for the online quality signal: the same phase 1 and phase 2 and the same route decision
    (BiSeNet's 1/8-resolution head logits with align_corners=False when the frame is exactly 8x the head, align_corners=True otherwise),
    then ``egress.confidence`` instead of the egress launch -> (conf8 uint8 [B,H,W], labels uint8 [B,H,W] | None, stats int64
    [B, CONF_NSTATS] | None).  The labels equal ``alter_res_batch_render``'s; ``kind``, ``low``, ``lut``, ``out``, ``labels_out`` and
    ``stats`` as ``egress.confidence`` takes them (True: allocated here, a tensor: the caller's, None: not wanted).  Feed the rows of
    ``stats`` to an ``egress.DriftMonitor``."""
    from . import egress
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    return egress.confidence(lo, H, W, kind=kind, low=low, out=out, labels_out=labels_out, lut=lut, stats=stats, align_corners=not fused_up)


def alter_res_batch_calibration(lr_net, ref_ps, imgs, mv_qs, labels, scale=0.5, cal=None, hist=None, ignore_label=255, groups=None, n_groups=1,
                                kind="top1"):
    """``alter_res_batch_pred``'s sibling for the reliability table: the same phase 1 and phase 2 and the same route decision, then
    ``ops.calibration`` of the logits against ``labels`` (int64 [B,H,W]) -> (cal int64 [n_groups, n_cls, 256, 2], hist int64
    [n_groups, n_cls, n_cls] | None), both accumulated when given.  ``hist``: True or a tensor to also run the grouped evaluator tail on
    the same logits (``ops.argmax_confusion_grouped``, whose column sums and diagonal the table's sums over the codes are), None for the
    table alone.  ``groups`` / ``n_groups`` as ``ops.calibration`` takes them.  Nothing comes to the host in between."""
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    lo = lo.contiguous()
    if hist is not None:
        _, hist = ops.argmax_confusion_grouped(lo, labels, [0] * B if groups is None else groups, n_groups, H, W, None if hist is True else hist,
                                               ignore_label, want_pred=False, align_corners=not fused_up)
    cal = ops.calibration(lo, labels, H, W, groups=groups, n_groups=n_groups, cal=cal, ignore_label=ignore_label, kind=kind,
                          align_corners=not fused_up)
    return cal, hist


def alter_res_batch_consistency(lr_net, ref_ps, imgs, mv_qs, key_labels, scale=0.5, lut=None, change_out=True, labels_out=True, stats=True):
    """``alter_res_batch_confidence``'s sibling for temporal consistency: the same phase 1 and phase 2 and the same route decision
    (BiSeNet's 1/8-resolution head logits with align_corners=False when the frame is exactly 8x the head, align_corners=True otherwise),
    then ``egress.consistency`` against ``key_labels``, the keyframe's TRAIN-ID plane (uint8 [H,W] or [1,H,W]:
    ``egress.labels8(net.forward_keyframe(key)[0], H, W)`` without a lut; [B,H,W] for a reference per frame), through ``mv_qs`` -- the
    int16 field [B,H,W,2] accumulated back to the keyframe that phase 2 warps with -> (change8 uint8 [B,H,W] | None, labels uint8
    [B,H,W] | None, stats int64 [B, TC_NSTATS] | None).  The labels equal ``alter_res_batch_render``'s; ``lut``, ``change_out``,
    ``labels_out`` and ``stats`` as ``egress.consistency`` takes them (True: allocated here, a tensor: the caller's, None: not wanted).
    Feed the rows of ``stats`` to an ``egress.ConsistencyMonitor`` or to ``egress.tc_table``."""
    from . import egress
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    return egress.consistency(lo, key_labels, mv_qs, H, W, change_out=change_out, labels_out=labels_out, lut=lut, stats=stats,
                              align_corners=not fused_up)


def alter_res_batch_consistency_linked(lr_net, ref_ps, imgs, mv_qs, key_labels, scale=0.5, lut=None, change_out=True, labels_out=True, stats=True,
                                       link=None, link_mask=_lib.LINK_INTRA | _lib.LINK_UNCOVERED):
    """``alter_res_batch_consistency`` gated by the motion chain's link bytes: ``link`` uint8 [B,H,W], the frames' planes of
    ``ingest.MotionChain(track_links=True).link()[1:]`` (the chain ``mv_qs`` came from), ``link_mask`` the flags that gate.  The same phase 1,
    phase 2 and route decision; then TWO passes over the label plane instead of one over the logits: the fused tail writes the train-id
    plane (``egress.labels8``), and ``egress.consistency_of_planes(..., link=link)`` compares it (the logits form has no linked variant).
    A pixel with ``link & link_mask`` is unlinked: change8 128, in no counter of ``stats``, counted per frame in ``unlinked``.
    -> (change8 | None, labels uint8 [B,H,W] | None, stats | None, unlinked int64 [B]).  ``labels_out`` True or a buffer: the labels as
    ``alter_res_batch_consistency`` returns them (through ``lut`` when given, which costs one more tail launch: the comparison needs train
    ids).  ``link_mask=0`` gives ``alter_res_batch_consistency``'s planes and statistics."""
    from . import egress
    if link is None:
        raise _lib.ArsegError("alter_res_batch_consistency_linked: link is required (alter_res_batch_consistency is the form without)")
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    keep = labels_out if torch.is_tensor(labels_out) and lut is None else None
    train_ids = egress.labels8(lo, H, W, out=keep, align_corners=not fused_up)
    change, stats, unlinked = egress.consistency_of_planes(train_ids, key_labels, mv_qs, lo.shape[1], change_out=change_out, stats=stats, link=link,
                                                           link_mask=link_mask, unlinked=True)
    if labels_out is None:
        labels = None
    elif lut is None:
        labels = train_ids
    else:
        labels = egress.labels8(lo, H, W, lut=lut, out=labels_out if torch.is_tensor(labels_out) else None, align_corners=not fused_up)
    return change, labels, stats, unlinked


def alter_res_batch_stabilised(lr_net, ref_ps, imgs, mv_qs, key_labels, bonus, scale=0.5, link=None, link_mask=_lib.LINK_INTRA | _lib.LINK_UNCOVERED,
                               key_conf=None, ref_low=0, lut=None, hold_out=None, stats=True):
    """``alter_res_batch_consistency``'s sibling that acts on what it measures: the same phase 1 and phase 2 and the same route decision,
    then ``egress.stabilise`` against ``key_labels`` (the keyframe's TRAIN-ID plane) through ``mv_qs`` with the hold threshold ``bonus``
    (a float or fp32 [B] on the device; ``egress.hold_bonus``) -> (labels uint8 [B,H,W], hold8 uint8 [B,H,W] | None, stats int64
    [B, ST_NSTATS] | None).  ``link`` / ``link_mask``: the chain's link planes of the frames and the flags that gate (None: no gate);
    ``key_conf`` / ``ref_low``: the keyframe's ``egress.confidence`` plane and the code below which it offers no prior (None: no gate);
    ``lut``, ``hold_out`` and ``stats`` as ``egress.stabilise`` takes them.  With ``bonus <= 0`` the labels equal ``alter_res_batch_render``'s."""
    from . import egress
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    return egress.stabilise(lo, key_labels, mv_qs, H, W, bonus, link=link, link_mask=link_mask, ref_conf=key_conf, ref_low=ref_low, labels_out=True,
                            hold_out=hold_out, stats=stats, lut=lut, align_corners=not fused_up)


def alter_res_batch_rle(lr_net, ref_ps, imgs, mv_qs, capacity, scale=0.5, lut=None, labels_out=True):
    """``alter_res_batch_render``'s sibling for run-length coded masks: the same phase 1 and phase 2 and the same route decision
    (BiSeNet's 1/8-resolution head logits with align_corners=False when the frame is exactly 8x the head, align_corners=True otherwise),
    then ``egress.rle`` -> (``egress.RleFrames`` with room for ``capacity`` runs per frame, labels uint8 [B,H,W]).  The labels equal
    ``alter_res_batch_render``'s (through ``lut`` when given) and are the plane the runs were taken from; ``labels_out``: True -- allocated
    here -- or the caller's buffer.  ``RleFrames.to_host()`` brings the runs over the host link, ``RleFrames.decode()`` gives the planes
    back on a GPU."""
    from . import egress
    lr_net = _unwrap(lr_net)
    B, _, H, W = imgs.shape
    h, w = _downscale_hw(H, W, scale)
    feat = lr_net.phase1_nhwc4(ops.ingest_input(imgs, h, w, lr_net.storage_dtype), aux=ops.config.aux_outputs)[-1]
    fused_up = hasattr(lr_net, "out_upsample")
    if fused_up:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs, upsample=False)
        if (8 * lo.shape[-2], 8 * lo.shape[-1]) != (H, W):
            lo, fused_up = ops.resize_nchw(lo, 8 * lo.shape[-2], 8 * lo.shape[-1], _lib.BILINEAR, False), False
    else:
        lo, _ = lr_net.phase2_warp(feat, list(ref_ps), mv_qs)
    if labels_out is True or labels_out is None:
        labels_out = torch.empty((B, H, W), dtype=torch.uint8, device=lo.device)
    frames = egress.rle(lo, H, W, capacity, lut=lut, labels_out=labels_out, align_corners=not fused_up)
    return frames, labels_out


def alter_res_batch_regions(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, scale=0.5, lut=None, labels_out=True, connectivity=8):
    """``alter_res_batch_rle``'s sibling for the objects of each frame: the same phases, route decision and run code (room for ``capacity``
    runs per frame), then ``egress.regions`` on it -> (``egress.RegionFrames`` with room for ``region_capacity`` regions per frame, whose
    ``.frames`` is the ``RleFrames``; labels uint8 [B,H,W]).  Nothing comes to the host in between; ``RegionFrames.to_host()`` brings the
    records (value, area, bounding box, centroid) over."""
    from . import egress
    frames, labels = alter_res_batch_rle(lr_net, ref_ps, imgs, mv_qs, capacity, scale=scale, lut=lut, labels_out=labels_out)
    return egress.regions(frames, region_capacity, connectivity=connectivity), labels


def alter_res_batch_absorb(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, min_area, scale=0.5, lut=None, labels_out=True,
                           connectivity=8, protect=None, pair_capacity=None):
    """``alter_res_batch_regions``'s sibling for masks without specks: the same phases, run code and regions, then ``egress.absorb`` (every
    region below ``min_area`` pixels whose value is not in ``protect`` goes into the neighbour it shares the longest border with) and
    ``egress.regions`` on the new code -> (``egress.RegionFrames`` of the cleaned masks, whose ``.frames`` is the ``egress.AbsorbedFrames``
    and its ``.source`` the regions before the pass; labels uint8 [B,H,W]: the plane before the pass).  Nothing comes to the host in
    between."""
    from . import egress
    found, labels = alter_res_batch_regions(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, scale=scale, lut=lut, labels_out=labels_out,
                                            connectivity=connectivity)
    cleaned = egress.absorb(found, min_area, protect=protect, pair_capacity=pair_capacity)
    return egress.regions(cleaned, region_capacity, connectivity=connectivity), labels


def alter_res_batch_contours(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, scale=0.5, lut=None, labels_out=True, connectivity=8,
                             min_area=None, protect=None, pair_capacity=None, loop_capacity=None, vertex_capacity=None):
    """``alter_res_batch_regions``'s sibling for vector outlines: the same phases, run code and regions, then ``egress.contours`` ->
    (``egress.ContourFrames``, whose ``.source`` is the ``egress.RegionFrames`` the outlines belong to; labels uint8 [B,H,W]).  With
    ``min_area`` the specks are absorbed first (``alter_res_batch_absorb``: ``egress.absorb`` + ``egress.regions``) and the outlines are
    those of the cleaned masks; labels stay the plane before the pass.  Nothing comes to the host in between;
    ``ContourFrames.to_host()`` brings the polygons over."""
    from . import egress
    if min_area is None:
        found, labels = alter_res_batch_regions(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, scale=scale, lut=lut,
                                                labels_out=labels_out, connectivity=connectivity)
    else:
        found, labels = alter_res_batch_absorb(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, min_area, scale=scale, lut=lut,
                                               labels_out=labels_out, connectivity=connectivity, protect=protect, pair_capacity=pair_capacity)
    return egress.contours(found, loop_capacity=loop_capacity, vertex_capacity=vertex_capacity), labels


def alter_res_batch_polygons(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, tolerance, scale=0.5, lut=None, labels_out=True,
                             connectivity=8, min_area=None, protect=None, pair_capacity=None, loop_capacity=None, vertex_capacity=None,
                             shared_borders=False):
    """``alter_res_batch_contours`` + ``egress.simplify``: the outlines within ``tolerance`` pixels (a non-negative multiple of 0.25) ->
    (``egress.SimplifiedContours``, whose ``.contours`` are the exact outlines and ``.source`` the regions; labels uint8 [B,H,W]).  With
    ``min_area`` the specks are absorbed first.  With ``shared_borders`` the last step is ``egress.simplify_shared`` (->
    ``egress.SharedContours``): a border between two regions is simplified once, so neighbouring polygons leave no gap between them.
    Nothing comes to the host in between; ``to_host()`` brings the polygons over."""
    from . import egress
    outlines, labels = alter_res_batch_contours(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, scale=scale, lut=lut, labels_out=labels_out,
                                                connectivity=connectivity, min_area=min_area, protect=protect, pair_capacity=pair_capacity,
                                                loop_capacity=loop_capacity, vertex_capacity=vertex_capacity)
    return (egress.simplify_shared if shared_borders else egress.simplify)(outlines, tolerance), labels


def alter_res_batch_polygon_fidelity(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, tolerance, scale=0.5, lut=None, connectivity=8,
                                     min_area=None, protect=None, pair_capacity=None, loop_capacity=None, vertex_capacity=None,
                                     shared_borders=False, background=255):
    """``alter_res_batch_polygons`` + ``egress.fill``: the polygons filled back into masks and compared with the masks they were traced
    from -> (the polygons, ``egress.FilledFrames``, labels uint8 [B,H,W]).  ``FilledFrames.fidelity()`` tells per frame what
    ``tolerance`` did: uncovered and doubly covered pixels (both 0 with ``shared_borders``), changed pixels and the IoU per value.  The
    reference is ``labels``, the mask before any absorption: with ``min_area`` the absorbed specks count as changed.  Nothing comes to the
    host in between."""
    from . import egress
    polygons, labels = alter_res_batch_polygons(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, tolerance, scale=scale, lut=lut,
                                                labels_out=True, connectivity=connectivity, min_area=min_area, protect=protect,
                                                pair_capacity=pair_capacity, loop_capacity=loop_capacity, vertex_capacity=vertex_capacity,
                                                shared_borders=shared_borders)
    return polygons, egress.fill(polygons, background=background, ref=labels), labels


def alter_res_batch_links(lr_net, ref_ps, imgs, mv_qs, key_regions, capacity, region_capacity, scale=0.5, lut=None, labels_out=True,
                          connectivity=8, pair_capacity=None):
    """``alter_res_batch_regions``'s sibling for object association: the same phases, run code and regions, then ``egress.links`` of every
    frame's regions to ``key_regions`` -- the ``egress.RegionFrames`` of the keyframe's mask (one frame, made with the same ``lut`` and
    ``connectivity``) -- through ``mv_qs``, the int16 field [B,H,W,2] accumulated back to the keyframe that phase 2 warps with ->
    (``egress.LinkFrames``, ``egress.RegionFrames``, labels uint8 [B,H,W]).  Nothing comes to the host in between;
    ``LinkFrames.to_host()`` brings the links over, ``egress.TrackIds`` turns them into ids that last over the stream."""
    from . import egress
    found, labels = alter_res_batch_regions(lr_net, ref_ps, imgs, mv_qs, capacity, region_capacity, scale=scale, lut=lut, labels_out=labels_out,
                                            connectivity=connectivity)
    return egress.links(found, key_regions, mv_qs, pair_capacity=pair_capacity), found, labels
