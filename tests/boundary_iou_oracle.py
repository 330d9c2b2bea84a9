"""The definition of the Boundary IoU counts (include/arseg_hip.h, arseg_boundary_iou_fwd) restated through the window of
tests/bands_oracle.py (a plain helper module): per pixel and byte plane the clipped window grows until it holds another byte or, with the
border, leaves the image.  Hand cases carry both distance planes and the counts as literals.

``pred_bytes``   prediction -> byte (255: outside the classes)
``edge``         min(x + 1, y + 1, W - x, H - y): the smallest r whose window leaves the image
``distance``     D per pixel of a byte plane, R + 1 where nothing is within R; the border term when asked for
``distance_minmax`` the same from iterated 3 x 3 extremes, for the large planes and radii of the GPU tests
``planes``       both band planes of frames [N, H, W]
``counts``       int64 [n_groups, 3, n_bands + 1, n_cls] from the band planes
``boundary_iou`` the two together
"""
import numpy as np

import bands_oracle as bo

R_HAND = 3          # the hand cases' largest radius: a distance beyond it is written as R_HAND + 1 = 4
RADII_HAND = (1, 2, 3)
HAND_N_CLS = 4


def pred_bytes(pred, n_cls):
    p = np.asarray(pred).astype(np.int64)
    return np.where((p >= 0) & (p < n_cls), p, 255).astype(np.uint8)


def edge(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.minimum(np.minimum(xx + 1, yy + 1), np.minimum(W - xx, H - yy)).astype(np.int64)


def distance_minmax(b, R):
    """D for the large planes and radii of the GPU tests: a 3 x 3 minimum and a 3 x 3 maximum filter with edge replication, iterated; after
    r rounds they are the extremes of the clipped (2r+1) x (2r+1) window, which holds another byte than its centre's exactly when they
    differ.  The CPU tests hold it to ``bands_oracle.distance_fast``."""
    def spread(a, pick):
        p = np.pad(a, ((1, 1), (0, 0)), mode="edge")
        a = pick(pick(p[:-2], p[1:-1]), p[2:])
        p = np.pad(a, ((0, 0), (1, 1)), mode="edge")
        return pick(pick(p[:, :-2], p[:, 1:-1]), p[:, 2:])

    lo = hi = b
    d = np.full(b.shape, R + 1, np.int64)
    for r in range(1, R + 1):
        lo, hi = spread(lo, np.minimum), spread(hi, np.maximum)
        d = np.where((d > r) & (lo != hi), r, d)
        if int(d.max()) <= r:
            break
    return d


_MEMO = {}          # the vectorised distances per (form, plane, R): computed once, shared by the tests that need them


def distance(b, R, border, fast=False):
    """``fast``: False the window grown pixel by pixel, True ``bands_oracle.distance_fast``, "minmax" ``distance_minmax``."""
    if fast:
        key = (fast, b.tobytes(), b.shape, R)
        if key not in _MEMO:
            _MEMO[key] = distance_minmax(b, R) if fast == "minmax" else bo.distance_fast(b, R)
        d = _MEMO[key]
    else:
        d = bo.distance(b, R)
    return np.minimum(d, edge(*b.shape)) if border else d


def planes(label, pred, radii, n_cls, ignore_label=255, border=True, fast=False):
    """[N, H, W] labels and predictions -> (label bands, prediction bands), uint8 [N, H, W]."""
    lb, pb = bo.void_bytes(label, n_cls, ignore_label), pred_bytes(pred, n_cls)
    bg = np.stack([bo.bands(distance(p, radii[-1], border, fast), radii) for p in lb])
    bp = np.stack([bo.bands(distance(p, radii[-1], border, fast), radii) for p in pb])
    return bg, bp


def counts(label, pred, bg, bp, groups, n_groups, n_bands, n_cls, ignore_label=255):
    """A pixel whose label byte and prediction byte are both classes, in a frame whose group is in [0, n_groups), counts at
    [group, 0, bg, label], at [group, 1, bp, pred] and, where the two agree, at [group, 2, max(bg, bp), label]."""
    out = np.zeros((n_groups, 3, n_bands + 1, n_cls), np.int64)
    lb, pb = bo.void_bytes(label, n_cls, ignore_label).astype(np.int64), pred_bytes(pred, n_cls).astype(np.int64)
    for n, g in enumerate(groups):
        if not 0 <= g < n_groups:
            continue
        keep = (lb[n] != 255) & (pb[n] != 255)
        hit = keep & (lb[n] == pb[n])
        for row, band, cls, sel in ((0, bg[n], lb[n], keep), (1, bp[n], pb[n], keep), (2, np.maximum(bg[n], bp[n]), lb[n], hit)):
            codes = band[sel].astype(np.int64) * n_cls + cls[sel]
            out[g, row] += np.bincount(codes, minlength=(n_bands + 1) * n_cls).reshape(n_bands + 1, n_cls)
    return out


def boundary_iou(label, pred, radii, n_cls, ignore_label=255, border=True, groups=None, n_groups=1, fast=False):
    """-> (counts, label bands, prediction bands) of frames [N, H, W]."""
    label, pred = np.asarray(label), np.asarray(pred)
    bg, bp = planes(label, pred, radii, n_cls, ignore_label, border, fast)
    ids = [0] * label.shape[0] if groups is None else [int(g) for g in groups]
    return counts(label, pred, bg, bp, ids, n_groups, len(radii), n_cls, ignore_label), bg, bp


def sparse(entries):
    """The counts of a hand case from their non-zero entries {(row, band, class): count}: int64 [3, len(RADII_HAND) + 1, HAND_N_CLS]."""
    out = np.zeros((3, len(RADII_HAND) + 1, HAND_N_CLS), np.int64)
    for at, v in entries.items():
        out[at] = v
    return out


V = 255
_EDGE5 = [[1, 1, 1, 1, 1], [1, 2, 2, 2, 1], [1, 2, 3, 2, 1], [1, 2, 2, 2, 1], [1, 1, 1, 1, 1]]
_STRIPE = [[0, 0, 1, 0, 0]] * 5
_STEP, _STEP_SHIFTED = [[0, 0, 1, 1, 1]] * 5, [[0, 0, 0, 1, 1]] * 5
_SPECK = [[0] * 7] * 3 + [[0, 0, 0, 1, 0, 0, 0]] + [[0] * 7] * 3
# Hand-made planes of 4 classes at the radii (1, 2, 3), ignore_label 255.  (name, labels, predictions, border, D of the labels, D of the
# predictions, the non-zero counts {(row, band, class): count}); a distance of 4 is "nothing within 3", band 3 the interior.
HAND = [
    # nothing differs and the border is no boundary: everything is interior
    ("constant-without-border", [[2] * 5] * 5, [[2] * 5] * 5, 0, [[4] * 5] * 5, [[4] * 5] * 5, {(0, 3, 2): 25, (1, 3, 2): 25, (2, 3, 2): 25}),
    # the border is the only boundary: D is the distance to the edge, 16 pixels at 1, 8 at 2, 1 at 3
    ("constant-with-border", [[2] * 5] * 5, [[2] * 5] * 5, 1, _EDGE5, _EDGE5,
     {(r, b, 2): v for r in range(3) for b, v in ((0, 16), (1, 8), (2, 1))}),
    # equal planes: equal distances, and row 2 repeats rows 0 and 1
    ("prediction-equals-label", _STRIPE, _STRIPE, 0, [[2, 1, 1, 1, 2]] * 5, [[2, 1, 1, 1, 2]] * 5,
     {(r, b, c): v for r in range(3) for (b, c), v in {(0, 0): 10, (0, 1): 5, (1, 0): 10}.items()}),
    # the boundary between columns 1 | 2 in the labels and 2 | 3 in the predictions; column 2 is labelled 1 and predicted 0
    ("prediction-shifted-one-pixel", _STEP, _STEP_SHIFTED, 0, [[2, 1, 1, 2, 3]] * 5, [[3, 2, 1, 1, 2]] * 5,
     {(0, 0, 0): 5, (0, 1, 0): 5, (0, 0, 1): 5, (0, 1, 1): 5, (0, 2, 1): 5,
      (1, 0, 0): 5, (1, 1, 0): 5, (1, 2, 0): 5, (1, 0, 1): 5, (1, 1, 1): 5,
      (2, 1, 0): 5, (2, 2, 0): 5, (2, 1, 1): 5, (2, 2, 1): 5}),
    # a speck predicted inside a large region: the ground truth's band misses it (all interior), the prediction's rings do not;
    # the intersection takes the larger band, so it is interior too
    ("speck-inside-a-region", [[0] * 7] * 7, _SPECK, 0, [[4] * 7] * 7, [[1 if d == 0 else d for d in row] for row in
                                                                       [[max(abs(y - 3), abs(x - 3)) for x in range(7)] for y in range(7)]],
     {(0, 3, 0): 49, (1, 0, 0): 8, (1, 1, 0): 16, (1, 2, 0): 24, (1, 0, 1): 1, (2, 3, 0): 48}),
    # void labels count nowhere and are a boundary on the label plane only: the prediction plane is constant
    ("void-block", [[1] * 5, [1, V, V, 1, 1], [1, V, V, 1, 1], [1] * 5, [1] * 5], [[1] * 5] * 5, 0,
     [[1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [2, 2, 2, 2, 2]], [[4] * 5] * 5,
     {(0, 0, 1): 12, (0, 1, 1): 9, (1, 3, 1): 21, (2, 3, 1): 21}),
    # predictions outside the classes are one byte, count nowhere and are a boundary on the prediction plane; with the border
    ("predictions-outside-the-classes", [[1] * 5] * 5, [[1] * 5, [1] * 5, [1, 1, -1, 4, 1], [1, 1, 99, 1, 1], [1] * 5], 1,
     _EDGE5, [[1] * 5] * 5, {(0, 0, 1): 16, (0, 1, 1): 6, (1, 0, 1): 22, (2, 0, 1): 16, (2, 1, 1): 6}),
    ("one-pixel-without-border", [[3]], [[3]], 0, [[4]], [[4]], {(0, 3, 3): 1, (1, 3, 3): 1, (2, 3, 3): 1}),
    ("one-pixel-with-border", [[3]], [[0]], 1, [[1]], [[1]], {(0, 0, 3): 1, (1, 0, 0): 1}),
    ("one-row", [[0, 0, 0, 1, 1, 1, 1, 1]], [[0, 0, 0, 0, 0, 1, 1, 1]], 0, [[3, 2, 1, 1, 2, 3, 4, 4]], [[4, 4, 3, 2, 1, 1, 2, 3]],
     {(0, 0, 0): 1, (0, 1, 0): 1, (0, 2, 0): 1, (0, 0, 1): 1, (0, 1, 1): 1, (0, 2, 1): 1, (0, 3, 1): 2,
      (1, 0, 0): 1, (1, 1, 0): 1, (1, 2, 0): 1, (1, 3, 0): 2, (1, 0, 1): 1, (1, 1, 1): 1, (1, 2, 1): 1,
      (2, 2, 0): 1, (2, 3, 0): 2, (2, 2, 1): 1, (2, 3, 1): 2}),
    # with the border a one-column plane is all boundary: every window leaves the image sideways at r = 1
    ("one-column-with-border", [[0], [0], [0], [1], [1], [1], [1], [1]], [[0], [0], [0], [1], [1], [1], [1], [1]], 1, [[1]] * 8, [[1]] * 8,
     {(r, 0, c): v for r in range(3) for c, v in ((0, 3), (1, 5))}),
]
HAND_IDS = [h[0] for h in HAND]
