"""The definition of the contour F-measure counts (include/arseg_hip.h, arseg_contour_f_fwd) stated directly (a plain helper module): per
contour pixel the least dx^2 + dy^2 over ALL contour pixels of its class on the other plane -- no rings, no tiles, no dilation.  Hand cases
carry both mark planes, both band planes and the counts as literals.

``marks``        byte plane -> the contour class of every pixel, -1 where it is no contour pixel
``m2_direct``    the least squared distance per contour pixel by the definition, INF where the other plane has no contour of the class
``m2_fast``      the same over the offsets of the disc of radius R (INF beyond R), vectorised over the plane, for the larger planes of
                 the GPU tests; the tests hold it to ``m2_direct``
``bands``        m2 -> band (255 where there is no contour pixel)
``counts``       int64 [n_groups, 2, n_bands + 1, n_cls] from the band planes
``contour_f``    all of it: -> (counts, label bands, prediction bands)
"""
import numpy as np

import bands_oracle as bo
import boundary_iou_oracle as bio

INF = 1 << 40
HAND_N_CLS = 4


def marks(b):
    """b: uint8 [H, W] bytes.  A pixel of byte c != 255 is a contour pixel of class c when one of its 8 neighbours inside the image holds
    a byte that is neither c nor 255."""
    H, W = b.shape
    out = np.full((H, W), -1, np.int64)
    for y in range(H):
        for x in range(W):
            c = int(b[y, x])
            if c == 255:
                continue
            near = b[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
            if ((near != c) & (near != 255)).any():
                out[y, x] = c
    return out


def marks_fast(b):
    """``marks`` for every pixel at once (held to it by the tests)."""
    H, W = b.shape
    p = np.pad(b, 1, constant_values=255)
    edge = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            v = p[dy:dy + H, dx:dx + W]
            edge |= (v != b) & (v != 255)
    return np.where((b != 255) & edge, b.astype(np.int64), -1)


def m2_direct(mine, theirs):
    """Per contour pixel of ``mine`` the least squared distance to a contour pixel of the same class of ``theirs``; INF where there is none
    (and where ``mine`` has no contour pixel)."""
    out = np.full(mine.shape, INF, np.int64)
    for y, x in np.argwhere(mine >= 0):
        ty, tx = np.nonzero(theirs == mine[y, x])
        if ty.size:
            out[y, x] = int(((ty - y) ** 2 + (tx - x) ** 2).min())
    return out


def m2_fast(mine, theirs, R):
    """``m2_direct`` where it is at most R * R, INF beyond: the least dy^2 + dx^2 over the offsets of the disc at which ``theirs`` holds the
    pixel's class."""
    H, W = mine.shape
    out = np.full((H, W), INF, np.int64)
    for dy in range(-min(R, H - 1), min(R, H - 1) + 1):
        for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
            d2 = dy * dy + dx * dx
            if d2 > R * R:
                continue
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))          # the pixels whose partner is inside
            yo, xo = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            hit = (mine[ys, xs] >= 0) & (mine[ys, xs] == theirs[yo, xo])
            out[ys, xs] = np.where(hit & (out[ys, xs] > d2), d2, out[ys, xs])
    return out


def bands(m2, mine, radii):
    """band = the first radius whose square reaches m2, len(radii) for unmatched; 255 where there is no contour pixel."""
    band = np.searchsorted(np.asarray(radii, dtype=np.int64) ** 2, m2, side="left")
    return np.where(mine >= 0, band, 255).astype(np.uint8)


_MEMO = {}          # the planes of the fast form per input: computed once, shared by the tests that need them


def planes(label, pred, radii, n_cls, ignore_label=255, fast=False):
    """[N, H, W] labels and predictions -> (label marks, prediction marks, label bands, prediction bands)."""
    lb, pb = bo.void_bytes(label, n_cls, ignore_label), bio.pred_bytes(pred, n_cls)
    key = (lb.tobytes(), pb.tobytes(), lb.shape, tuple(radii))
    if fast and key in _MEMO:
        return _MEMO[key]
    mk = marks_fast if fast else marks
    ml, mp = np.stack([mk(p) for p in lb]), np.stack([mk(p) for p in pb])
    if fast:
        dl = [m2_fast(a, b, radii[-1]) for a, b in zip(ml, mp)]
        dp = [m2_fast(b, a, radii[-1]) for a, b in zip(ml, mp)]
    else:
        dl = [m2_direct(a, b) for a, b in zip(ml, mp)]
        dp = [m2_direct(b, a) for a, b in zip(ml, mp)]
    out = (ml, mp, np.stack([bands(d, m, radii) for d, m in zip(dl, ml)]), np.stack([bands(d, m, radii) for d, m in zip(dp, mp)]))
    if fast:
        _MEMO[key] = out
    return out


def counts(label, pred, ml, mp, bl, bp, groups, n_groups, n_bands, n_cls, ignore_label=255):
    """A contour pixel at which both planes' bytes are classes, in a frame whose group is in [0, n_groups), counts at
    [group, 0, band, class] on the label plane and at [group, 1, band, class] on the prediction plane."""
    out = np.zeros((n_groups, 2, n_bands + 1, n_cls), np.int64)
    lb, pb = bo.void_bytes(label, n_cls, ignore_label), bio.pred_bytes(pred, n_cls)
    for n, g in enumerate(groups):
        if not 0 <= g < n_groups:
            continue
        keep = (lb[n] != 255) & (pb[n] != 255)
        for row, mark, band in ((0, ml[n], bl[n]), (1, mp[n], bp[n])):
            sel = keep & (mark >= 0)
            codes = band[sel].astype(np.int64) * n_cls + mark[sel]
            out[g, row] += np.bincount(codes, minlength=(n_bands + 1) * n_cls).reshape(n_bands + 1, n_cls)
    return out


def contour_f(label, pred, radii, n_cls, ignore_label=255, groups=None, n_groups=1, fast=False):
    """-> (counts, label bands, prediction bands) of frames [N, H, W]."""
    label, pred = np.asarray(label), np.asarray(pred)
    ml, mp, bl, bp = planes(label, pred, radii, n_cls, ignore_label, fast)
    ids = [0] * label.shape[0] if groups is None else [int(g) for g in groups]
    return counts(label, pred, ml, mp, bl, bp, ids, n_groups, len(radii), n_cls, ignore_label), bl, bp


def sparse(entries, n_bands):
    """The counts of a hand case from their non-zero entries {(row, band, class): count}: int64 [2, n_bands + 1, HAND_N_CLS]."""
    out = np.zeros((2, n_bands + 1, HAND_N_CLS), np.int64)
    for at, v in entries.items():
        out[at] = v
    return out


def lone(H, W, background, *pixels):
    """A plane of one class with single pixels (y, x, class) of others."""
    p = [[background] * W for _ in range(H)]
    for y, x, c in pixels:
        p[y][x] = c
    return p


V = 255
_ = -1              # in a mark plane: no contour pixel
X = 255             # in a band plane: no contour pixel
_SPLIT, _SPLIT_SHIFTED = [[0, 0, 1, 1, 1]] * 5, [[0, 0, 0, 1, 1]] * 5
_DIAGONAL = [[1 if x > y else 0 for x in range(5)] for y in range(5)]
_DIAGONAL_MARKS = [[0, 1, 1, _, _], [0, 0, 1, 1, _], [_, 0, 0, 1, 1], [_, _, 0, 0, 1], [_, _, _, 0, 0]]
# Hand-made planes of 4 classes, ignore_label 255.  (name, labels, predictions, radii, the labels' marks, the predictions' marks, the labels'
# bands, the predictions' bands, the non-zero counts {(row, band, class): count}); the band len(radii) is "unmatched".
HAND = [
    # no other class anywhere: no contour, and the image border is none
    ("constant", [[2] * 5] * 5, [[2] * 5] * 5, (1, 2, 3), [[_] * 5] * 5, [[_] * 5] * 5, [[X] * 5] * 5, [[X] * 5] * 5, {}),
    # the inner contours either side of the split, each on top of the other plane's: everything at distance 0
    ("split-prediction-equals-label", _SPLIT, _SPLIT, (0, 1), [[_, 0, 1, _, _]] * 5, [[_, 0, 1, _, _]] * 5, [[X, 0, 0, X, X]] * 5, [[X, 0, 0, X, X]] * 5,
     {(0, 0, 0): 5, (0, 0, 1): 5, (1, 0, 0): 5, (1, 0, 1): 5}),
    # the split one column further right in the prediction: every contour pixel finds its class one pixel away
    ("split-prediction-shifted-one-pixel", _SPLIT, _SPLIT_SHIFTED, (0, 1), [[_, 0, 1, _, _]] * 5, [[_, _, 0, 1, _]] * 5, [[X, 1, 1, X, X]] * 5,
     [[X, X, 1, 1, X]] * 5, {(0, 1, 0): 5, (0, 1, 1): 5, (1, 1, 0): 5, (1, 1, 1): 5}),
    # a diagonal step: the pixels one below the diagonal (class 0) and two right of it (class 1) touch the other class by a corner only
    ("diagonal-step", _DIAGONAL, _DIAGONAL, (1,), _DIAGONAL_MARKS, _DIAGONAL_MARKS, [[X if m == _ else 0 for m in row] for row in _DIAGONAL_MARKS],
     [[X if m == _ else 0 for m in row] for row in _DIAGONAL_MARKS], {(0, 0, 0): 9, (0, 0, 1): 7, (1, 0, 0): 9, (1, 0, 1): 7}),
    # a pixel of class 2 on each plane, (3, 4) apart: 25 is beyond 4 and within 5.  The rings of class 0 around them match by the same rule:
    # (0, 0) finds (3, 4) at 25, (2, 2) finds it at 5
    ("lone-pixels-offset-3-4", lone(6, 7, 0, (1, 1, 2)), lone(6, 7, 0, (4, 5, 2)), (4, 5),
     [[0, 0, 0, _, _, _, _], [0, 2, 0, _, _, _, _], [0, 0, 0, _, _, _, _], [_] * 7, [_] * 7, [_] * 7],
     [[_] * 7, [_] * 7, [_] * 7, [_, _, _, _, 0, 0, 0], [_, _, _, _, 0, 2, 0], [_, _, _, _, 0, 0, 0]],
     [[1, 1, 0, X, X, X, X], [1, 1, 0, X, X, X, X], [1, 0, 0, X, X, X, X], [X] * 7, [X] * 7, [X] * 7],
     [[X] * 7, [X] * 7, [X] * 7, [X, X, X, X, 0, 0, 1], [X, X, X, X, 0, 1, 1], [X, X, X, X, 0, 1, 1]],
     {(0, 0, 0): 4, (0, 1, 0): 4, (0, 1, 2): 1, (1, 0, 0): 4, (1, 1, 0): 4, (1, 1, 2): 1}),
    # (4, 4) apart: inside the square of 5, outside the disc (32 > 25) -- unmatched.  Where the disc differs from the square
    ("lone-pixels-offset-4-4", lone(7, 7, 0, (1, 1, 2)), lone(7, 7, 0, (5, 5, 2)), (5,),
     [[0, 0, 0, _, _, _, _], [0, 2, 0, _, _, _, _], [0, 0, 0, _, _, _, _], [_] * 7, [_] * 7, [_] * 7, [_] * 7],
     [[_] * 7, [_] * 7, [_] * 7, [_] * 7, [_, _, _, _, 0, 0, 0], [_, _, _, _, 0, 2, 0], [_, _, _, _, 0, 0, 0]],
     [[1, 0, 0, X, X, X, X], [0, 1, 0, X, X, X, X], [0, 0, 0, X, X, X, X], [X] * 7, [X] * 7, [X] * 7, [X] * 7],
     [[X] * 7, [X] * 7, [X] * 7, [X] * 7, [X, X, X, X, 0, 0, 0], [X, X, X, X, 0, 1, 0], [X, X, X, X, 0, 0, 1]],
     {(0, 0, 0): 7, (0, 1, 0): 1, (0, 1, 2): 1, (1, 0, 0): 7, (1, 1, 0): 1, (1, 1, 2): 1}),
    # targets at (5, 5), Chebyshev ring 5, squared distance 50, and at (0, 6), ring 6, squared distance 36: the label's pixel is within 6.
    # From the prediction's side (6, 6) finds the label's pixel at 50 (within 8), (1, 7) at 36
    ("nearer-target-in-a-later-ring", lone(8, 9, 0, (1, 1, 2)), lone(8, 9, 0, (6, 6, 2), (1, 7, 2)), (6, 7, 8),
     [[0, 0, 0, _, _, _, _, _, _], [0, 2, 0, _, _, _, _, _, _], [0, 0, 0, _, _, _, _, _, _], [_] * 9, [_] * 9, [_] * 9, [_] * 9, [_] * 9],
     [[_, _, _, _, _, _, 0, 0, 0], [_, _, _, _, _, _, 0, 2, 0], [_, _, _, _, _, _, 0, 0, 0], [_] * 9, [_] * 9, [_, _, _, _, _, 0, 0, 0, _],
      [_, _, _, _, _, 0, 2, 0, _], [_, _, _, _, _, 0, 0, 0, _]],
     [[0, 0, 0, X, X, X, X, X, X], [0, 0, 0, X, X, X, X, X, X], [0, 0, 0, X, X, X, X, X, X], [X] * 9, [X] * 9, [X] * 9, [X] * 9, [X] * 9],
     [[X, X, X, X, X, X, 0, 0, 0], [X, X, X, X, X, X, 0, 0, 0], [X, X, X, X, X, X, 0, 0, 0], [X] * 9, [X] * 9, [X, X, X, X, X, 0, 0, 0, X],
      [X, X, X, X, X, 0, 2, 1, X], [X, X, X, X, X, 0, 1, 2, X]],
     {(0, 0, 0): 8, (0, 0, 2): 1, (1, 0, 0): 13, (1, 0, 2): 1, (1, 1, 0): 2, (1, 2, 0): 1, (1, 2, 2): 1}),
    # a void block on the labels' split: the class pixels beside it (column 1, and column 2 in rows 1 and 2 is void itself) are no contour;
    # the prediction's contour runs over it: (1, 2) and (2, 2) get their band in the plane and count nowhere, and (1, 3) of the labels
    # still finds (1, 2) one pixel away
    ("void-block", [[1, 1, 1, 0, 0, 0], [1, V, V, 0, 0, 0], [1, V, V, 0, 0, 0], [1, 1, 1, 0, 0, 0]], [[1, 1, 0, 0, 0, 0]] * 4, (0, 1, 2),
     [[_, _, 1, 0, _, _], [_, _, _, 0, _, _], [_, _, _, 0, _, _], [_, _, 1, 0, _, _]],
     [[_, 1, 0, _, _, _], [_, 1, 0, _, _, _], [_, 1, 0, _, _, _], [_, 1, 0, _, _, _]],
     [[X, X, 1, 1, X, X], [X, X, X, 1, X, X], [X, X, X, 1, X, X], [X, X, 1, 1, X, X]],
     [[X, 1, 1, X, X, X], [X, 2, 1, X, X, X], [X, 2, 1, X, X, X], [X, 1, 1, X, X, X]],
     {(0, 1, 0): 4, (0, 1, 1): 2, (1, 1, 0): 2, (1, 1, 1): 2}),
    # predictions outside the classes are the byte 255: no contour beside them in row 2, and the labels' contour there does not count
    ("predictions-outside-the-classes", _SPLIT, [[0, 0, 1, 4, 1], [0, 0, 1, 1, 1], [0, -1, 99, 1, 1], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1]], (0, 1),
     [[_, 0, 1, _, _]] * 5, [[_, 0, 1, _, _], [_, 0, 1, _, _], [_] * 5, [_, 0, 1, _, _], [_, 0, 1, _, _]],
     [[X, 0, 0, X, X], [X, 0, 0, X, X], [X, 1, 1, X, X], [X, 0, 0, X, X], [X, 0, 0, X, X]],
     [[X, 0, 0, X, X], [X, 0, 0, X, X], [X] * 5, [X, 0, 0, X, X], [X, 0, 0, X, X]],
     {(0, 0, 0): 4, (0, 0, 1): 4, (1, 0, 0): 4, (1, 0, 1): 4}),
    # class 3 is predicted only: its four contour pixels are unmatched (precision counts in the last band), its recall row is zero
    ("class-on-one-plane-only", [[0, 0, 0, 1, 1, 1]] * 5,
     [[0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 3, 3], [0, 0, 0, 1, 3, 3], [0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1]], (1, 2),
     [[_, _, 0, 1, _, _]] * 5,
     [[_, _, 0, 1, 1, 1], [_, _, 0, 1, 3, 3], [_, _, 0, 1, 3, 3], [_, _, 0, 1, 1, 1], [_, _, 0, 1, _, _]],
     [[X, X, 0, 0, X, X]] * 5,
     [[X, X, 0, 0, 0, 1], [X, X, 0, 0, 2, 2], [X, X, 0, 0, 2, 2], [X, X, 0, 0, 0, 1], [X, X, 0, 0, X, X]],
     {(0, 0, 0): 5, (0, 0, 1): 5, (1, 0, 0): 5, (1, 0, 1): 7, (1, 1, 1): 2, (1, 2, 3): 4}),
    ("one-pixel", [[3]], [[0]], (0,), [[_]], [[_]], [[X]], [[X]], {}),
    ("one-row", [[0, 0, 0, 1, 1, 1, 1, 1]], [[0, 0, 0, 0, 0, 1, 1, 1]], (1, 2), [[_, _, 0, 1, _, _, _, _]], [[_, _, _, _, 0, 1, _, _]],
     [[X, X, 1, 1, X, X, X, X]], [[X, X, X, X, 1, 1, X, X]], {(0, 1, 0): 1, (0, 1, 1): 1, (1, 1, 0): 1, (1, 1, 1): 1}),
    ("one-column", [[0], [0], [0], [1], [1], [1], [1], [1]], [[0], [0], [0], [0], [0], [1], [1], [1]], (1, 2),
     [[_], [_], [0], [1], [_], [_], [_], [_]], [[_], [_], [_], [_], [0], [1], [_], [_]],
     [[X], [X], [1], [1], [X], [X], [X], [X]], [[X], [X], [X], [X], [1], [1], [X], [X]], {(0, 1, 0): 1, (0, 1, 1): 1, (1, 1, 0): 1, (1, 1, 1): 1}),
]
HAND_IDS = [h[0] for h in HAND]
