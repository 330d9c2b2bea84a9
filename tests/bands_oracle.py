"""The definition of the boundary bands (include/arseg_hip.h, arseg_label_bands_fwd) restated without the separable form the kernels use
(a plain helper module): per pixel the clipped window grows until it holds a different byte.  Hand cases carry their distances as literals.

``void_bytes``   label -> byte (255: void)
``distance``     D per pixel, R + 1 where there is no other byte within R: the window grown pixel by pixel (``distance_pixel``)
``distance_fast`` the same from the offsets of the window, vectorised over the plane, for the larger planes of the GPU tests; the tests
                 hold it to ``distance``
``bands``        D -> band
``banded_hist``  the confusion counts per group and band
"""
import numpy as np

R_HAND = 3          # the hand cases' largest radius: a distance beyond it is written as R_HAND + 1 = 4


def void_bytes(label, n_cls, ignore_label=255):
    lab = np.asarray(label).astype(np.int64)
    return np.where((lab >= 0) & (lab < n_cls) & (lab != ignore_label), lab, 255).astype(np.uint8)


def distance_pixel(b, y, x, R):
    """The smallest r in 1 .. R whose (2r+1) x (2r+1) window at (y, x), clipped to the plane ``b``, holds a byte other than b[y, x]; R + 1
    if none does."""
    H, W = b.shape
    for r in range(1, R + 1):
        if (b[max(y - r, 0):min(y + r, H - 1) + 1, max(x - r, 0):min(x + r, W - 1) + 1] != b[y, x]).any():
            return r
    return R + 1


def distance(b, R):
    return np.array([[distance_pixel(b, y, x, R) for x in range(b.shape[1])] for y in range(b.shape[0])], dtype=np.int64).reshape(b.shape)


def distance_fast(b, R):
    """``distance`` for every pixel at once: the least max(|dy|, |dx|) over the offsets within R at which the plane holds another byte."""
    H, W = b.shape
    d = np.full((H, W), R + 1, np.int64)
    for dy in range(-min(R, H - 1), min(R, H - 1) + 1):
        for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
            r = max(abs(dy), abs(dx))
            if r == 0:
                continue
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))          # the pixels whose partner is inside
            yo, xo = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            differs = b[ys, xs] != b[yo, xo]
            d[ys, xs] = np.where(differs & (d[ys, xs] > r), r, d[ys, xs])
    return d


def bands(d, radii):
    """band = the first radius that reaches d; len(radii): interior."""
    return np.searchsorted(np.asarray(radii), d, side="left").astype(np.uint8)


def label_bands(label, radii, n_cls, ignore_label=255, fast=False):
    """[..., H, W] labels -> the band planes, frame by frame."""
    lab = np.asarray(label)
    b = void_bytes(lab, n_cls, ignore_label).reshape((-1,) + lab.shape[-2:])
    dist = distance_fast if fast else distance
    return np.stack([bands(dist(p, radii[-1]), radii) for p in b]).reshape(lab.shape)


def banded_hist(label, pred, band, groups, n_groups, n_bands, n_cls, ignore_label=255):
    """int64 [n_groups, n_bands + 1, n_cls, n_cls] of frames [N, H, W]: a non-void pixel with a prediction in [0, n_cls), in a frame whose
    group is in [0, n_groups), counts at [group, band, label, pred]."""
    hist = np.zeros((n_groups, n_bands + 1, n_cls, n_cls), np.int64)
    b = void_bytes(label, n_cls, ignore_label)
    pred = np.asarray(pred).astype(np.int64)
    for n, g in enumerate(groups):
        if not 0 <= g < n_groups:
            continue
        keep = (b[n] != 255) & (pred[n] >= 0) & (pred[n] < n_cls)
        np.add.at(hist[g], (band[n][keep].astype(np.int64), b[n][keep].astype(np.int64), pred[n][keep]), 1)
    return hist


def confusion(label, pred, n_cls, ignore_label=255):
    """The plain confusion matrix of the evaluator tail: int64 [n_cls, n_cls]."""
    b = void_bytes(label, n_cls, ignore_label)
    pred = np.asarray(pred).astype(np.int64)
    keep = (b != 255) & (pred >= 0) & (pred < n_cls)
    return np.bincount(b[keep].astype(np.int64) * n_cls + pred[keep], minlength=n_cls * n_cls).reshape(n_cls, n_cls)


V = 255
# Hand-made planes of 4 classes with the distances written out for R = 3 (4: nothing within 3).  (name, labels, ignore_label, D).  The first
# nine are 5 x 5 with ignore_label 255, so that they can be the frames of one call.
HAND = [
    ("constant", [[2] * 5] * 5, 255, [[4] * 5] * 5),
    ("checkerboard", [[(x + y) & 1 for x in range(5)] for y in range(5)], 255, [[1] * 5] * 5),
    ("odd-pixel-in-a-corner", [[1, 0, 0, 0, 0]] + [[0] * 5] * 4, 255,
     [[1, 1, 2, 3, 4], [1, 1, 2, 3, 4], [2, 2, 2, 3, 4], [3, 3, 3, 3, 4], [4, 4, 4, 4, 4]]),
    ("odd-pixel-in-the-centre", [[0] * 5, [0] * 5, [0, 0, 3, 0, 0], [0] * 5, [0] * 5], 255,
     [[2, 2, 2, 2, 2], [2, 1, 1, 1, 2], [2, 1, 1, 1, 2], [2, 1, 1, 1, 2], [2, 2, 2, 2, 2]]),
    ("vertical-stripe", [[0, 0, 1, 0, 0]] * 5, 255, [[2, 1, 1, 1, 2]] * 5),
    ("horizontal-stripe", [[0] * 5, [0] * 5, [1] * 5, [0] * 5, [0] * 5], 255, [[2] * 5, [1] * 5, [1] * 5, [1] * 5, [2] * 5]),
    ("diagonal-step", [[1 if x > y else 0 for x in range(5)] for y in range(5)], 255,
     [[1, 1, 1, 2, 2], [1, 1, 1, 1, 2], [2, 1, 1, 1, 1], [2, 2, 1, 1, 1], [3, 2, 2, 1, 1]]),
    ("void-block", [[1] * 5, [1, V, V, 1, 1], [1, V, V, 1, 1], [1] * 5, [1] * 5], 255,
     [[1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [1, 1, 1, 1, 2], [2, 2, 2, 2, 2]]),
    ("malformed-labels-are-one-value", [[-1, 255, 7, -5, 4], [99, 1 << 40, 255, 4, -(1 << 40)], [2] * 5, [2] * 5, [2] * 5], 255,
     [[2] * 5, [1] * 5, [1] * 5, [2] * 5, [3] * 5]),
    ("ignore-label-inside-the-classes", [[1, 1, 0], [5, -1, 0]], 1, [[2, 1, 1], [2, 1, 1]]),
    ("one-row", [[0, 0, 0, 1, 1, 1, 1, 1]], 255, [[3, 2, 1, 1, 2, 3, 4, 4]]),
    ("one-column", [[0], [0], [0], [1], [1], [1], [1], [1]], 255, [[3], [2], [1], [1], [2], [3], [4], [4]]),
]
HAND_IDS = [h[0] for h in HAND]
HAND_N_CLS = 4


def noise_plane(seed, H, W, n_cls, void=0.05):
    """Uniform noise labels with a share of void pixels: nearly every pixel at distance 1."""
    g = np.random.Generator(np.random.PCG64(seed))
    lab = g.integers(0, n_cls, (H, W)).astype(np.int64)
    lab[g.random((H, W)) < void] = 255
    return lab


def block_plane(seed, H, W, n_cls, cell=9):
    """Blocks of about ``cell`` pixels of one label, a void ring around some: every band is populated."""
    g = np.random.Generator(np.random.PCG64(seed))
    coarse = g.integers(0, n_cls, (H // cell + 2, W // cell + 2)).astype(np.int64)
    oy, ox = int(g.integers(0, cell)), int(g.integers(0, cell))
    lab = np.kron(coarse, np.ones((cell, cell), np.int64))[oy:oy + H, ox:ox + W].copy()
    yy, xx = np.mgrid[0:H, 0:W]
    ring = (((yy + oy) % cell == 0) | ((xx + ox) % cell == 0)) & (coarse[(yy + oy) // cell, (xx + ox) // cell] == 0)
    lab[ring] = 255
    return lab
