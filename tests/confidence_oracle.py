"""float64 oracle of arseg_segment_confidence_fwd (include/arseg_hip.h), written from its contract with torch on the CPU: the fp32 logits
-> F.interpolate(bilinear, align_corners) in float64 -> softmax -> top-1 / top-2 -> floor(255 c + 0.5), NaN -> 0.  Also the comparison rule
the GPU tests hold the kernel to, and the seeded inputs both test files use (tests/test_confidence.py shows on the CPU that every one of
them leaves the reference inside the rule's caps).

Error budget behind the rule, for |logit| <= 8: the kernel's fp32 blend is a convex combination, absolute error <= ~8e-6 (the run route's
regrouped form included), so the relative error of p1 is <= ~2.3e-5 = 0.006 codes, and <= 0.012 codes for the margin.  The rule leaves
pixels out whose exact 255 c lies within 0.025 (twice that) of a rounding boundary j + 0.5."""
import numpy as np
import torch
import torch.nn.functional as F

BOUNDARY = 0.025          # codes: excluded distance to a rounding boundary j + 0.5
MAX_BOUNDARY_SHARE = 0.10
MIN_DISTINCT = 64
KINDS = ("top1", "margin")

# (name, seed, N, n_cls, h, w, H, W, align_corners): the smallest shapes at which each route can go wrong -- same size; per-pixel bilinear;
# the run route at x2 / x4 / x8 on an odd-sized map narrower than a wave (first and last half-runs in play); 32 classes on two routes
CASES = [
    ("same", 101, 2, 12, 24, 40, 24, 40, True),
    ("bilinear", 102, 2, 19, 17, 20, 136, 160, True),
    ("x2", 103, 3, 19, 9, 11, 18, 22, False),
    ("x4", 104, 3, 19, 9, 11, 36, 44, False),
    ("x8", 105, 3, 19, 9, 11, 72, 88, False),
    ("same-32", 106, 2, 32, 24, 40, 24, 40, True),
    ("x8-32", 107, 2, 32, 9, 11, 72, 88, False),
]
CASE_IDS = [c[0] for c in CASES]


def make_logits(seed, N, n_cls, h, w, scale=3.0):
    """Seeded fp32 logits with |x| <= 8: clipped normal draws, spread enough that the codes cover most of 0..255."""
    g = np.random.Generator(np.random.PCG64(seed))
    return np.clip(g.standard_normal((N, n_cls, h, w)) * scale, -8.0, 8.0).astype(np.float32)


def case_logits(case):
    _, seed, N, n_cls, h, w = case[:6]
    return make_logits(seed, N, n_cls, h, w)


def exact(logits, H, W, align_corners, kind):
    """fp32 logits [N,n_cls,h,w] (numpy) -> x = 255 c in float64 [N,H,W]; NaN where c is NaN."""
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32)).double()
    if tuple(x.shape[-2:]) != (H, W):
        x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align_corners))
    with np.errstate(all="ignore"):
        p = torch.softmax(x, dim=1).numpy()
    top = np.sort(p, axis=1)[:, ::-1]          # NaN sorts last, then comes first: a pixel with a NaN probability has a NaN top-1
    p1 = top[:, 0]
    p2 = top[:, 1] if p.shape[1] > 1 else np.zeros_like(p1)
    nan = np.isnan(p).any(axis=1)
    if kind == "top1":
        c = p1
    elif kind == "margin":
        c = p1 - p2
    else:
        raise ValueError(kind)
    return np.where(nan, np.nan, 255.0 * c)


def codes(x):
    """x = 255 c -> q uint8: floor(x + 0.5), NaN -> 0."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0.0, np.floor(x + 0.5)).astype(np.uint8)


def boundary_mask(x):
    """Pixels whose exact 255 c lies within BOUNDARY of a rounding boundary j + 0.5 (NaN pixels are never boundary pixels)."""
    with np.errstate(invalid="ignore"):
        d = np.abs(x - (np.floor(x) + 0.5))
        return np.where(np.isnan(x), False, d <= BOUNDARY)


def reference_figures(x):
    """(share of boundary pixels, distinct codes) of a case's reference."""
    return float(boundary_mask(x).mean()), int(len(np.unique(codes(x))))


def check(q, x, what="", distinct=True):
    """The comparison rule: |q - q_ref| <= 1 on every pixel; q == q_ref on every pixel outside the boundary mask; the mask holds at most
    MAX_BOUNDARY_SHARE of the pixels; the reference takes at least MIN_DISTINCT distinct codes (``distinct=False`` only where the contract
    fixes the codes, as for n_cls == 1).  Prints the figures, then asserts."""
    q = np.asarray(q)
    q_ref = codes(x)
    assert q.shape == q_ref.shape and q.dtype == np.uint8
    diff = np.abs(q.astype(np.int64) - q_ref.astype(np.int64))
    mask = boundary_mask(x)
    share, n_distinct = float(mask.mean()), int(len(np.unique(q_ref)))
    off_outside, off_inside = int((diff[~mask] != 0).sum()), int((diff[mask] != 0).sum())
    print(f"\n{what}: max |q - q_ref| {int(diff.max())}, {off_outside} differing outside the boundary mask, {off_inside} inside; "
          f"boundary share {100 * share:.2f} %, {n_distinct} distinct reference codes, {int(np.isnan(x).sum())} NaN pixels")
    assert int(diff.max()) <= 1
    assert off_outside == 0
    assert share <= MAX_BOUNDARY_SHARE
    if distinct:
        assert n_distinct >= MIN_DISTINCT


def plant_specials(x):
    """Plants, in place, into logits [N >= 2, n_cls >= 8, h >= 8, w >= 8] at interior low-resolution pixels: exact ties of the top two
    classes on a row and of all classes at some pixels, a NaN logit, a +inf logit and an all -inf pixel.  Returns the (n, y, x) of the three
    pixels whose confidence is NaN by the contract."""
    x[:, 3, 4, :] = 8.0
    x[:, 6, 4, :] = 8.0                                       # classes 3 and 6 tie for the maximum on a whole row
    x[:, :, 6, 2::3] = 0.5                                     # all classes tie
    x[0, 5, 2, 2] = np.nan
    x[1, 2, 2, 6] = np.inf
    x[1, :, 6, 6] = -np.inf
    return [(0, 2, 2), (1, 2, 6), (1, 6, 6)]
