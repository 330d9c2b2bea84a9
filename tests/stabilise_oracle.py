"""numpy / torch (CPU) oracle of arseg_segment_stabilise_fwd (include/arseg_hip.h), written from the contract: the class values of every
output pixel, the reference's train-id plane(s), mv_q, the hold thresholds and the two optional gates in; the outcome of every pixel, the
label plane, the hold plane and the rows of statistics out.  On the same-size route the class values are the fp32 logits and the margin is an
fp32 subtraction: everything is exact.  On the resized routes the class values are a float64 bilinear blend, and the comparison rule below
leaves the HELD / OWN decision open in a band around the threshold.  Also the seeded inputs both test files use, on top of
tests/consistency_oracle.py's generators (tests/test_stabilise.py shows on the CPU that every one of them exercises all seven outcomes).

Comparison rule (``compare``).  k* is the GPU's own (ops.argmax_confusion), as in tests/test_gpu_consistency.py.  Same-size route: every
byte and counter equals the oracle's.  Resized routes: every output label is that k* or c_ref; the HELD / OWN decision equals the oracle's
wherever |d64 - beta| > BAND, pixels inside the band may go either way, and at most BAND_CAP of a case's pixels may lie inside it.
BAND = 2e-5: the project's blend bound of ~8e-6 per class value for |logit| <= 8, taken twice (m and v_ref), plus the
rounding of the fp32 subtraction (<= 2^-24 * 16 ~ 1e-6), rounded up."""
import numpy as np
import torch
import torch.nn.functional as F

import consistency_oracle as tc

ST_NSTATS = 8 + 2 * 32
UNLINKED, OUTSIDE, VOID, WEAK, AGREE, HELD, OWN = range(7)
OUTCOMES = ("unlinked", "outside", "void", "weak", "agree", "held", "own")
INTO, FROM = 8, 40
HOLD_CODE = np.array([128, 128, 128, 128, 0, 255, 192], dtype=np.uint8)
LINK_INTRA, LINK_UNCOVERED, LINK_CLAMPED = 1, 2, 4
LINK_MASK = LINK_INTRA | LINK_UNCOVERED
REF_LOW = 128
BAND, BAND_CAP = 2e-5, 0.005

# (name, seed, N, n_cls, h, w, H, W, align_corners, shared reference planes): tests/consistency_oracle.py's shapes -- the smallest at which
# each route can go wrong: same size; per-pixel bilinear; the run route at x2 / x4 / x8 on an odd-sized map narrower than a wave (first and
# last half-runs in play); 32 classes.
CASES = list(tc.CASES)
CASE_IDS = [c[0] for c in CASES]


def label_rule(values):
    """[N,n_cls,H,W] class values -> k* int64 [N,H,W] by the one label rule: the first maximum wins, a NaN counts as the maximum (the first
    NaN wins), all -inf gives class 0."""
    v = np.asarray(values)
    N, n_cls, H, W = v.shape
    best = np.full((N, H, W), -np.inf, dtype=v.dtype)
    bi = np.zeros((N, H, W), dtype=np.int64)
    best_nan = np.zeros((N, H, W), dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in range(n_cls):
            isn = np.isnan(v[:, k])
            take = ~best_nan & ((v[:, k] > best) | isn)
            best, bi, best_nan = np.where(take, v[:, k], best), np.where(take, k, bi), best_nan | (take & isn)
    return bi


def class_values(logits, H, W, align_corners):
    """fp32 logits [N,n_cls,h,w] -> the class values the oracle decides on: the logits themselves (fp32) when h == H and w == W, their float64
    bilinear blend otherwise."""
    x = np.asarray(logits, dtype=np.float32)
    if tuple(x.shape[-2:]) == (H, W):
        return x
    return F.interpolate(torch.from_numpy(x).double(), size=(H, W), mode="bilinear", align_corners=bool(align_corners)).numpy()


def prior(ref, mv_q, n_cls, link=None, link_mask=0, ref_conf=None, ref_low=0):
    """-> pre int64 [N,H,W]: c_ref where the keyframe offers a prior, -(outcome + 1) for UNLINKED / OUTSIDE / VOID / WEAK, decided in that order."""
    ref, mv_q = np.asarray(ref), np.asarray(mv_q)
    N, H, W = mv_q.shape[:3]
    assert ref.dtype == np.uint8 and ref.shape[1:] == (H, W) and ref.shape[0] in (1, N) and mv_q.dtype == np.int16 and 0 <= ref_low <= 256
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    pre = np.empty((N, H, W), dtype=np.int64)
    for n in range(N):
        tx, ty = xs + tc.round_half_even_div4(mv_q[n, ..., 0]), ys + tc.round_half_even_div4(mv_q[n, ..., 1])
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        cx, cy = np.where(inside, tx, 0), np.where(inside, ty, 0)
        r = ref[n if ref.shape[0] > 1 else 0][cy, cx].astype(np.int64)
        p = np.where(r < n_cls, r, -(VOID + 1))
        if ref_conf is not None:
            c = np.asarray(ref_conf)
            assert c.dtype == np.uint8 and c.shape[1:] == (H, W) and c.shape[0] in (1, N)
            p = np.where((r < n_cls) & (c[n if c.shape[0] > 1 else 0][cy, cx].astype(np.int64) < ref_low), -(WEAK + 1), p)
        p = np.where(inside, p, -(OUTSIDE + 1))
        if link is not None and link_mask:
            p = np.where((np.asarray(link)[n].astype(np.int64) & link_mask) != 0, -(UNLINKED + 1), p)
        pre[n] = p
    return pre


def margin(values, kstar, pre):
    """d = v[k*] - v[c_ref] in the precision of ``values`` (fp32: the same-size route's exact subtraction; float64: the blend), NaN where
    it is NaN; 0 where there is no prior."""
    v = np.asarray(values)
    cref = np.maximum(pre, 0)
    with np.errstate(invalid="ignore"):
        d = np.take_along_axis(v, kstar[:, None], axis=1)[:, 0] - np.take_along_axis(v, cref[:, None], axis=1)[:, 0]
    return np.where(pre >= 0, d, 0).astype(v.dtype)


def stabilise(values, ref, mv_q, beta, link=None, link_mask=0, ref_conf=None, ref_low=0, kstar=None, lut=None):
    """values [N,n_cls,H,W] (``class_values``), beta fp32 [N] -> dict(outcome int64 [N,H,W], pre, kstar, d, labels uint8, hold uint8, stats
    int64 [N,ST_NSTATS], band bool [N,H,W]).  ``kstar``: the classes to decide on (default: ``label_rule(values)``).  band: differing
    pixels with a prior whose float64 margin is within BAND of beta (never on fp32 values: the same-size route is exact)."""
    v = np.asarray(values)
    N, n_cls, H, W = v.shape
    beta = np.broadcast_to(np.asarray(beta, dtype=np.float32), (N,))
    kstar = label_rule(v) if kstar is None else np.asarray(kstar).astype(np.int64)
    pre = prior(ref, mv_q, n_cls, link, link_mask, ref_conf, ref_low)
    d = margin(v, kstar, pre)
    with np.errstate(invalid="ignore"):
        held = d < beta.astype(v.dtype)[:, None, None]                  # strict; False for a NaN margin or a NaN beta
        band = (pre >= 0) & (pre != kstar) & (np.abs(d - beta.astype(v.dtype)[:, None, None]) <= BAND) if v.dtype == np.float64 else \
            np.zeros((N, H, W), dtype=bool)
    outcome = np.where(pre < 0, -(pre + 1), np.where(pre == kstar, AGREE, np.where(held, HELD, OWN)))
    labels = np.where(outcome == HELD, pre, kstar)
    return {"outcome": outcome, "pre": pre, "kstar": kstar, "d": d, "band": band, "hold": HOLD_CODE[outcome],
            "labels": (labels if lut is None else np.asarray(lut, dtype=np.uint8)[labels]).astype(np.uint8),
            "stats": stats_of(outcome, pre, kstar, n_cls)}


def stats_of(outcome, pre, kstar, n_cls):
    """The rows of statistics of an outcome plane: seven counts, a zero, into_k (HELD by c_ref) and from_k (HELD by k*)."""
    N = outcome.shape[0]
    stats = np.zeros((N, ST_NSTATS), dtype=np.int64)
    for n in range(N):
        stats[n, :7] = np.bincount(outcome[n].reshape(-1), minlength=7)
        h = outcome[n] == HELD
        stats[n, INTO:INTO + n_cls] = np.bincount(pre[n][h], minlength=n_cls)
        stats[n, FROM:FROM + n_cls] = np.bincount(kstar[n][h], minlength=n_cls)
    return stats


def median_beta(values, ref, mv_q, link=None, link_mask=0, ref_conf=None, ref_low=0, kstar=None):
    """beta_n = the median of d over frame n's differing pixels with a prior, as fp32: HELD and OWN split about evenly."""
    v = np.asarray(values)
    kstar = label_rule(v) if kstar is None else kstar
    pre = prior(ref, mv_q, v.shape[1], link, link_mask, ref_conf, ref_low)
    d = margin(v, kstar, pre)
    out = np.zeros(v.shape[0], dtype=np.float32)
    for n in range(v.shape[0]):
        sel = (pre[n] >= 0) & (pre[n] != kstar[n])
        out[n] = np.float32(np.median(d[n][sel])) if sel.any() else np.float32(0)
    return out


def compare(o, labels, hold, stats, n_cls, lut=None):
    """The comparison rule (module docstring): ``o`` the oracle's answer computed on the GPU's k*, the three outputs of one launch as numpy
    arrays -> the number of band pixels decided against the oracle (0 on the same-size route).  Raises AssertionError on a miss."""
    labels, hold, stats = np.asarray(labels), np.asarray(hold), np.asarray(stats)
    free = o["band"]
    assert free.mean() <= BAND_CAP, f"{free.mean():.4%} of the pixels lie within {BAND} of beta"
    assert np.array_equal(hold[~free], o["hold"][~free]), "a pixel outside the band was decided differently"
    assert np.isin(hold[free], (255, 192)).all()
    got = np.where(hold == 255, o["pre"], o["kstar"])                  # every label is c_ref (held) or k*
    assert np.array_equal(labels, got.astype(np.uint8) if lut is None else np.asarray(lut, dtype=np.uint8)[got])
    outcome = np.where(hold == 255, HELD, np.where(hold == 192, OWN, o["outcome"]))
    assert np.array_equal(stats, stats_of(outcome, o["pre"], o["kstar"], n_cls)), "stats differ from what the two planes say"
    return int((hold[free] != o["hold"][free]).sum())


def build(case):
    """The seeded input of a case: tests/consistency_oracle.py's (blob logits with |logit| <= 8, a displaced reference, mv_q with halves in
    play, an off-frame border band, void rectangles) plus a link plane with flagged blocks -- a seeded 12 % of the blocks carry INTRA,
    UNCOVERED or both, another 10 % CLAMPED alone (not in LINK_MASK), all with hop counts in the high nibble -- and a confidence plane of the
    reference with a low-confidence region: a seeded 15 % of its blocks hold codes below REF_LOW.  -> dict(logits, ref, mv, link uint8
    [N,H,W], conf uint8 [R,H,W])."""
    _, seed, N, n_cls, h, w, H, W, align, shared = case
    b = tc.build(case)
    g = np.random.Generator(np.random.PCG64(seed + 1000))
    bs = max(2, min(H, W) // 6)
    by, bx = (H + bs - 1) // bs, (W + bs - 1) // bs
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    R = b["ref"].shape[0]
    link = np.empty((N, H, W), dtype=np.uint8)
    for n in range(N):
        order = g.permutation(by * bx).reshape(by, bx)                  # exactly ceil(12 %) and ceil(10 %) of the blocks, whatever their number
        gated, clamped = np.ceil(0.12 * by * bx), np.ceil(0.10 * by * bx)
        flags = np.where(order < gated, g.integers(1, 4, (by, bx)), np.where(order < gated + clamped, LINK_CLAMPED, 0))
        link[n] = (flags[ys // bs, xs // bs] | (g.integers(0, 16, (H, W)) << 4)).astype(np.uint8)
    conf = np.empty((R, H, W), dtype=np.uint8)
    for r in range(R):
        low = g.permutation(by * bx).reshape(by, bx) < np.ceil(0.15 * by * bx)
        conf[r] = np.where(low[ys // bs, xs // bs], g.integers(0, REF_LOW, (H, W)), g.integers(REF_LOW, 256, (H, W))).astype(np.uint8)
    return {"logits": b["logits"], "ref": b["ref"], "mv": b["mv"], "link": link, "conf": conf}


def solve(case, b=None, kstar=None):
    """A case with both gates on and the median thresholds -> (the input dict with values and beta added, the oracle's answer)."""
    b = build(case) if b is None else b
    H, W, align = case[6], case[7], case[8]
    b["values"] = class_values(b["logits"], H, W, align)
    b["beta"] = median_beta(b["values"], b["ref"], b["mv"], b["link"], LINK_MASK, b["conf"], REF_LOW, kstar)
    return b, stabilise(b["values"], b["ref"], b["mv"], b["beta"], b["link"], LINK_MASK, b["conf"], REF_LOW, kstar)
