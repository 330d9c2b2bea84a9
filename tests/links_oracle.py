"""Oracle of arseg_region_links_fwd (include/arseg_hip.h), written from the contract: the per-pixel rule restated on region-id planes (taken
from regions_oracle.label_planes, the rounding from consistency_oracle.round_half_even_div4), the pairs counted into a dense matrix of
(region, reference region) and every record read off that matrix.  Independent of arseg_amd.egress.links_numpy (which is tested against it).
Everything is an integer: the tests compare with np.array_equal.  Also the -1 / -2 / capacity rules (``expected``), the hand-made cases with
their links written out literally, and the inputs both test files use."""
import numpy as np

import consistency_oracle
import regions_oracle
import rle_oracle

GUARD_I32 = regions_oracle.GUARD_I32
GUARD_I64 = regions_oracle.GUARD_I64
LINK_FIELDS = ("ref_region", "overlap", "same", "outside", "mutual", "n_ref")
BACK_FIELDS = ("cur_region", "overlap", "covered", "n_cur")


def region_planes(planes, connectivity=8):
    """uint8 [N,H,W] -> per frame a dict: row_start [H+1], runs [needed], R, run_region [needed] and reg, the region number of every pixel
    int64 [H,W]."""
    planes = np.ascontiguousarray(planes)
    N, H, W = planes.shape
    row_start, runs = rle_oracle.encode(planes)
    out = []
    for n in range(N):
        R, rr, _ = regions_oracle.label(row_start[n], runs[n], H, W, connectivity)
        reg = np.empty((H, W), dtype=np.int64)
        for y in range(H):
            for i in range(row_start[n, y], row_start[n, y + 1]):
                x0 = int(runs[n][i]) >> 8
                x1 = int(runs[n][i + 1]) >> 8 if i + 1 < row_start[n, y + 1] else W
                reg[y, x0:x1] = rr[i]
        out.append({"row_start": row_start[n], "runs": runs[n], "R": R, "run_region": rr, "reg": reg})
    return out


def link_frame(val, reg, R, rval, rreg, K, mv):
    """One frame: its value and region planes [H,W], R; the reference's, K; mv int16 [H,W,2] or None -> (n_pairs, links int64 [R,6],
    back int64 [K,4])."""
    H, W = val.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    tx, ty = xs.copy(), ys.copy()
    if mv is not None:
        assert mv.dtype == np.int16 and mv.shape == (H, W, 2)
        tx, ty = xs + consistency_oracle.round_half_even_div4(mv[..., 0]), ys + consistency_oracle.round_half_even_div4(mv[..., 1])
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    pairs = np.zeros((R, K), dtype=np.int64)
    outside = np.zeros(R, dtype=np.int64)
    for y, x in zip(*np.nonzero(~inside)):
        outside[reg[y, x]] += 1
    sy, sx = np.nonzero(inside)
    same = rval[ty[sy, sx], tx[sy, sx]] == val[sy, sx]
    np.add.at(pairs, (reg[sy, sx][same], rreg[ty[sy, sx], tx[sy, sx]][same]), 1)
    links = np.zeros((R, 6), dtype=np.int64)
    back = np.zeros((K, 4), dtype=np.int64)
    for k in range(K):
        col = pairs[:, k]
        best = int(np.argmax(col))                                # the first of equal maxima: the smaller r
        back[k] = (best if col[best] > 0 else -1, col[best], col.sum(), np.count_nonzero(col))
    for r in range(R):
        row = pairs[r]
        best = int(np.argmax(row))                                # the smaller k
        k = best if row[best] > 0 else -1
        links[r] = (k, row[best], row.sum(), outside[r], 1 if k >= 0 and back[k, 0] == r else 0, np.count_nonzero(row))
    return int(np.count_nonzero(pairs)), links, back


def link_planes(cur, ref, mv_q=None, connectivity=8):
    """cur uint8 [N,H,W], ref uint8 [1,H,W] (shared) or [N,H,W], mv_q int16 [N,H,W,2] or None -> [(n_pairs, links, back)] per frame."""
    cur, ref = np.ascontiguousarray(cur), np.ascontiguousarray(ref)
    N = cur.shape[0]
    assert ref.shape[0] in (1, N) and ref.shape[1:] == cur.shape[1:]
    a, b = region_planes(cur, connectivity), region_planes(ref, connectivity)
    out = []
    for n in range(N):
        m = n if ref.shape[0] > 1 else 0
        out.append(link_frame(cur[n].astype(np.int64), a[n]["reg"], a[n]["R"], ref[m].astype(np.int64), b[m]["reg"], b[m]["R"],
                              None if mv_q is None else mv_q[n]))
    return out


def expected(answer, linkable, rcap, kcap, pcap, links_before, back_before):
    """What the buffers of one frame hold after the call.  answer: link_frame's; linkable: neither run code overflowed and both n_regions
    entries are >= 0; links_before [rcap,6] / back_before [kcap,4]: the buffers as they were -> (n_pairs, links, back).  Not linkable: -1
    and nothing is touched; more than pcap distinct pairs: -2 and nothing is touched; otherwise the rows below min(R, rcap) and
    min(R_ref, kcap) are exact and the rows from there on untouched."""
    links, back = np.array(links_before, dtype=np.int64, copy=True), np.array(back_before, dtype=np.int64, copy=True)
    n_pairs, want_links, want_back = answer
    if not linkable:
        return -1, links, back
    if n_pairs > pcap:
        return -2, links, back
    r, k = min(len(want_links), rcap), min(len(want_back), kcap)
    links[:r] = want_links[:r]
    back[:k] = want_back[:k]
    return n_pairs, links, back


def device_inputs(planes, cap=None, connectivity=8, extra=3):
    """The four arrays of one side as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them, made on the host: (row_start int32 [N,H+1],
    runs uint32 [N,cap], n_regions int32 [N], run_region int32 [N,cap]).  cap: default room for every run and ``extra`` more; a frame that
    needs more than cap runs is left as the device leaves it (the stored words, n_regions = -1, run_region untouched).  The words and region
    numbers beyond the needed runs hold guard values."""
    sides = region_planes(planes, connectivity)
    N, H = len(sides), planes.shape[1]
    cap = max(len(s["runs"]) for s in sides) + extra if cap is None else cap
    row_start = np.stack([s["row_start"] for s in sides]).astype(np.int32)
    runs = np.full((N, cap), rle_oracle.GUARD_WORD, dtype=np.uint32)
    n_regions = np.zeros(N, dtype=np.int32)
    run_region = np.full((N, cap), GUARD_I32, dtype=np.int32)
    for n, s in enumerate(sides):
        need = len(s["runs"])
        runs[n, :min(need, cap)] = s["runs"][:cap]
        if need > cap:
            n_regions[n] = -1
        else:
            n_regions[n] = s["R"]
            run_region[n, :need] = s["run_region"]
    return row_start, runs, n_regions, run_region


def block_motion(seed, N, H, W, block=8, amp=None):
    """Block-constant quarter-pel motion int16 [N,H,W,2] (blocks of ``block`` pixels, what a decoder delivers), uniform in +-amp pixels
    (default: +-W, so that whole rows leave the frame), fractions included."""
    g = np.random.Generator(np.random.PCG64(seed))
    amp = W if amp is None else amp
    by, bx = -(-H // block), -(-W // block)
    coarse = g.integers(-4 * amp, 4 * amp + 1, (N, by, bx, 2))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, axis=1), block, axis=2)[:, :H, :W].astype(np.int16))


def uniform_motion(N, H, W, dx_px, dy_px):
    mv = np.empty((N, H, W, 2), dtype=np.int16)
    mv[..., 0], mv[..., 1] = 4 * dx_px, 4 * dy_px
    return mv


def _p(rows):
    return np.array(rows, dtype=np.uint8)


_TWO = _p([[1, 1, 1, 2, 2, 2], [1, 1, 1, 2, 2, 2], [3, 3, 3, 3, 3, 3], [3, 3, 3, 3, 3, 3]])
_CORNER = _p([[5, 5, 5, 5, 5, 5], [5, 5, 5, 5, 5, 5], [5, 5, 5, 7, 7, 7], [5, 5, 5, 7, 7, 7]])
_BAR = _p([[0] * 8, [0, 9, 9, 9, 9, 9, 9, 0], [0] * 8])
_CUT = _p([[0] * 8, [0, 9, 9, 4, 4, 9, 9, 0], [0] * 8])
_A, _B, _C = _p([[1, 1, 2, 2]] * 2), _p([[1, 1, 3, 3]] * 2), _p([[5, 5, 3, 3]] * 2)
_WIDE = _p([[1] * 60 + [2] * 10 + [1] * 60] * 2)
_ROUND_MV = np.zeros((1, 1, 8, 2), dtype=np.int16)
_ROUND_MV[0, 0, :5, 0] = (2, 6, -2, -6, 10)                     # 0.5 -> 0, 1.5 -> 2, -0.5 -> 0, -1.5 -> -2, 2.5 -> 2
_NONE4, _NONE6 = (-1, 0, 0, 0), (-1, 0, 0, 0, 0, 0)

# Hand-made cases with the answer written out (not computed by this file): name -> (cur [N,H,W], ref [1 or N,H,W], mv_q or None, per frame
# (n_pairs, links rows {ref_region, overlap, same, outside, mutual, n_ref}, back rows {cur_region, overlap, covered, n_cur})).
# 8-connectivity; regions are numbered in the raster order of their first pixel.
HAND = {
    # every region finds itself
    "identity": (_TWO[None], _TWO[None], None, [(3, [(0, 6, 6, 0, 1, 1), (1, 6, 6, 0, 1, 1), (2, 12, 12, 0, 1, 1)],
                                                 [(0, 6, 6, 1), (1, 6, 6, 1), (2, 12, 12, 1)])]),
    # target = (x + 3, y - 2): rows 0 and 1 leave at the top (12 pixels of region 0), columns 3 .. 5 of rows 2 and 3 at the right (region 1);
    # the 6 pixels left of region 0 land on region 0
    "translation": (_CORNER[None], _CORNER[None], uniform_motion(1, 4, 6, 3, -2),
                    [(1, [(0, 6, 6, 12, 1, 1), (-1, 0, 0, 6, 0, 0)], [(0, 6, 6, 1), _NONE4])]),
    # the bar (reference region 1) cut into two equal halves (regions 1 and 3) by another class (region 2): both link to it, the tie in
    # back goes to the smaller r, so exactly one half is mutual
    "split": (_CUT[None], _BAR[None], None, [(3, [(0, 18, 18, 0, 1, 1), (1, 2, 2, 0, 1, 1), _NONE6, (1, 2, 2, 0, 0, 1)],
                                              [(0, 18, 18, 1), (1, 2, 4, 2)])]),
    "merge": (_BAR[None], _CUT[None], None, [(3, [(0, 18, 18, 0, 1, 1), (1, 2, 4, 0, 1, 2)],
                                              [(0, 18, 18, 1), (1, 2, 2, 1), _NONE4, (1, 2, 2, 1)])]),
    # the same shape with another value links to nothing
    "class-change": (_B[None], _A[None], None, [(1, [(0, 4, 4, 0, 1, 1), _NONE6], [(0, 4, 4, 1), _NONE4])]),
    # two reference regions of one value under one region, two pixels each: the smaller k
    "reference-tie": (_p([[7, 7, 7, 7, 7]])[None], _p([[7, 7, 0, 7, 7]])[None], None,
                      [(2, [(0, 2, 4, 0, 1, 2)], [(0, 2, 2, 1), _NONE4, (0, 2, 2, 1)])]),
    # one pixel per region on both sides; the values of the current row are those of its targets under round-half-even only.  Columns 4
    # and 6 both land on reference region 6: it keeps the smaller r
    "rounding": (_p([[10, 13, 12, 11, 16, 15, 16, 17]])[None], _p([[10, 11, 12, 13, 14, 15, 16, 17]])[None], _ROUND_MV,
                 [(8, [(0, 1, 1, 0, 1, 1), (3, 1, 1, 0, 1, 1), (2, 1, 1, 0, 1, 1), (1, 1, 1, 0, 1, 1), (6, 1, 1, 0, 1, 1), (5, 1, 1, 0, 1, 1),
                       (6, 1, 1, 0, 0, 1), (7, 1, 1, 0, 1, 1)],
                   [(0, 1, 1, 1), (3, 1, 1, 1), (2, 1, 1, 1), (1, 1, 1, 1), _NONE4, (5, 1, 1, 1), (4, 1, 2, 2), (7, 1, 1, 1)])]),
    # region 1 covers columns 60 .. 69 and region 2 columns 70 .. 129 of both rows: their pairs straddle x = 63 | 64 and 127 | 128
    "wave-boundary": (_WIDE[None], _WIDE[None], None, [(3, [(0, 120, 120, 0, 1, 1), (1, 20, 20, 0, 1, 1), (2, 120, 120, 0, 1, 1)],
                                                        [(0, 120, 120, 1), (1, 20, 20, 1), (2, 120, 120, 1)])]),
    "shared-reference": (np.stack([_A, _B]), _A[None], None, [(2, [(0, 4, 4, 0, 1, 1), (1, 4, 4, 0, 1, 1)], [(0, 4, 4, 1), (1, 4, 4, 1)]),
                                                               (1, [(0, 4, 4, 0, 1, 1), _NONE6], [(0, 4, 4, 1), _NONE4])]),
    "per-frame-references": (np.stack([_A, _B]), np.stack([_B, _C]), None, [(1, [(0, 4, 4, 0, 1, 1), _NONE6], [(0, 4, 4, 1), _NONE4]),
                                                                             (1, [_NONE6, (1, 4, 4, 0, 1, 1)], [_NONE4, (1, 4, 4, 1)])]),
}
HAND_IDS = list(HAND)

# H = 3 at the widths around a wave, and small heights at W = 16: (H, W)
EDGE_SHAPES = [(3, 1), (3, 63), (3, 64), (3, 65), (3, 129), (1, 16), (2, 16), (5, 16)]
# dense three-valued noise with more than 256 distinct pairs per frame (tests/test_links.py asserts it): seed, N, H, W
DENSE = (21, 2, 64, 65)
