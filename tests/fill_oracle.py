"""The contract of arseg_contours_fill_fwd (include/arseg_hip.h) stated on the pixel centres, without the crossing formula: for every pixel
and region the edges of the region's loops that lie at or to the left of the pixel's centre on the centre's row are counted with an
exact orientation test in doubled coordinates (an edge through the centre counts); an odd count covers the pixel (even-odd per region);
the covering region with the largest number gives the value (the painter's rule), the background where none covers.  Hand cases with
the expected planes written out.  Loops are [(region, hole, [(x, y), ...])] as contours_oracle.trace_plane gives them."""
import numpy as np

NSTATS = 3 + 3 * 256
GUARD_I64 = np.int64(-0x5A5A5A5A5A5A5A5B)


def _edges(loops):
    """Every non-horizontal edge, ordered so that ya < yb -> int64 arrays (region, xa, ya, xb, yb)."""
    rows = []
    for region, _, pts in loops:
        pts = [(int(x), int(y)) for x, y in pts]
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if y0 != y1:
                rows.append((region, x0, y0, x1, y1) if y0 < y1 else (region, x1, y1, x0, y0))
    return np.array(rows, dtype=np.int64).reshape(-1, 5).T


def crossings(loops):
    """E: the rows crossed, summed over the edges."""
    _, _, ya, _, yb = _edges(loops)
    return int((yb - ya).sum())


def cover(loops, H, W):
    """-> (k int64 [H,W]: the regions that cover each pixel, owner int64 [H,W]: the largest of them, -1 for none)."""
    region, xa, ya, xb, yb = _edges(loops)
    k, owner = np.zeros((H, W), dtype=np.int64), np.full((H, W), -1, dtype=np.int64)
    dy = yb - ya
    e = np.repeat(np.arange(len(dy)), dy)
    if len(e) == 0:
        return k, owner
    y = ya[e] + np.arange(len(e)) - np.repeat(np.cumsum(dy) - dy, dy)               # 2 ya < 2 y + 1 < 2 yb: the rows ya <= y < yb
    px, py = 2 * np.arange(W)[None, :] + 1, (2 * y + 1)[:, None]
    ax, ay, bx, by = (2 * v[e][:, None] for v in (xa, ya, xb, yb))
    left = ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) <= 0                      # the centre lies right of the edge, or on it
    pairs, inverse = np.unique(region[e] * H + y, return_inverse=True)
    count = np.zeros((len(pairs), W), dtype=np.int64)
    np.add.at(count, inverse.reshape(-1), left)
    inside = count & 1
    np.add.at(k, pairs % H, inside)
    np.maximum.at(owner, pairs % H, np.where(inside == 1, (pairs // H)[:, None], -1))
    return k, owner


def fill(loops, values, H, W, background=255):
    """-> (plane uint8 [H,W], gaps, excess, k)."""
    k, owner = cover(loops, H, W)
    values = np.asarray(values, dtype=np.int64)
    plane = np.where(owner >= 0, values[np.maximum(owner, 0)] & 0xFF if len(values) else 0, background).astype(np.uint8)
    return plane, int((k == 0).sum()), int(np.maximum(k - 1, 0).sum()), k


def stats(plane, k, ref=None):
    """The int64 [NSTATS] row of one frame: gaps, excess, changed, ref_area[256], fill_area[256], both[256]."""
    out = np.zeros(NSTATS, dtype=np.int64)
    covered = k > 0
    out[0], out[1] = (~covered).sum(), np.maximum(k - 1, 0).sum()
    out[3 + 256:3 + 512] = np.bincount(plane[covered], minlength=256)
    if ref is not None:
        out[2] = ((plane != ref) | ~covered).sum()
        out[3:3 + 256] = np.bincount(ref.reshape(-1), minlength=256)
        out[3 + 512:] = np.bincount(plane[covered & (plane == ref)], minlength=256)
    return out


def values_of(plane, loops):
    """The value of every region of trace_plane's loops: an outer loop begins at the top-left corner of its region's first pixel."""
    values = np.zeros(1 + max((r for r, _, _ in loops), default=-1), dtype=np.int64)
    for region, hole, pts in loops:
        if not hole:
            values[region] = plane[pts[0][1], pts[0][0]]
    return values


def records_of(values, rcap=None):
    """int64 [rcap,8] region records holding the values (the other fields are guard words: the pass does not read them)."""
    rec = np.full((len(values) if rcap is None else rcap, 8), GUARD_I64, dtype=np.int64)
    rec[:len(values), 0] = values
    return rec


def _rows(text):
    """"0 0 . 1 / ..." -> owners int [H,W], -1 for '.'."""
    return np.array([[-1 if c == "." else int(c) for c in row.split()] for row in text.split("/")], dtype=np.int64)


_SQ = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]

# name, H, W, loops, owners, gaps, excess, E
HAND = [
    ("two-triangles", 4, 4, [(0, 0, [(0, 0), (4, 0), (0, 4)]), (1, 0, [(4, 0), (4, 4), (0, 4)])],
     "0 0 0 1 / 0 0 1 1 / 0 1 1 1 / 1 1 1 1", 0, 0, 16),
    ("bow-tie", 4, 4, [(0, 0, [(0, 0), (4, 4), (4, 0), (0, 4)])],
     ". . . 0 / 0 . 0 0 / 0 . 0 0 / . . . 0", 8, 0, 16),
    ("square-with-hole", 4, 4, [(0, 0, _SQ(0, 0, 4, 4)), (0, 1, [(1, 1), (1, 3), (3, 3), (3, 1)]), (1, 0, _SQ(1, 1, 3, 3))],
     "0 0 0 0 / 0 1 1 0 / 0 1 1 0 / 0 0 0 0", 0, 0, 16),
    ("overlapping-squares", 5, 5, [(0, 0, _SQ(0, 0, 3, 3)), (1, 0, _SQ(1, 1, 4, 4))],
     "0 0 0 . . / 0 1 1 1 . / 0 1 1 1 . / . 1 1 1 . / . . . . .", 11, 4, 12),
    ("loop-twice", 2, 2, [(0, 0, _SQ(0, 0, 2, 2)), (0, 0, _SQ(0, 0, 2, 2))],
     ". . / . .", 4, 0, 8),
    ("two-vertex-loop", 2, 2, [(0, 0, _SQ(0, 0, 2, 2)), (1, 0, [(0, 0), (2, 2)])],
     "0 0 / 0 0", 0, 0, 8),
    ("edge-over-all-rows", 5, 3, [(0, 0, [(0, 0), (3, 0), (0, 5)])],
     "0 0 0 / 0 0 . / 0 . . / 0 . . / . . .", 8, 0, 10),
    ("edge-along-x-W", 2, 3, [(0, 0, _SQ(1, 0, 3, 2))],
     ". 0 0 / . 0 0", 2, 0, 4),
]
HAND_IDS = [h[0] for h in HAND]
HAND_VALUES = np.array([7, 200], dtype=np.int64)          # region 0 and 1 of every hand case


def hand_plane(case, background=255):
    """The expected plane of a hand case."""
    owners = _rows(case[4])
    return np.where(owners >= 0, HAND_VALUES[np.maximum(owners, 0)], background).astype(np.uint8)


def bar_loops(counts, regions=3):
    """Loops whose row i is crossed exactly counts[i] times: counts[i] / 2 unit squares over every other column, dealt to ``regions``
    regions in turn -> (loops, H, W)."""
    loops = []
    for i, c in enumerate(counts):
        assert c % 2 == 0
        loops += [(j % regions, 0, _SQ(2 * j, i, 2 * j + 1, i + 1)) for j in range(c // 2)]
    return loops, len(counts), max(max(counts), 1)
