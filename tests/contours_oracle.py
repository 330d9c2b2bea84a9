"""Oracle of arseg_rle_contours_fwd (include/arseg_hip.h), written from the contract and independent of run walking: it works on the pixel
plane.  The region ids of links_oracle.region_planes, one directed unit edge per pixel side that faces another region or the border (the
region on the right hand, y down), the edges linked at every grid corner with the turn rule, the cycles traced, collinear vertices
dropped, every loop rotated to its smallest vertex and the loops sorted as the contract says.  Whether a loop is a hole is read off the sign
of its shoelace area, not off the run it starts at.  Independent of arseg_amd.egress.contours_numpy (which is tested against it).
Everything is an integer: the tests compare with np.array_equal.  Also the refusal and capacity rules (``expected``), the hand-made planes
with their loops written out literally, and the inputs both test files use."""
import numpy as np

import links_oracle
import regions_oracle
import rle_oracle

GUARD_I32 = regions_oracle.GUARD_I32
GUARD_WORD = rle_oracle.GUARD_WORD

# a pixel side -> (the neighbour across it, the edge's start and end corner relative to the pixel): the pixel lies on the right hand
_SIDES = (((0, -1), (0, 0), (1, 0)),          # top: heading east
          ((1, 0), (1, 0), (1, 1)),           # right: heading south
          ((0, 1), (1, 1), (0, 1)),           # bottom: heading west
          ((-1, 0), (0, 1), (0, 0)))          # left: heading north


def shoelace2(points):
    """Twice the signed area of a closed polygon of (x, y) points: positive for a loop that runs clockwise on the screen (y down)."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    return int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


def trace_plane(plane, connectivity=8):
    """One plane uint8 [H,W] -> the loops of the frame in canonical order: [(region, hole, [(x, y), ...])]."""
    assert connectivity in (4, 8)
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    H, W = plane.shape
    reg = links_oracle.region_planes(plane[None], connectivity)[0]["reg"]
    out = {}                                                      # (region, start corner) -> [(heading, end corner)]
    for y in range(H):
        for x in range(W):
            r = int(reg[y, x])
            for (dx, dy), (sx, sy), (ex, ey) in _SIDES:
                qx, qy = x + dx, y + dy
                if 0 <= qx < W and 0 <= qy < H and reg[qy, qx] == r:
                    continue
                start, end = (x + sx, y + sy), (x + ex, y + ey)
                out.setdefault((r, start), []).append(((ex - sx, ey - sy), end))
    seen = set()
    loops = []
    for (r, start) in sorted(out):
        for heading, end in out[(r, start)]:
            if (r, start, heading) in seen:
                continue
            corners = []
            at, h, nxt = start, heading, end
            while (r, at, h) not in seen:
                seen.add((r, at, h))
                options = out[(r, nxt)]
                if len(options) == 1:
                    h2, end2 = options[0]
                else:                                             # a saddle: the region holds the two diagonal pixels at this corner
                    assert len(options) == 2
                    want = (h[1], -h[0]) if connectivity == 8 else (-h[1], h[0])          # left : right of the heading
                    (h2, end2), = [o for o in options if o[0] == want]
                if h2 != h:
                    corners.append(nxt)
                at, h, nxt = nxt, h2, end2
            assert (at, h) == (start, heading)                    # the walk closes where it began
            k = min(range(len(corners)), key=lambda i: (corners[i][1], corners[i][0]))
            corners = corners[k:] + corners[:k]
            area2 = shoelace2(corners)
            assert area2 != 0
            loops.append((r, 1 if area2 < 0 else 0, corners))
    loops.sort(key=lambda l: (l[2][0][1], l[2][0][0], -l[1]))     # rising first vertex in (y, x) order, the hole first
    return loops


def arrays(loops):
    """trace_plane's loops -> (counts int32 [2] = {L, V}, loops int32 [L,4] = {region, first, count, hole}, verts uint32 [V] = y << 16 | x)."""
    rec = np.zeros((len(loops), 4), dtype=np.int32)
    words = []
    for k, (r, hole, corners) in enumerate(loops):
        rec[k] = (r, len(words), len(corners), hole)
        words += [(y << 16) | x for x, y in corners]
    return np.array([len(loops), len(words)], dtype=np.int32), rec, np.array(words, dtype=np.uint32)


def contour_plane(plane, connectivity=8):
    """One plane -> (counts, loops, verts) as arseg_rle_contours_fwd leaves them with room for everything."""
    return arrays(trace_plane(plane, connectivity))


def expected(answer, processable, lcap, vcap, counts_before, loops_before, verts_before):
    """What the buffers of one frame hold after the call.  answer: contour_plane's; processable: the run code did not overflow and
    n_regions >= 0; the three buffers as they were -> (counts [2], loops [lcap,4], verts [vcap]).  Not processable: counts = {-1, -1} and
    nothing else is touched; otherwise counts exact, the rows below min(L, lcap) and the words below min(V, vcap) exact, the rest untouched."""
    counts = np.array(counts_before, dtype=np.int32, copy=True)
    loops = np.array(loops_before, dtype=np.int32, copy=True).reshape(lcap, 4)
    verts = np.array(verts_before, dtype=np.uint32, copy=True)
    if not processable:
        counts[:] = -1
        return counts, loops, verts
    counts[:] = answer[0]
    l, v = min(len(answer[1]), lcap), min(len(answer[2]), vcap)
    loops[:l] = answer[1][:l]
    verts[:v] = answer[2][:v]
    return counts, loops, verts


def polygons(answer):
    """(counts, loops, verts) -> [(region, hole, int32 [k,2] of (x, y))], what ContourFrames.to_host gives for the frame."""
    _, loops, verts = answer
    return [(int(r), int(hole), np.stack([verts[f:f + c] & 0xFFFF, verts[f:f + c] >> 16], axis=1).astype(np.int32)) for r, f, c, hole in loops]


def fill_even_odd(polys, H, W):
    """The pixels inside a set of loops by the even-odd rule -> bool [H,W]: pixel (x, y) is inside iff a ray from its centre to the left
    crosses an odd number of the loops' vertical edges."""
    crossings = np.zeros((H, W + 1), dtype=np.int64)
    for pts in polys:
        nxt = np.roll(pts, -1, axis=0)
        for (x0, y0), (x1, y1) in zip(pts, nxt):
            if x0 == x1:
                crossings[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(crossings, axis=1)[:, :W] % 2) == 1


def _p(rows):
    return np.array(rows, dtype=np.uint8)


_O = lambda r, pts: (r, 0, pts)
_HOLE = lambda r, pts: (r, 1, pts)
_UNIT = lambda x, y: [(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]

_DIAG = [[1, 0], [0, 1]]
_L = [[1, 0, 0], [1, 0, 0], [1, 1, 1]]
_TWO_HOLES = [[5] * 7, [5, 0, 5, 5, 2, 2, 5], [5, 0, 5, 5, 2, 2, 5], [5] * 7]
_CUP = [[3] * 5, [3, 0, 3, 0, 3], [3, 0, 0, 0, 3], [3] * 5]

# Hand-made planes with the loops written out (not computed by this file): name -> (plane rows, {connectivity: [(region, hole, [(x, y)])]}).
# Regions are numbered in the raster order of their first pixel.
_BOTH = lambda answer: {4: answer, 8: answer}
HAND = {
    "one-pixel": ([[7]], _BOTH([_O(0, [(0, 0), (1, 0), (1, 1), (0, 1)])])),
    "centre": ([[5, 5, 5], [5, 9, 5], [5, 5, 5]],
               _BOTH([_O(0, [(0, 0), (3, 0), (3, 3), (0, 3)]), _HOLE(0, [(1, 1), (1, 2), (2, 2), (2, 1)]), _O(1, [(1, 1), (2, 1), (2, 2), (1, 2)])])),
    # the two diagonals: one region each at 8-connectivity, whose loops pass through the centre twice; four pixels at 4-connectivity
    "diagonal": (_DIAG, {8: [_O(0, [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]),
                             _O(1, [(1, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1), (1, 1)])],
                         4: [_O(0, _UNIT(0, 0)), _O(1, _UNIT(1, 0)), _O(2, _UNIT(0, 1)), _O(3, _UNIT(1, 1))]}),
    # straight continuation across rows gives no vertex: the left side of the L is one edge from (0, 3) to (0, 0)
    "l-shape": (_L, _BOTH([_O(0, [(0, 0), (1, 0), (1, 2), (3, 2), (3, 3), (0, 3)]), _O(1, [(1, 0), (3, 0), (3, 2), (1, 2)])])),
    "two-holes": (_TWO_HOLES, _BOTH([_O(0, [(0, 0), (7, 0), (7, 4), (0, 4)]), _HOLE(0, [(1, 1), (1, 3), (2, 3), (2, 1)]),
                                     _O(1, [(1, 1), (2, 1), (2, 3), (1, 3)]), _HOLE(0, [(4, 1), (4, 3), (6, 3), (6, 1)]),
                                     _O(2, [(4, 1), (6, 1), (6, 3), (4, 3)])])),
    # a hole shaped like a cup: two prongs in one row, joined below
    "cup-hole": (_CUP, _BOTH([_O(0, [(0, 0), (5, 0), (5, 4), (0, 4)]),
                              _HOLE(0, [(1, 1), (1, 3), (4, 3), (4, 1), (3, 1), (3, 2), (2, 2), (2, 1)]),
                              _O(1, [(1, 1), (2, 1), (2, 2), (3, 2), (3, 1), (4, 1), (4, 3), (1, 3)])])),
    "one-row": ([[4, 4, 9, 4, 4, 4]], _BOTH([_O(0, [(0, 0), (2, 0), (2, 1), (0, 1)]), _O(1, [(2, 0), (3, 0), (3, 1), (2, 1)]),
                                             _O(2, [(3, 0), (6, 0), (6, 1), (3, 1)])])),
    "one-column": ([[1], [1], [2], [1]], _BOTH([_O(0, [(0, 0), (1, 0), (1, 2), (0, 2)]), _O(1, [(0, 2), (1, 2), (1, 3), (0, 3)]),
                                                _O(2, [(0, 3), (1, 3), (1, 4), (0, 4)])])),
}
HAND_IDS = list(HAND)


def hand_plane(name):
    return _p(HAND[name][0])


def hand_arrays(name, connectivity):
    return arrays(HAND[name][1][connectivity])


# one long loop each, the worst case of the pointer jumping: the spiral's wall and corridor (222 and 182 run ends, more than a wave), the
# comb's 40 teeth (162) and a larger spiral whose wall has more run ends than a workgroup has threads (tests/test_contours.py asserts it)
LONG = {"spiral-21x21": regions_oracle.HAND["spiral-21x21"][0], "comb-40-teeth": regions_oracle.HAND["comb-40-teeth"][0],
        "spiral-33x33": regions_oracle._spiral(33, 6, 1)}


def cpu_planes():
    """The planes of the CPU checks: (name, uint8 [H,W])."""
    out = [(name, hand_plane(name)) for name in HAND_IDS] + [(name, np.ascontiguousarray(p)) for name, p in LONG.items()]
    for case in rle_oracle.CASES:
        out += [("%s-%d" % (case[0], n), p) for n, p in enumerate(rle_oracle.build(case))]
    out += [("noise-%d" % n, p) for n, p in enumerate(regions_oracle.noise_planes(*regions_oracle.NOISE))]
    out += [("dense-%d" % n, p) for n, p in enumerate(regions_oracle.dense_noise(41, 2, 12, 33))]
    return out


def device_inputs(planes, cap=None, connectivity=8, extra=3):
    """links_oracle.device_inputs: (row_start, runs, n_regions, run_region) as arseg_labels_rle_fwd + arseg_rle_regions_fwd leave them."""
    return links_oracle.device_inputs(np.ascontiguousarray(planes), cap, connectivity, extra)
