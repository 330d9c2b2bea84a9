"""Oracle of arseg_contours_simplify_shared_fwd (include/arseg_hip.h), written from the contract on the pixel plane: the degree of a grid
corner read off the four pixels around it, the loops of contours_oracle.trace_plane walked a unit step at a time to find the junctions
inside their straight edges, the expanded loops cut into arcs at every junction passage, and per arc the plain recursion on lists of
Python-int points with the direction-free tie rule (the smallest vertex word).  No run code, no flags, no walk: nothing is shared with
arseg_amd.egress.simplify_shared_numpy (which is tested against it) or with the kernel.  Also the hand-made planes with the kept loops
written out literally, the matching check, and the planes that put junctions inside long edges."""
import sys

import numpy as np

import contours_oracle
import simplify_oracle

GUARD_I32 = simplify_oracle.GUARD_I32
GUARD_WORD = simplify_oracle.GUARD_WORD
TOLERANCES = simplify_oracle.TOLERANCES
TOL2_QS = simplify_oracle.TOL2_QS
expected = simplify_oracle.expected
loops_of = simplify_oracle.loops_of

sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))          # _chain recurses as deep as an arc is long, at the worst


def _value(plane, x, y):
    H, W = plane.shape
    return int(plane[y, x]) if 0 <= x < W and 0 <= y < H else None


def degree(plane, x, y):
    """The border edges among the four unit grid edges at corner (x, y): an edge is one if its two pixels differ in value, or if exactly
    one of them lies outside the frame."""
    a, b, c, d = _value(plane, x - 1, y - 1), _value(plane, x, y - 1), _value(plane, x - 1, y), _value(plane, x, y)
    return sum(1 for p, q in ((a, b), (c, d), (a, c), (b, d)) if p != q)          # None == None: both outside, no border


def is_junction(plane, x, y):
    H, W = plane.shape
    return degree(plane, x, y) >= 3 or (x in (0, W) and y in (0, H))


def expand(plane, points):
    """One loop of corners -> the expanded loop: [((x, y), is a junction passage)], with the junctions strictly inside its edges added."""
    out = []
    for (x0, y0), (x1, y1) in zip(points, points[1:] + points[:1]):
        assert (x0 == x1) != (y0 == y1)
        sx, sy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
        out.append(((x0, y0), is_junction(plane, x0, y0)))
        x, y = x0 + sx, y0 + sy
        while (x, y) != (x1, y1):
            if is_junction(plane, x, y):
                out.append(((x, y), True))
            x, y = x + sx, y + sy
    return out


def _word(p):
    return (p[1] << 16) | p[0]


def _cross(p, a, b):
    return abs((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]))


def _chain(P, a, b, tol2_q):
    """The interior positions of the segment (a, b) of an arc that are kept: the largest c, the smallest vertex word of a tie."""
    if b - a < 2:
        return []
    c, at = max(((_cross(P[i], P[a], P[b]), -_word(P[i])), i) for i in range(a + 1, b))
    if 16 * c[0] * c[0] <= tol2_q * ((P[b][0] - P[a][0]) ** 2 + (P[b][1] - P[a][1]) ** 2):
        return []
    return _chain(P, a, at, tol2_q) + [at] + _chain(P, at, b, tol2_q)


def arc_kept(P, tol2_q):
    """The points P[0..m] of one arc -> the positions below m that are kept, rising (P[m] belongs to the next arc)."""
    m = len(P) - 1
    if P[0] != P[m]:
        return [0] + _chain(P, 0, m, tol2_q)
    _, a1 = max((((P[i][0] - P[0][0]) ** 2 + (P[i][1] - P[0][1]) ** 2, -_word(P[i])), i) for i in range(m))
    kept = [0] + _chain(P, 0, a1, tol2_q) + [a1] + _chain(P, a1, m, tol2_q)
    return kept if len(kept) >= 3 else list(range(m))


def arcs_of(expanded):
    """An expanded loop -> its arcs as (first position, length m), in order from the first junction passage (position 0 without one)."""
    n = len(expanded)
    cuts = [i for i, (_, junction) in enumerate(expanded) if junction]
    if not cuts:
        return [(0, n)]
    return [(a, (b - a) if b > a else b + n - a) for a, b in zip(cuts, cuts[1:] + cuts[:1])]


def on_frame(plane, P):
    """An arc lies on the frame: all its points on one of the four frame lines (it is then one straight piece between two junctions)."""
    H, W = plane.shape
    return any(all(p[axis] == line for p in P) for axis, line in ((0, 0), (0, W), (1, 0), (1, H)))


def simplify_plane(plane, connectivity, tol2_q, source=None):
    """One plane -> ([(region, hole, [(x, y)])] of the kept loops, [(p, q)] the directed output segments of the arcs not on the frame,
    [[(x, y)]] the expanded loops, [[position]] the kept positions in them)."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    source = contours_oracle.trace_plane(plane, connectivity) if source is None else source
    loops, segments, expanded_loops, kept_positions = [], [], [], []
    for region, hole, pts in source:
        ex = expand(plane, [(int(x), int(y)) for x, y in pts])
        n = len(ex)
        keep = set()
        for first, m in arcs_of(ex):
            P = [ex[(first + i) % n][0] for i in range(m + 1)]
            kept = arc_kept(P, tol2_q)
            keep.update((first + i) % n for i in kept)
            if not on_frame(plane, P):
                chain = [P[i] for i in kept] + [P[m]]
                segments += list(zip(chain, chain[1:]))
        positions = sorted(keep)
        loops.append((region, hole, [ex[i][0] for i in positions]))
        expanded_loops.append([p for p, _ in ex])
        kept_positions.append(positions)
    return loops, segments, expanded_loops, kept_positions


def simplify_frame(plane, connectivity, tol2_q, source=None):
    """One plane -> (counts, loops, verts) as arseg_contours_simplify_shared_fwd leaves them with room for everything."""
    return contours_oracle.arrays(simplify_plane(plane, connectivity, tol2_q, source)[0])


def unmatched(segments):
    """Directed segments [(p, q)] -> those whose count differs from the count of their reverse (each once)."""
    count = {}
    for s in segments:
        count[s] = count.get(s, 0) + 1
    return sorted(s for s in count if count[s] != count.get((s[1], s[0]), 0))


def interior_segments(plane, loops):
    """The directed segments of output loops that do not lie on a frame line (for output whose arcs are not known)."""
    out = []
    for _, _, pts in loops:
        out += [(p, q) for p, q in zip(pts, pts[1:] + pts[:1]) if not on_frame(plane, [p, q])]
    return out


def _p(rows):
    return np.array(rows, dtype=np.uint8)


_O = lambda r, pts: (r, 0, pts)
_HOLE = lambda r, pts: (r, 1, pts)
_BIG = 1 << 20
_HEAD = [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]]
_FRAMED = [[5] * 8] + [[5] + [1 if x <= y else 2 for x in range(6)] + [5] for y in range(6)] + [[5] * 8]
_CUP_OUT = _O(0, [(0, 0), (5, 0), (5, 4), (0, 4)])
# at 8 the two 1-regions are joined across the saddle (2, 2), and so are the 0 pixels: the head's other side is a hole of region 0
_HEAD_8 = [_O(0, [(0, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4)]), _HOLE(0, [(1, 1), (1, 2), (2, 2), (2, 1)]),
           _O(1, [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (2, 4), (2, 2), (1, 2)])]

# Hand-made planes with the kept loops written out (not computed by this file): (name, plane rows, connectivity, tol2_q, loops).
HAND = [
    # the T at (1, 1) is inside region 0's bottom edge: it is inserted, and stays at every tolerance
    ("t-horizontal", [[1, 1], [2, 3]], 8, 0, [_O(0, [(0, 0), (2, 0), (2, 1), (1, 1), (0, 1)]), _O(1, [(0, 1), (1, 1), (1, 2), (0, 2)]),
                                              _O(2, [(1, 1), (2, 1), (2, 2), (1, 2)])]),
    ("t-horizontal", [[1, 1], [2, 3]], 8, _BIG, [_O(0, [(0, 0), (2, 0), (2, 1), (1, 1), (0, 1)]), _O(1, [(0, 1), (1, 1), (1, 2), (0, 2)]),
                                                 _O(2, [(1, 1), (2, 1), (2, 2), (1, 2)])]),
    ("t-vertical", [[1, 2], [1, 3]], 8, 0, [_O(0, [(0, 0), (1, 0), (1, 1), (1, 2), (0, 2)]), _O(1, [(1, 0), (2, 0), (2, 1), (1, 1)]),
                                            _O(2, [(1, 1), (2, 1), (2, 2), (1, 2)])]),
    # the staircase is one open arc (1, 0) .. (6, 5) for both neighbours: at 0.5 px the last step goes (the chord (4, 4) - (6, 5))
    ("stairs", simplify_oracle._STAIRS, 8, 4, [
        _O(0, [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (6, 5), (6, 6), (0, 6)]),
        _O(1, [(1, 0), (6, 0), (6, 5), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)])]),
    ("stairs", simplify_oracle._STAIRS, 8, 16, [_O(0, [(0, 0), (1, 0), (6, 5), (6, 6), (0, 6)]), _O(1, [(1, 0), (6, 0), (6, 5)])]),
    ("plus", simplify_oracle._PLUS, 8, 16, [
        _O(0, [(0, 0), (1, 0), (0, 1)]), _O(1, [(1, 0), (2, 0), (3, 1), (3, 2), (2, 3), (1, 3), (0, 2), (0, 1)]), _O(2, [(2, 0), (3, 0), (3, 1)]),
        _O(3, [(0, 2), (1, 3), (0, 3)]), _O(4, [(3, 2), (3, 3), (2, 3)])]),
    ("notch", [[0, 0, 0], [0, 1, 0]], 8, 4, [_O(0, [(0, 0), (3, 0), (3, 2), (2, 2), (2, 1), (1, 1), (1, 2), (0, 2)]),
                                             _O(1, [(1, 1), (2, 1), (2, 2), (1, 2)])]),
    # a degenerate loop: the notch is thinner than 1 px, its open arc (1, 2) .. (2, 2) collapses onto its chord on both sides
    ("notch", [[0, 0, 0], [0, 1, 0]], 8, 16, [_O(0, [(0, 0), (3, 0), (3, 2), (2, 2), (1, 2), (0, 2)]), _O(1, [(2, 2), (1, 2)])]),
    # one closed arc from (1, 1): the hole and the region inside it keep the same prong corners, (2, 1) and (2, 2)
    ("cup", contours_oracle._CUP, 8, 4, [_CUP_OUT, _HOLE(0, [(1, 1), (1, 3), (4, 3), (4, 1), (2, 2), (2, 1)]),
                                         _O(1, [(1, 1), (2, 1), (2, 2), (4, 1), (4, 3), (1, 3)])]),
    # the one-pixel head hangs on the saddle (2, 2): a closed arc between two passages of that point, kept whole (fewer than 3 otherwise)
    ("head", _HEAD, 8, 0, _HEAD_8),
    ("head", _HEAD, 8, 16, _HEAD_8),
    ("head", _HEAD, 4, 16, [_O(0, [(0, 0), (4, 0), (4, 2), (2, 2), (2, 1), (1, 1), (1, 2), (2, 2), (2, 4), (0, 4)]),
                            _O(1, [(1, 1), (2, 1), (2, 2), (1, 2)]), _O(2, [(2, 2), (4, 2), (4, 4), (2, 4)])]),
    # no arc on the frame: the staircase between 1 and 2 is an open arc (2, 1) .. (7, 6), their other sides arcs shared with the hole
    ("framed-stairs", _FRAMED, 8, 16, [_O(0, [(0, 0), (8, 0), (8, 8), (0, 8)]), _HOLE(0, [(1, 7), (7, 6), (7, 1), (2, 1)]),
                                       _O(1, [(2, 1), (7, 6), (1, 7)]), _O(2, [(2, 1), (7, 1), (7, 6)])]),
]
HAND_IDS = ["%s-c%d-q%d" % (h[0], h[2], h[3]) for h in HAND]


def bar_over_columns(columns, vertical=False):
    """A bar of value 9 over `columns` single-pixel columns of alternating value 1 / 2, three pixels long: the bar's long edge has
    columns - 1 T-junctions inside it.  vertical: the same plane transposed (the bar's long edge runs down)."""
    plane = _p([[9] * columns] + [[1 + x % 2 for x in range(columns)]] * 3)
    return np.ascontiguousarray(plane.T) if vertical else plane


def stairs_with_neighbour(steps, stripe):
    """simplify_oracle.staircase(steps) whose upper region (value 0) is cut into horizontal stripes `stripe` rows high of alternating
    values 0 / 3: every stripe boundary ends in a junction on the staircase."""
    plane = simplify_oracle.staircase(steps).copy()
    for y in range(steps):
        if (y // stripe) % 2:
            plane[y][plane[y] == 0] = 3
    return plane


def wave_plane(width, seed, split=False, framed=False):
    """A thin plane (7 rows) whose region of value 1 hangs from the top down to a seeded square wave -- 1 or 2 rows in even columns, 4 or 5
    in odd ones -- over value 2: a loop of 2 width + 2 corners of which all but four lie on one long arc.  split: the rows from 3 on
    below the wave hold value 3 instead, so that a T-junction lies inside each of the wave's width - 1 vertical edges (3 width + 1
    expanded vertices).  framed: a one-pixel frame of 5 around it all -- the loop then starts at a plain corner, its first junction far
    from position 0."""
    g = np.random.Generator(np.random.PCG64(seed))
    depth = g.integers(1, 3, size=width) + 3 * (np.arange(width) % 2)
    rows = np.arange(7)[:, None]
    plane = np.where(rows < depth[None, :], 1, np.where((rows >= 3) & split, 3, 2)).astype(np.uint8)
    if framed:
        plane = np.pad(plane, 1, constant_values=5)
    return np.ascontiguousarray(plane)


def cpu_planes():
    """The planes of the CPU checks: simplify_oracle's and the hand planes of this file that it does not have."""
    seen, out = set(), simplify_oracle.cpu_planes()
    for name, rows, _, _, _ in HAND:
        if name not in seen and name not in ("stairs", "plus"):
            out.append(("shared-" + name, _p(rows)))
        seen.add(name)
    out += [("bar-5", bar_over_columns(5)), ("bar-5-down", bar_over_columns(5, True)), ("striped-stairs-9", stairs_with_neighbour(9, 2)),
            ("wave-9", wave_plane(9, 3)), ("wave-9-split", wave_plane(9, 4, True)), ("wave-9-framed", wave_plane(9, 5, True, True))]
    return out
