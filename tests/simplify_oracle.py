"""Oracle of arseg_contours_simplify_fwd (include/arseg_hip.h), written from the contract as the plain recursion on lists of Python-int
points: the farthest vertex from the first, Douglas-Peucker on the two chains, the fewer-than-3 rule.  No flags, no walk, nothing shared
with arseg_amd.egress.simplify_numpy (which is tested against it).  Also the refusal and capacity rules (``expected``), the hand-made
planes with the kept vertices written out literally at named tolerances, and the inputs both test files use."""
import numpy as np

import contours_oracle
import links_oracle
import regions_oracle
import rle_oracle

GUARD_I32 = contours_oracle.GUARD_I32
GUARD_WORD = contours_oracle.GUARD_WORD

# the tolerances of the tests as tol2_q = 16 x the squared tolerance: 0, 0.5, 1, 1.5 and 2 px, and one far beyond every shape
TOLERANCES = {0.0: 0, 0.5: 4, 1.0: 16, 1.5: 36, 2.0: 64, 256.0: 1 << 20}
TOL2_QS = list(TOLERANCES.values())


def _cross(p, a, b):
    return abs((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]))


def _chain(P, a, b, tol2_q):
    """The interior positions of the chain segment (a, b) that are kept, in order."""
    best, at = -1, None
    for i in range(a + 1, b):
        c = _cross(P[i], P[a], P[b])
        if c > best:                                              # strictly: the smallest position of a tie
            best, at = c, i
    if at is None or 16 * best * best <= tol2_q * ((P[b][0] - P[a][0]) ** 2 + (P[b][1] - P[a][1]) ** 2):
        return []
    return _chain(P, a, at, tol2_q) + [at] + _chain(P, at, b, tol2_q)


def kept_positions(points, tol2_q):
    """One loop [(x, y), ...] -> the positions of the vertices that stay, rising."""
    n = len(points)
    P = list(points) + [points[0]]
    far = [(x - P[0][0]) ** 2 + (y - P[0][1]) ** 2 for x, y in points]
    a1 = far.index(max(far))                                      # the smallest position of a tie
    kept = [0] + _chain(P, 0, a1, tol2_q) + ([a1] if a1 > 0 else []) + _chain(P, a1, n, tol2_q)
    return kept if len(kept) >= 3 else list(range(n))


def simplify_loops(loops, tol2_q):
    """contours_oracle.trace_plane's loops [(region, hole, [(x, y)])] -> the same with the kept vertices."""
    return [(r, hole, [pts[i] for i in kept_positions([(int(x), int(y)) for x, y in pts], tol2_q)]) for r, hole, pts in loops]


def loops_of(answer):
    """(counts, loops, verts) of one frame -> [(region, hole, [(x, y)])] of Python ints."""
    return [(r, hole, [(int(x), int(y)) for x, y in pts]) for r, hole, pts in contours_oracle.polygons(answer)]


def simplify_frame(answer, tol2_q):
    """(counts, loops, verts) of one frame as arseg_rle_contours_fwd leaves them -> the same three arrays after the pass."""
    return contours_oracle.arrays(simplify_loops(loops_of(answer), tol2_q))


def expected(answer, processable, vcap_out, counts_before, loops_before, verts_before):
    """What the output buffers of one frame hold after the call.  answer: simplify_frame's; processable: the source frame was neither
    refused nor overflowed; the three buffers as they were -> (counts [2], loops [lcap,4], verts [vcap_out]).  Not processable: counts =
    {-1, -1} and nothing else is touched; otherwise counts and the rows below L exact, the words below min(V', vcap_out) exact, the rest
    untouched."""
    counts = np.array(counts_before, dtype=np.int32, copy=True)
    loops = np.array(loops_before, dtype=np.int32, copy=True).reshape(-1, 4)
    verts = np.array(verts_before, dtype=np.uint32, copy=True)
    if not processable:
        counts[:] = -1
        return counts, loops, verts
    counts[:] = answer[0]
    v = min(len(answer[2]), vcap_out)
    loops[:len(answer[1])] = answer[1]
    verts[:v] = answer[2][:v]
    return counts, loops, verts


def _p(rows):
    return np.array(rows, dtype=np.uint8)


_STAIRS = [[1 if x <= y else 0 for x in range(6)] for y in range(6)]
_PLUS = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
_NOTCHED = [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]]
_FRAME = [[3] * 6, [3, 0, 0, 0, 0, 3], [3, 0, 0, 0, 0, 3], [3] * 6]

_O = lambda r, pts: (r, 0, pts)
_HOLE = lambda r, pts: (r, 1, pts)
_BIG = 1 << 20


def _BY(groups):
    """{(tol2_q, ...): loops} -> {tol2_q: loops}"""
    return {q: loops for qs, loops in groups.items() for q in qs}


_EVERY = (0, 4, 16, 36, 64, _BIG)
_STAIRS_0 = [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (0, 6)]
_STAIRS_1 = [(1, 0), (6, 0), (6, 5), (5, 5), (5, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)]
_CUP_OUT = _O(0, [(0, 0), (5, 0), (5, 4), (0, 4)])
_PLUS_CORNERS = lambda middle: [_O(0, [(0, 0), (1, 0), (1, 1), (0, 1)]), _O(1, middle), _O(2, [(2, 0), (3, 0), (3, 1), (2, 1)]),
                                _O(3, [(0, 2), (1, 2), (1, 3), (0, 3)]), _O(4, [(2, 2), (3, 2), (3, 3), (2, 3)])]
_NOTCH_IN = _O(1, [(1, 1), (2, 1), (2, 2), (1, 2)])
_NOTCHED_IN = _O(1, [(3, 3), (4, 3), (4, 4), (3, 4)])

# Hand-made planes with the kept vertices written out (not computed by this file): name -> (plane rows, {tol2_q: [(region, hole, [(x, y)])]}).
# The loops are the same at both connectivities (tests/test_simplify.py asserts it).  For the reader: the corner of a unit stair step
# lies 1 / sqrt(2) = 0.71 px off the line through its neighbours; at the far tolerance everything is dropped and rule 3 gives the loop back.
HAND = {
    # rule 3: either chain of the square drops its corner at 1 px (0.71 px off the diagonal), two vertices are left, so all four stay
    "unit-square": ([[7]], _BY({_EVERY: [_O(0, [(0, 0), (1, 0), (1, 1), (0, 1)])]})),
    # the corners lie 8 / sqrt(20) = 1.79 px off the diagonal: kept below that, and beyond it rule 3 keeps them
    "rectangle-4x2": ([[2] * 4] * 2, _BY({_EVERY: [_O(0, [(0, 0), (4, 0), (4, 2), (0, 2)])]})),
    # the staircase triangle: at 0.5 px only the last step goes (1 / sqrt(5) = 0.45 px off the chord (5, 4) - (6, 6)), at 1 px all steps
    "stairs": (_STAIRS, _BY({
        (0, _BIG): [_O(0, _STAIRS_0), _O(1, _STAIRS_1)],
        (4,): [_O(0, _STAIRS_0[:10] + [(6, 6), (0, 6)]), _O(1, _STAIRS_1[:10])],
        (16, 36, 64): [_O(0, [(0, 0), (6, 6), (0, 6)]), _O(1, [(1, 0), (6, 0), (6, 5)])],
    })),
    "l-shape": (contours_oracle._L, _BY({
        (0, 4, _BIG): [_O(0, [(0, 0), (1, 0), (1, 2), (3, 2), (3, 3), (0, 3)]), _O(1, [(1, 0), (3, 0), (3, 2), (1, 2)])],
        (16, 36, 64): [_O(0, [(0, 0), (3, 3), (0, 3)]), _O(1, [(1, 0), (3, 0), (3, 2), (1, 2)])],
    })),
    # the hole runs counter-clockwise and the loop of the region inside it clockwise: the same vertices stay at 1 px.  At 0.5 px the
    # two prong corners of a chain tie (c = 3 against the chord along the rim) and the smaller position is kept, the other dropped
    "cup-hole": (contours_oracle._CUP, _BY({
        (0, 64, _BIG): [_CUP_OUT, _HOLE(0, [(1, 1), (1, 3), (4, 3), (4, 1), (3, 1), (3, 2), (2, 2), (2, 1)]),
                        _O(1, [(1, 1), (2, 1), (2, 2), (3, 2), (3, 1), (4, 1), (4, 3), (1, 3)])],
        (4,): [_CUP_OUT, _HOLE(0, [(1, 1), (1, 3), (4, 3), (4, 1), (3, 1), (3, 2)]), _O(1, [(1, 1), (2, 1), (2, 2), (4, 1), (4, 3), (1, 3)])],
        (16, 36): [_CUP_OUT, _HOLE(0, [(1, 1), (1, 3), (4, 3), (4, 1)]), _O(1, [(1, 1), (4, 1), (4, 3), (1, 3)])],
    })),
    "two-holes": (contours_oracle._TWO_HOLES, _BY({
        _EVERY: [_O(0, [(0, 0), (7, 0), (7, 4), (0, 4)]), _HOLE(0, [(1, 1), (1, 3), (2, 3), (2, 1)]), _O(1, [(1, 1), (2, 1), (2, 3), (1, 3)]),
                 _HOLE(0, [(4, 1), (4, 3), (6, 3), (6, 1)]), _O(2, [(4, 1), (6, 1), (6, 3), (4, 3)])],
    })),
    # the plus: c ties on its chords ((2, 0) and (2, 1) against (1, 0) - (3, 1), both 1); from 0.5 px on its four tips' leading corners stay
    "plus": (_PLUS, _BY({
        (0, 64, _BIG): _PLUS_CORNERS([(1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (2, 2), (2, 3), (1, 3), (1, 2), (0, 2), (0, 1), (1, 1)]),
        (4, 16, 36): _PLUS_CORNERS([(1, 0), (3, 1), (2, 3), (0, 2)]),
    })),
    # a tie of c that decides the result: (2, 1) and (1, 1) lie 1 px off the chord (3, 2) - (0, 2); at 0.5 px the smaller position, (2, 1),
    # is kept, and with it (2, 2), while (1, 1) and (1, 2) then lie within 0.45 px of (2, 1) - (0, 2)
    "notch-tie": ([[0, 0, 0], [0, 1, 0]], _BY({
        (0, 64, _BIG): [_O(0, [(0, 0), (3, 0), (3, 2), (2, 2), (2, 1), (1, 1), (1, 2), (0, 2)]), _NOTCH_IN],
        (4,): [_O(0, [(0, 0), (3, 0), (3, 2), (2, 2), (2, 1), (0, 2)]), _NOTCH_IN],
        (16, 36): [_O(0, [(0, 0), (3, 0), (3, 2), (0, 2)]), _NOTCH_IN],
    })),
    # the farthest vertex from (0, 0) ties: (4, 3) and (3, 4) are both at 5; the smaller position, (4, 3), is the anchor and stays
    "notched-square": (_NOTCHED, _BY({
        (0, 4, _BIG): [_O(0, [(0, 0), (4, 0), (4, 3), (3, 3), (3, 4), (0, 4)]), _NOTCHED_IN],
        (16, 36, 64): [_O(0, [(0, 0), (4, 0), (4, 3), (0, 4)]), _NOTCHED_IN],
    })),
    "frame-hole": (_FRAME, _BY({
        _EVERY: [_O(0, [(0, 0), (6, 0), (6, 4), (0, 4)]), _HOLE(0, [(1, 1), (1, 3), (5, 3), (5, 1)]), _O(1, [(1, 1), (5, 1), (5, 3), (1, 3)])],
    })),
}
HAND_IDS = list(HAND)


def hand_plane(name):
    return _p(HAND[name][0])


def staircase(steps):
    """A plane whose region 1 is a staircase of `steps` steps: its outer loop has 2 steps + 2 vertices (pixels with x <= y)."""
    return _p([[1 if x <= y else 0 for x in range(steps)] for y in range(steps)])


def stair_loop(vertices, seed, x=0, y=0):
    """An uneven staircase from (x, y) down to the right with seeded steps of 1 to 3, closed along its bottom and left side: a loop of
    `vertices` corners (even, >= 4) in the contract's form -- axes alternate, it starts at its smallest vertex, clockwise on the screen."""
    assert vertices >= 4 and vertices % 2 == 0
    g = np.random.Generator(np.random.PCG64(seed))
    steps = g.integers(1, 4, size=vertices - 2).tolist()
    pts = [(x, y)]
    for k, d in enumerate(steps):
        px, py = pts[-1]
        pts.append((px + d, py) if k % 2 == 0 else (px, py + d))
    return pts + [(x, pts[-1][1])]


def stair_frame(vertices, seed):
    """One frame of three loops as arseg_rle_contours_fwd would leave them -- a rectangle, an uneven staircase of `vertices` corners and
    a short staircase behind it -- written down as vertices: ((counts, loops, verts), the side of a square frame that holds them)."""
    long = stair_loop(vertices, seed, 0, 2)
    far = max(max(p) for p in long)
    loops = [(0, 0, [(0, 0), (far, 0), (far, 2), (0, 2)]), (1, 0, long), (2, 0, stair_loop(8, seed + 1, far + 1, 2))]
    side = max(max(p) for _, _, pts in loops for p in pts) + 1
    assert side <= 16384
    return contours_oracle.arrays(loops), side


def cpu_planes():
    """The planes of the CPU checks: (name, uint8 [H,W])."""
    out = [(name, hand_plane(name)) for name in HAND_IDS] + [(name, np.ascontiguousarray(p)) for name, p in contours_oracle.LONG.items()]
    for case in rle_oracle.CASES:
        out += [("%s-%d" % (case[0], n), p) for n, p in enumerate(rle_oracle.build(case))]
    out += [("noise-%d" % n, p) for n, p in enumerate(regions_oracle.noise_planes(*regions_oracle.NOISE))]
    out += [("dense-%d" % n, p) for n, p in enumerate(regions_oracle.dense_noise(*links_oracle.DENSE))]
    return out
