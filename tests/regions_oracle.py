"""Oracle of arseg_rle_regions_fwd (include/arseg_hip.h), written from the contract: a union-find over the runs of one frame in plain Python,
the adjacency of two runs of neighbouring rows stated as the header states it.  Independent of arseg_amd.egress.regions_numpy (which is
tested against it).  Everything is an integer: the tests compare with np.array_equal.  Also the hand-made planes with their regions written
out literally, the seeded noise planes and the planes with a given number of runs and regions that both test files use."""
import numpy as np

import rle_oracle

GUARD_I32 = 0x5A5A5A5A
GUARD_I64 = 0x5A5A5A5A5A5A5A5A


def label(row_start, runs, H, W, connectivity):
    """One frame, complete run code (row_start [H+1], runs [row_start[H]]) -> (R, run_region int32 [runs], records int64 [R,8]:
    value, area, x_min, y_min, x_max, y_max, sum_x, sum_y).  The root of a region is its smallest run index; regions are numbered by
    rising root."""
    assert connectivity in (4, 8)
    d = 1 if connectivity == 8 else 0
    rs = [int(v) for v in row_start]
    n = rs[H]
    x0 = [int(w) >> 8 for w in runs[:n]]
    val = [int(w) & 0xFF for w in runs[:n]]
    x1, row = [0] * n, [0] * n
    for y in range(H):
        for i in range(rs[y], rs[y + 1]):
            x1[i] = x0[i + 1] if i + 1 < rs[y + 1] else W
            row[i] = y
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    X0, X1, V = np.array(x0, dtype=np.int64), np.array(x1, dtype=np.int64), np.array(val, dtype=np.int64)
    for y in range(1, H):
        if rs[y + 1] - rs[y] == 0 or rs[y] - rs[y - 1] == 0:
            continue
        a, b = slice(rs[y], rs[y + 1]), slice(rs[y - 1], rs[y])
        a0, a1, va = X0[a][:, None], X1[a][:, None], V[a][:, None]
        b0, b1, vb = X0[b][None, :], X1[b][None, :], V[b][None, :]
        adjacent = (a0 < b1 + d) & (b0 < a1 + d) & (va == vb)
        for ia, ib in np.argwhere(adjacent):
            ra, rb = find(rs[y] + int(ia)), find(rs[y - 1] + int(ib))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = [find(i) for i in range(n)]
    number = {r: k for k, r in enumerate(sorted(set(root)))}
    R = len(number)
    rec = np.zeros((R, 8), dtype=np.int64)
    rec[:, 2:4] = np.iinfo(np.int64).max
    rec[:, 4:6] = -1
    run_region = np.zeros(n, dtype=np.int32)
    for i in range(n):
        k = number[root[i]]
        run_region[i] = k
        length = x1[i] - x0[i]
        rec[k, 0] = val[root[i]]
        rec[k, 1] += length
        rec[k, 2], rec[k, 3] = min(rec[k, 2], x0[i]), min(rec[k, 3], row[i])
        rec[k, 4], rec[k, 5] = max(rec[k, 4], x1[i] - 1), max(rec[k, 5], row[i])
        rec[k, 6] += (x0[i] + x1[i] - 1) * length // 2
        rec[k, 7] += row[i] * length
    return R, run_region, rec


def expected(row_start, runs, cap, rcap, H, W, connectivity, run_region_before, regions_before):
    """What the buffers of one frame hold after the call: row_start [H+1], runs: the frame's COMPLETE run list, cap / rcap: the capacities,
    run_region_before [cap] / regions_before [rcap,8] (or None): the buffers as they were -> (n_regions, run_region [cap], regions).
    A frame that needs more than cap runs: n_regions = -1 and nothing else is touched.  Otherwise n_regions = R exactly, run_region exact
    below the needed runs and untouched above, the records exact below min(R, rcap) and untouched above."""
    run_region = np.array(run_region_before, dtype=np.int32, copy=True)
    regions = None if regions_before is None else np.array(regions_before, dtype=np.int64, copy=True)
    need = int(row_start[H])
    if need > cap:
        return -1, run_region, regions
    R, rr, rec = label(row_start, runs, H, W, connectivity)
    run_region[:need] = rr
    if regions is not None:
        k = min(R, rcap)
        regions[:k] = rec[:k]
    return R, run_region, regions


def label_planes(planes, connectivity):
    """uint8 [N,H,W] -> [(R, run_region, records)] per frame, through rle_oracle.encode."""
    N, H, W = planes.shape
    row_start, runs = rle_oracle.encode(planes)
    return [label(row_start[n], runs[n], H, W, connectivity) for n in range(N)]


def noise_planes(seed, N, H, W):
    """tests/test_gpu_rle.py's _row_planes, rebuilt: rows of random runs (mean length about 5), every third row constant, every third row
    one of three values per pixel -- many small regions, and diagonal contacts that 4-connectivity does not join."""
    g = np.random.Generator(np.random.PCG64(seed))
    p = np.empty((N, H, W), dtype=np.uint8)
    for n in range(N):
        for y in range(H):
            if (y + n) % 3 == 1:
                p[n, y] = g.integers(0, 256)
            elif (y + n) % 3 == 2:
                p[n, y] = g.integers(0, 3, W) * 127
            else:
                p[n, y] = np.repeat(g.integers(0, 256, W), g.integers(1, 10, W))[:W]
    return p


# the seeded noise planes of the CPU and GPU tests: seed chosen so that in both frames a diagonal contact joins two regions of one value
# (tests/test_regions.py asserts it)
NOISE = (18, 2, 12, 65)


def dense_noise(seed, N, H, W, values=3):
    """Every pixel one of ``values`` values: regions of every shape, many diagonal contacts."""
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(0, values, (N, H, W)) * (255 // (values - 1))).astype(np.uint8)


def stripes(rows, stripes_per_row, extra_rows=0):
    """rows x stripes_per_row vertical stripes two pixels wide with alternating values, then extra_rows constant rows of another value:
    rows * stripes_per_row + extra_rows runs in stripes_per_row + (1 if extra_rows else 0) regions."""
    p = np.empty((1, rows + extra_rows, 2 * stripes_per_row), dtype=np.uint8)
    p[0, :rows] = np.repeat(np.arange(stripes_per_row) % 2 * 200 + 10, 2)
    p[0, rows:] = 99
    return p


def alternating(count, rows=1):
    """``rows`` equal rows of ``count`` single pixels with alternating values: rows * count runs in count regions (either connectivity
    when rows == 1; 4-connectivity otherwise)."""
    return np.tile((np.arange(count) % 2 * 7 + 1).astype(np.uint8), (1, rows, 1))


# planes with exactly 255, 256 and 257 runs (in 17, 16 and 17 regions) and with exactly 255, 256 and 257 regions (in twice as many runs):
# the numbering scan works 256 runs at a time with a carry
RUN_COUNT_PLANES = {255: stripes(15, 17), 256: stripes(16, 16), 257: stripes(16, 16, 1)}
REGION_COUNT_PLANES = {k: alternating(k, 2) for k in (255, 256, 257)}


def _spiral(n, wall, floor):
    """A square spiral of one-pixel walls and one-pixel corridors, n x n, the wall starting at (0, 0) to the right."""
    p = np.full((n, n), floor, dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    p[0, 0] = wall
    inside = lambda a, b: 0 <= a < n and 0 <= b < n
    while True:
        moved = False
        while inside(y + dy, x + dx) and p[y + dy, x + dx] == floor and (not inside(y + 2 * dy, x + 2 * dx) or p[y + 2 * dy, x + 2 * dx] == floor):
            y, x = y + dy, x + dx
            p[y, x] = wall
            moved = True
        if not moved:
            return p
        dy, dx = dx, -dy


def _rings(n, values):
    """n x n, the value of a pixel by its distance from the border."""
    d = np.minimum.reduce([np.arange(n)[:, None] + 0 * np.arange(n), np.arange(n)[None, :] + 0 * np.arange(n)[:, None],
                           n - 1 - np.arange(n)[:, None] + 0 * np.arange(n), n - 1 - np.arange(n)[None, :] + 0 * np.arange(n)[:, None]])
    return np.array(values, dtype=np.uint8)[d]


_COMB = np.array([[5 * (x % 2) for x in range(81)]] * 2 + [[5] * 81], dtype=np.uint8)
_COMB_ROW = [1 if x % 2 else (0 if x == 0 else x // 2 + 1) for x in range(81)]

# Hand-made planes with the answer written out (not computed by this file): name -> (plane, {connectivity: (n_regions, the region number
# of every run in (y, x) order, the records)}).  A record: (value, area, x_min, y_min, x_max, y_max, sum_x, sum_y).
_BOTH = lambda answer: {4: answer, 8: answer}
HAND = {
    "constant": (np.full((3, 5), 7, np.uint8), _BOTH((1, [0, 0, 0], [(7, 15, 0, 0, 4, 2, 30, 15)]))),
    # every pixel a run; alone at 4-connectivity, joined along the diagonals at 8
    "checkerboard-6x6": (np.array([[(x + y) % 2 for x in range(6)] for y in range(6)], np.uint8), {
        4: (36, list(range(36)), [((x + y) % 2, 1, x, y, x, y, x, y) for y in range(6) for x in range(6)]),
        8: (2, [(x + y) % 2 for y in range(6) for x in range(6)], [(0, 18, 0, 0, 5, 5, 45, 45), (1, 18, 0, 0, 5, 5, 45, 45)])}),
    "corner-contact": (np.array([[1, 1, 0, 0], [0, 0, 1, 1]], np.uint8), {
        4: (4, [0, 1, 2, 3], [(1, 2, 0, 0, 1, 0, 1, 0), (0, 2, 2, 0, 3, 0, 5, 0), (0, 2, 0, 1, 1, 1, 1, 2), (1, 2, 2, 1, 3, 1, 5, 2)]),
        8: (2, [0, 1, 1, 0], [(1, 4, 0, 0, 3, 1, 6, 2), (0, 4, 0, 0, 3, 1, 6, 2)])}),
    # the arms meet in the last row: the right arm's root is known only at the end
    "u-shape": (np.array([[1, 0, 1], [1, 0, 1], [1, 1, 1]], np.uint8),
                _BOTH((2, [0, 1, 0, 0, 1, 0, 0], [(1, 7, 0, 0, 2, 2, 7, 8), (0, 2, 1, 0, 1, 1, 2, 1)]))),
    # 40 teeth at the odd columns joined by the bottom row, 41 gaps: 81 runs in a row, 40 unions into one root
    "comb-40-teeth": (_COMB, _BOTH((42, _COMB_ROW + _COMB_ROW + [1],
                                    [(0, 2, 0, 0, 0, 1, 0, 1), (5, 161, 0, 0, 80, 2, 6440, 202)] +
                                    [(0, 2, 2 * m, 0, 2 * m, 1, 4 * m, 1) for m in range(1, 41)]))),
    # one-pixel wall and one-pixel corridor wound 21 x 21: long parent chains.  The wall is 241 pixels and the corridor 200, each centred
    # on the middle (sums = 10 x area, up to the wall's head start of 5); the region of a run is given by its value: wall 0, corridor 1
    "spiral-21x21": (_spiral(21, 3, 0), _BOTH((2, {3: 0, 0: 1}, [(3, 241, 0, 0, 20, 20, 2415, 2415), (0, 200, 0, 1, 19, 19, 1995, 1995)]))),
    # two rings of one value with a ring of another between them: two regions, not one
    "ring-in-ring": (_rings(7, [2, 0, 2, 0]), _BOTH((4, [0,  0, 1, 0,  0, 1, 2, 1, 0,  0, 1, 2, 3, 2, 1, 0,  0, 1, 2, 1, 0,  0, 1, 0,  0],
                                                      [(2, 24, 0, 0, 6, 6, 72, 72), (0, 16, 1, 1, 5, 5, 48, 48), (2, 8, 2, 2, 4, 4, 24, 24),
                                                       (0, 1, 3, 3, 3, 3, 3, 3)]))),
    "one-row": (np.array([[4, 4, 9, 4, 4, 4]], np.uint8),
                _BOTH((3, [0, 1, 2], [(4, 2, 0, 0, 1, 0, 1, 0), (9, 1, 2, 0, 2, 0, 2, 0), (4, 3, 3, 0, 5, 0, 12, 0)]))),
    "one-column": (np.array([[1], [1], [2], [1]], np.uint8),
                   _BOTH((3, [0, 0, 1, 2], [(1, 2, 0, 0, 0, 1, 0, 1), (2, 1, 0, 2, 0, 2, 0, 2), (1, 1, 0, 3, 0, 3, 0, 3)]))),
    # four regions that alternate along every row; the third one (columns 2 and 4) is joined in row 2 only: a top-down pass that numbers
    # provisional labels as it meets them gives the run at (0, 4) a number of its own, the contract gives it the number of the run at (0, 2)
    "interleaved": (np.array([[1, 0, 1, 0, 1], [1, 0, 1, 0, 1], [1, 0, 1, 1, 1], [1, 0, 0, 0, 0]], np.uint8),
                    _BOTH((4, [0, 1, 2, 3, 2,  0, 1, 2, 3, 2,  0, 1, 2,  0, 1],
                           [(1, 4, 0, 0, 0, 3, 0, 6), (0, 7, 1, 0, 4, 3, 13, 15), (1, 7, 2, 0, 4, 2, 21, 8), (0, 2, 3, 0, 3, 1, 6, 1)]))),
}
HAND_IDS = list(HAND)


def hand_plane(name):
    return np.ascontiguousarray(HAND[name][0])[None]
