"""Oracle of the two-list (B-frame) record chain (include/arseg_hip.h, arseg_mv_records_bi_*), written independently of
arseg_amd.ingest.chain_records_numpy: each list is rasterised with mv_records_oracle.rasterize on the records of that list, then every pixel
is walked in plain Python.  Also the hand cases (8x8, gop 4, expected values as literals) and the seeded GOP generator both the CPU and the
GPU tests run."""
import functools

import numpy as np

import mv_records_oracle as base
from mv_records_oracle import rec

POLICIES = ("list0", "near", "mean")
STAT_KEYS = ("both", "only_list1", "neither_under_winner", "intra_gap", "near_tie", "mean_half")


def _lists(records, H, W):
    """Per list: the dense (mvx, mvy, ref) of the winners as nested lists, and which pixels a record of that list covers.  rasterize reads
    (0, 0, -1) where nothing covers, which is also a valid forward record, so coverage comes from a second pass with every ref set to 0."""
    records = np.asarray(records, dtype=np.int16).reshape(-1, 8)
    # a record wholly left of the frame covers nothing; rasterize would hand x + w < 0 to a slice as its end, which counts from the right
    records = records[records[:, 0].astype(np.int64) + records[:, 2] > 0]
    dense, cover = [], []
    for l in (0, 1):
        sel = records[(records[:, 7] & 1) == l]
        mark = sel.copy()
        mark[:, 6] = 0
        dense.append(base.rasterize(sel, H, W).tolist())
        cover.append((base.rasterize(mark, H, W)[..., 2] == 0).tolist())
    return dense, cover


def _mean(a, b):
    return round((a + b) / 2)                      # Python's round: half to even; (a + b) / 2 is exact


def chain(pushes, H, W, gop, max_ref=3, policy="list0", stats=None):
    """pushes: [(f, int16 [n,8])] in decode order -> merged int16 [gop,H,W,2] (frame 0 = -1, frames never pushed = 0).  stats: a dict that
    receives pixel counts per STAT_KEYS, summed over the frames."""
    assert policy in POLICIES and 2 <= gop <= 64
    merged = np.zeros((gop, H, W, 2), dtype=np.int16)
    merged[0] = -1
    D = {0}
    m = {}                                          # frames chained so far as nested lists (a frame never changes once written)
    count = dict.fromkeys(STAT_KEYS, 0)

    def link(x, y, mvx, mvy, t):
        k2 = min(max(x + round(mvx / 4), 0), W - 1)                    # Python's round: half to even; mvx / 4 is exact
        j2 = min(max(y + round(mvy / 4), 0), H - 1)
        if t > 0:
            a, b = m[t][j2][k2]
            return 4 * (k2 - x) + a, 4 * (j2 - y) + b
        return 4 * (k2 - x), 4 * (j2 - y)

    for f, records in pushes:
        assert 1 <= f < gop and f not in D
        dense, cover = _lists(records, H, W)
        target = {}                                 # reference code -> its target, for the codes that are in range and whose target is in D
        for ref in range(-max_ref, max_ref):
            t = max(0, f - ref - 1) if ref >= 0 else f - ref
            if t in D:
                target[ref] = t
        p = max(g for g in D if g < f)
        out = []
        for y in range(H):
            c0, c1, d0, d1 = cover[0][y], cover[1][y], dense[0][y], dense[1][y]
            row = []
            for x in range(W):
                l0 = l1 = t0 = t1 = None
                if c0[x]:
                    mvx, mvy, ref = d0[x]
                    t0 = target.get(ref)
                    if t0 is not None:
                        l0 = link(x, y, mvx, mvy, t0)
                if c1[x]:
                    mvx, mvy, ref = d1[x]
                    t1 = target.get(ref)
                    if t1 is not None:
                        l1 = link(x, y, mvx, mvy, t1)
                if l0 is not None and l1 is not None:
                    count["both"] += 1
                    count["near_tie"] += abs(t0 - f) == abs(t1 - f)
                    count["mean_half"] += (l0[0] + l1[0]) % 2 == 1 or (l0[1] + l1[1]) % 2 == 1
                    if policy == "list0":
                        v = l0
                    elif policy == "near":
                        v = l1 if abs(t1 - f) < abs(t0 - f) else l0
                    else:
                        v = (_mean(l0[0], l1[0]), _mean(l0[1], l1[1]))
                elif l0 is not None:
                    v = l0
                elif l1 is not None:
                    count["only_list1"] += 1
                    v = l1
                else:
                    count["neither_under_winner"] += c0[x] or c1[x]
                    count["intra_gap"] += p != f - 1
                    v = m[p][y][x] if p > 0 else (0, 0)
                assert -32768 <= v[0] <= 32767 and -32768 <= v[1] <= 32767
                row.append(v)
            out.append(row)
        merged[f] = np.array(out, dtype=np.int16).reshape(H, W, 2)
        m[f] = merged[f].tolist()
        D.add(f)
    if stats is not None:
        stats.update(count)
    return merged


# ---- hand cases: 8x8, gop 4 ----
def _a(rows):
    return np.array(rows, dtype=np.int16).reshape(-1, 8)


def _rows(fn):
    return [[fn(y, x) for x in range(8)] for y in range(8)]


def _patch(frame, y0, y1, x0, x1, v):
    return [[v if y0 <= y < y1 and x0 <= x < x1 else frame[y][x] for x in range(8)] for y in range(8)]


Z = _rows(lambda y, x: (0, 0))
BASE = rec(0, 0, 8, 8, 4, 0, 0)                                       # the whole frame one pixel to the right in the previous frame
M1 = _rows(lambda y, x: (4, 0) if x < 7 else (0, 0))                 # BASE at f = 1: column 7 clamps onto itself
M2 = _rows(lambda y, x: ((8, 0) if x <= 5 else (4, 0) if x == 6 else (0, 0)))          # BASE at f = 2 over M1
# rec(0, 0, 8, 8, 0, 8, 1) at f = 3 (two rows down, into frame 1) over M1: rows 6 and 7 clamp
M3 = _rows(lambda y, x: (4 if x < 7 else 0, 8 if y <= 5 else 4 if y == 6 else 0))


def hand_cases():
    """[(name, max_ref, pushes, {policy: {f: frame literal [8][8] of (dx, dy)}})].  Every frame pushed is listed."""
    def same(frames):
        return {pol: frames for pol in POLICIES}

    bi = [rec(2, 2, 4, 4, 4, 0, 0, 0), rec(2, 2, 4, 4, -4, 4, -1, 1)]                 # list 0 back to frame 1, list 1 forward to frame 3
    bi_swapped = [rec(2, 2, 4, 4, 4, 0, 0, 0x7ff1), rec(2, 2, 4, 4, -4, 4, -1, -2)]  # the same two with the lists exchanged, other reserved bits set
    back = _patch(M1, 2, 6, 2, 6, (8, 0))                                            # (4, 0) + M1[y][x + 1]
    fwd = _patch(_patch(M1, 2, 5, 2, 6, (0, 12)), 5, 6, 2, 6, (0, 8))                 # (-4, 4) + M3[y + 1][x - 1]
    mean = _patch(_patch(M1, 2, 5, 2, 6, (4, 6)), 5, 6, 2, 6, (4, 4))
    order_132 = lambda b: [(1, _a([BASE])), (3, _a([rec(0, 0, 8, 8, 0, 8, 1)])), (2, _a(b))]
    low_delay = [rec(2, 2, 4, 4, 0, 0, 1, 0), rec(2, 2, 4, 4, 0, -4, 0, 1)]           # list 0 two frames back, list 1 one frame back
    lr = lambda f, l, r: _patch(_patch(f, 2, 6, 0, 4, l), 2, 6, 4, 8, r)
    odd = [(1, _a([rec(0, 2, 4, 4, 4, -4, 0, 0), rec(0, 2, 4, 4, 0, 0, 0, 1), rec(4, 2, 4, 4, -4, 4, 0, 0), rec(4, 2, 4, 4, 0, 0, 0, 1)])),
           (2, _a([rec(0, 2, 4, 4, 0, 0, 0, 0), rec(0, 2, 4, 4, 0, 0, 1, 1), rec(4, 2, 4, 4, 0, 0, 0, 0), rec(4, 2, 4, 4, 0, 0, 1, 1)])),
           (3, _a([rec(0, 2, 4, 4, 0, 0, 0, 0), rec(0, 2, 4, 4, 0, 0, 1, 1), rec(4, 2, 4, 4, 0, 0, 0, 0), rec(4, 2, 4, 4, -4, 4, 2, 1)]))]
    first = lr(Z, (4, -4), (-4, 4))
    return [
        ("bi block, list 0 back, list 1 forward, NEAR tie", 3, order_132(bi),
         {"list0": {1: M1, 3: M3, 2: back}, "near": {1: M1, 3: M3, 2: back}, "mean": {1: M1, 3: M3, 2: mean}}),
        ("bi block, list 0 forward, list 1 back", 3, order_132(bi_swapped),
         {"list0": {1: M1, 3: M3, 2: fwd}, "near": {1: M1, 3: M3, 2: fwd}, "mean": {1: M1, 3: M3, 2: mean}}),
        ("two past references, NEAR takes list 1", 3, [(1, _a([BASE])), (2, _a([BASE])), (3, _a(low_delay))],
         {"list0": {1: M1, 2: M2, 3: _patch(M2, 2, 6, 2, 6, (4, 0))}, "near": {1: M1, 2: M2, 3: _patch(M2, 2, 6, 2, 6, (8, -4))},
          "mean": {1: M1, 2: M2, 3: _patch(M2, 2, 6, 2, 6, (6, -2))}}),
        # MEAN: (4, -4) & 0 -> (2, -2); (2, -2) & 0 -> (1, -1); then (1, -1) + (2, -2) = (3, -3) -> (2, -2): halves away from zero, to even;
        # on the right (-1, 1) + (-4, 4) = (-5, 5) -> (-2, 2): halves towards zero, to even
        ("MEAN with odd sums in both signs", 3, odd,
         {"list0": {1: first, 2: first, 3: first}, "near": {1: first, 2: first, 3: first},
          "mean": {1: lr(Z, (2, -2), (-2, 2)), 2: lr(Z, (1, -1), (-1, 1)), 3: lr(Z, (2, -2), (-2, 2))}}),
        ("unusable winner over a usable lower index reads intra", 3,
         [(1, _a([BASE])), (2, _a([rec(2, 2, 4, 4, 4, 0, 0, 0), rec(2, 2, 2, 4, 4, 0, 5, 0), rec(2, 2, 4, 1, 4, 0, -4, 0)]))],
         same({1: M1, 2: _patch(M1, 3, 6, 4, 6, (8, 0))})),
        ("target not yet done", 3,
         [(1, _a([BASE])), (2, _a([rec(2, 2, 4, 2, 0, 0, -1, 0), rec(2, 2, 4, 2, 4, 0, 0, 1), rec(2, 4, 4, 2, 0, 0, -1, 0)]))],
         same({1: M1, 2: _patch(M1, 2, 4, 2, 6, (8, 0))})),
        ("forward target >= gop", 3,
         [(1, _a([BASE])), (3, _a([rec(2, 2, 4, 2, 0, 0, -1, 0), rec(2, 2, 4, 2, 4, 0, 1, 1), rec(2, 4, 4, 2, 0, 0, -3, 1)]))],
         same({1: M1, 3: _patch(M1, 2, 4, 2, 6, (8, 0))})),
        ("intra with a gap in D", 3, [(1, _a([BASE])), (3, _a([rec(2, 2, 4, 4, 0, 4, 1, 0)])), (2, _a([]))],
         same({1: M1, 3: _patch(M1, 2, 6, 2, 6, (4, 4)), 2: M1})),
        ("past clamp max(0, .)", 3, [(1, _a([rec(2, 2, 4, 4, 8, 0, 2, 0)])), (2, _a([rec(2, 2, 4, 4, -4, 0, 2, 1)]))],
         same({1: _patch(Z, 2, 6, 2, 6, (8, 0)), 2: _patch(Z, 2, 6, 2, 6, (-4, 0))})),
    ]


def hand_expected(frames):
    """{f: literal} -> int16 [4,8,8,2] with frame 0 = -1 and frames not pushed = 0."""
    want = np.zeros((4, 8, 8, 2), dtype=np.int16)
    want[0] = -1
    for f, lit in frames.items():
        want[f] = np.array(lit, dtype=np.int16)
    return want


# ---- generated GOPs ----
GOP = 8
ORDERS = ((1, 2, 3, 4, 5, 6, 7), (3, 1, 2, 6, 4, 5, 7), (4, 2, 1, 3, 6, 5, 7), (7, 3, 1, 2, 5, 4, 6))
SEED = 1                            # chosen on the CPU: with it every rule below is met by the oracle alone (test_mv_brecords.py)


def _pick_ref(rng, f, D, gop, max_ref):
    """A reference code: mostly one whose target is done, some whose target is not (or lies past the GOP), some out of range."""
    codes = list(range(-max_ref, max_ref))
    target = lambda r: max(0, f - r - 1) if r >= 0 else f - r
    done = [r for r in codes if target(r) in D]
    undone = [r for r in codes if target(r) not in D]
    u = rng.random()
    if u < 0.08:
        return int(rng.choice([max_ref, max_ref + 2, -max_ref - 1, 90, -90]))
    if (u < 0.2 and undone) or not done:            # e.g. frame 7 decoded first with max_ref 3: nothing it can name is done
        return int(rng.choice(undone))
    return int(rng.choice(done))


def make_gop(seed, H, W, order, max_ref, gop=GOP):
    """[(f, int16 [n,8])] in the decode order `order`: 8x8 blocks each with no record, list 0 only, list 1 only or both; a few rectangles
    that overlap them (first and last in the list), off-frame records, zero padding, random upper bits in `reserved`."""
    rng = np.random.default_rng([seed, H, W, max_ref] + list(order))
    D, pushes = {0}, []
    for f in order:
        rows = []

        def one(x, y, w, h, l):
            hi = int(rng.integers(-8192, 8192)) * 2                  # bits 1..15 of reserved: ignored
            rows.append(rec(x, y, w, h, int(rng.integers(-24, 25)), int(rng.integers(-24, 25)), _pick_ref(rng, f, D, gop, max_ref), hi | l))

        for _ in range(2):                                            # overlapped by the blocks below wherever those have a record
            one(int(rng.integers(-4, W)), int(rng.integers(-4, H)), int(rng.integers(1, 20)), int(rng.integers(1, 20)), int(rng.integers(0, 2)))
        for by in range(0, H, 8):
            for bx in range(0, W, 8):
                kind = int(rng.choice(4, p=[0.1, 0.15, 0.15, 0.6]))
                if kind in (1, 3):
                    one(bx, by, 8, 8, 0)
                if kind in (2, 3):
                    one(bx, by, 8, 8, 1)
                if rng.random() < 0.1:
                    rows.append([0] * 8)                              # padding between records
        for _ in range(3):                                            # these win over the blocks
            one(int(rng.integers(-4, W)), int(rng.integers(-4, H)), int(rng.integers(1, 12)), int(rng.integers(1, 12)), int(rng.integers(0, 2)))
        one(W, 3, 8, 8, 0)
        one(-9, -9, 9, 9, 1)                                          # wholly off the frame
        rows += [[0] * 8] * 3
        pushes.append((f, _a(rows)))
        D.add(f)
    return pushes


BANDED = (300, 200)                 # taller than the scatter's 256-row band


def banded_gop(order, max_ref, gop=GOP):
    """make_gop at BANDED with a frame-sized record in each list put first (the scatter cuts such a record into bands of 256 rows): every
    pixel has a winner in both lists."""
    H, W = BANDED
    out = []
    for i, (f, r) in enumerate(make_gop(SEED, H, W, order, max_ref, gop)):
        big = _a([rec(-3, -3, W + 9, H + 9, 6 + i, -10, 0, 0), rec(0, 0, W, H, -7, 5 + i, -1 if i % 2 else 1, 1)])
        out.append((f, np.concatenate([big, r])))
    return out


@functools.lru_cache(maxsize=None)
def generated(H, W, order, max_ref, policy):
    """(pushes, merged, stats) of the generated GOP; computed once per process and shared (treat as read-only)."""
    pushes = banded_gop(order, max_ref) if (H, W) == BANDED else make_gop(SEED, H, W, order, max_ref)
    stats = {}
    merged = chain(pushes, H, W, GOP, max_ref, policy, stats)
    merged.setflags(write=False)
    return pushes, merged, stats
