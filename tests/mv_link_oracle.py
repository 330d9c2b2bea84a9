"""Oracle of the link bytes along the motion chain (include/arseg_hip.h, arseg_mv_link_reset / arseg_mv_records_step_link_fwd /
arseg_mv_records_bi_step_link_fwd), restated from the contract and independently of arseg_amd.ingest.chain_records_numpy: each list is
rasterised with mv_records_oracle.rasterize, then every pixel is walked in plain Python.  A link byte depends on where the links lead, never
on the accumulated vectors, so the oracle does not compute `merged` at all.  Also: the statistics row of a link plane, the hand cases (8x8,
expected bytes as literals), the seeded GOP generator the CPU and the GPU tests run, and a numpy oracle of the linked consistency form
(arseg_labels_consistency_linked_fwd)."""
import functools

import numpy as np

import mv_records_oracle as base
from mv_records_oracle import rec

INTRA, UNCOVERED, CLAMPED = 1, 2, 4
NSTATS = 4 + 16
POLICIES = ("list0", "near", "mean")


def _a(rows):
    return np.array(rows, dtype=np.int16).reshape(-1, 8)


def _visible(records):
    """A record wholly left of the frame covers nothing; rasterize would hand x + w < 0 to a slice as its end, which counts from the right."""
    records = np.asarray(records, dtype=np.int16).reshape(-1, 8)
    return records[records[:, 0].astype(np.int64) + records[:, 2] > 0]


def _field(records, H, W):
    """Records of one map -> (dense (mvx, mvy, ref) as nested lists, covered as nested lists).  rasterize reads (0, 0, -1) where nothing
    covers, which is also a record a decoder may send, so coverage comes from a second pass with every ref set to 0."""
    mark = records.copy()
    mark[:, 6] = 0
    return base.rasterize(records, H, W).tolist(), (base.rasterize(mark, H, W)[..., 2] == 0).tolist()


def _byte(own, gathered):
    return ((own | gathered) & 7) | (min(15, 1 + (gathered >> 4)) << 4)


def _hop(x, y, mvx, mvy, H, W):
    """The rounded target, clamped, and whether the clamp moved it."""
    tx, ty = x + round(mvx / 4), y + round(mvy / 4)                    # Python's round: half to even; mvx / 4 is exact
    k2, j2 = min(max(tx, 0), W - 1), min(max(ty, 0), H - 1)
    return k2, j2, CLAMPED if (k2, j2) != (tx, ty) else 0


def chain_p(frames, H, W, gop, max_ref=3):
    """The P entry: frames = [int16 [n,8]] for f = 1, 2, ... -> link uint8 [gop,H,W] (frame 0 and frames never pushed = 0)."""
    link = np.zeros((gop, H, W), dtype=np.uint8)
    done = {}
    for f, records in enumerate(frames, start=1):
        assert f < gop
        dense, cover = _field(_visible(records), H, W)
        out = []
        for y in range(H):
            row = []
            for x in range(W):
                mvx, mvy, ref = dense[y][x]
                own = 0
                if not cover[y][x]:
                    own, mvx, mvy, ref = UNCOVERED, 0, 0, 0
                elif ref < 0 or ref >= max_ref:
                    own, mvx, mvy, ref = INTRA, 0, 0, 0
                k2, j2, clamped = _hop(x, y, mvx, mvy, H, W)
                t = max(0, f - ref - 1)
                row.append(_byte(own | clamped, done[t][j2][k2] if t > 0 else 0))
            out.append(row)
        done[f] = out
        link[f] = np.array(out, dtype=np.uint8)
    return link


def chain(pushes, H, W, gop, max_ref=3, policy="list0", own=None):
    """The bi entry: pushes = [(f, int16 [n,8])] in decode order -> link uint8 [gop,H,W] (frame 0 and frames never pushed = 0).  own: a dict
    that receives per frame the flags each pixel set at its own hop (uint8 [H,W]); what a byte carries beyond them is inherited."""
    assert policy in POLICIES and 2 <= gop <= 64
    link = np.zeros((gop, H, W), dtype=np.uint8)
    done = {}                                                          # frames chained so far, as nested lists; 0 is in D with all zero
    for f, records in pushes:
        assert 1 <= f < gop and f not in done
        records = _visible(records)
        lists = [_field(records[(records[:, 7] & 1) == l], H, W) for l in (0, 1)]
        target = {}                                                    # reference code -> its target, where in range and in D
        for ref in range(-max_ref, max_ref):
            t = max(0, f - ref - 1) if ref >= 0 else f - ref
            if t == 0 or t in done:
                target[ref] = t
        p = max(g for g in [0] + list(done) if g < f)
        out, mine = [], []
        for y in range(H):
            row = []
            for x in range(W):
                cand, won = [], False
                for dense, cover in lists:
                    if not cover[y][x]:
                        cand.append(None)
                        continue
                    won = True
                    mvx, mvy, ref = dense[y][x]
                    t = target.get(ref)
                    if t is None:
                        cand.append(None)
                        continue
                    k2, j2, clamped = _hop(x, y, mvx, mvy, H, W)
                    cand.append((t, _byte(clamped, done[t][j2][k2] if t > 0 else 0), clamped))
                c0, c1 = cand
                if c0 is None and c1 is None:
                    first = INTRA if won else UNCOVERED
                    v = _byte(first, done[p][y][x] if p > 0 else 0)
                elif c1 is None:
                    v, first = c0[1], c0[2]
                elif c0 is None:
                    v, first = c1[1], c1[2]
                elif policy == "list0":
                    v, first = c0[1], c0[2]
                elif policy == "near":
                    v, first = (c1[1], c1[2]) if abs(c1[0] - f) < abs(c0[0] - f) else (c0[1], c0[2])
                else:
                    v, first = ((c0[1] | c1[1]) & 7) | (max(c0[1] >> 4, c1[1] >> 4) << 4), c0[2] | c1[2]
                row.append(v)
                mine.append(first)
            out.append(row)
        if own is not None:
            own[f] = np.array(mine, dtype=np.uint8).reshape(H, W)
        done[f] = out
        link[f] = np.array(out, dtype=np.uint8)
    return link


def stats_row(plane):
    """One link plane -> its row of link_stats: pixels with INTRA, UNCOVERED, CLAMPED, any flag, then the 16 hop bins."""
    row = [0] * NSTATS
    for v in np.asarray(plane).reshape(-1).tolist():
        row[0] += v & 1
        row[1] += (v >> 1) & 1
        row[2] += (v >> 2) & 1
        row[3] += (v & 7) != 0
        row[4 + (v >> 4)] += 1
    return row


def stats(link):
    return np.array([stats_row(p) for p in link], dtype=np.int64)


# ---- hand cases: 8x8 ----
def _rows(fn):
    return [[fn(y, x) for x in range(8)] for y in range(8)]


def _patch(frame, y0, y1, x0, x1, v):
    return [[v if y0 <= y < y1 and x0 <= x < x1 else frame[y][x] for x in range(8)] for y in range(8)]


def _flat(v):
    return _rows(lambda y, x: v)


STILL = rec(0, 0, 8, 8, 0, 0, 0)                                      # the whole frame onto the same pixels of the previous frame


def hand_cases():
    """[(name, max_ref, gop, pushes, {policy: {f: literal [8][8] of link bytes}})].  Every frame pushed is listed.  A byte reads
    0x<hops><flags>: flags 1 intra, 2 uncovered, 4 clamped."""
    def same(frames):
        return {pol: frames for pol in POLICIES}

    in_order = lambda frames: [(f, _a(r)) for f, r in enumerate(frames, start=1)]
    cases = []
    # the block of frame 1 has no usable prediction; frames 2, 3, 4 link each pixel to itself one frame back
    cases.append(("an intra block whose flag survives three further hops", 3, 5,
                  in_order([[STILL, rec(2, 2, 4, 4, 8, 8, 5)], [STILL], [STILL], [STILL]]),
                  same({f: _patch(_flat(f << 4), 2, 6, 2, 6, (f << 4) | 1) for f in (1, 2, 3, 4)})))
    # rows 3 and 4 of frame 1 have no record.  Frame 2 points one row down: rows 2 and 3 land on the hole (rows 3 and 4), row 7 clamps
    hole2 = _rows(lambda y, x: 0x22 if y in (2, 3) else 0x24 if y == 7 else 0x20)
    cases.append(("an uncovered hole", 3, 3, in_order([[rec(0, 0, 8, 3, 0, 0, 0), rec(0, 5, 8, 3, 0, 0, 0)], [rec(0, 0, 8, 8, 0, 4, 0)]]),
                  same({1: _rows(lambda y, x: 0x12 if y in (3, 4) else 0x10), 2: hole2})))
    # left half two pixels to the left: columns 0 and 1 clamp in x; right half one row up: row 0 clamps in y
    cases.append(("a vector clamped in x only and one in y only", 3, 2, in_order([[rec(0, 0, 4, 8, -8, 0, 0), rec(4, 0, 4, 8, 0, -4, 0)]]),
                  same({1: _rows(lambda y, x: 0x14 if x < 2 or (x >= 4 and y == 0) else 0x10)})))
    # one pixel to the right, twice: column 7 clamps in frame 1; in frame 2 column 6 is clean itself and lands on it
    cases.append(("a clean pixel that lands on a flagged one", 3, 3, in_order([[rec(0, 0, 8, 8, 4, 0, 0)], [rec(0, 0, 8, 8, 4, 0, 0)]]),
                  same({1: _rows(lambda y, x: 0x14 if x == 7 else 0x10), 2: _rows(lambda y, x: 0x24 if x >= 6 else 0x20)})))
    cases.append(("a 17-frame chain of ref 0 links saturating at 15", 3, 18, in_order([[STILL]] * 17),
                  same({f: _flat(min(f, 15) << 4) for f in range(1, 18)})))
    # frame 1 is all intra (ref -1: P entry intra; bi entry a forward code whose target is not chained).  ref 2 from frame 2: max(0, -1) = 0
    cases.append(("ref 2 from frame 2", 3, 3, in_order([[rec(0, 0, 8, 8, 4, 4, -1)], [rec(0, 0, 8, 8, 0, 0, 2)]]),
                  same({1: _flat(0x11), 2: _flat(0x10)})))
    # decode order 1 3 2.  Frame 3 links to frame 1 (2 hops).  Frame 2: list 0 everywhere, still, to frame 1 (2 hops, clean); list 1 on the
    # block, four pixels to the right into frame 3 (3 hops): columns 4 and 5 clamp.  |1 - 2| == |3 - 2|: NEAR takes list 0
    bi = [rec(0, 0, 8, 8, 0, 0, 0, 0), rec(2, 2, 4, 4, 16, 0, -1, 1)]
    mean = _patch(_patch(_flat(0x20), 2, 6, 2, 4, 0x30), 2, 6, 4, 6, 0x34)
    cases.append(("a bi block with one clamped and one clean list", 3, 4, [(1, _a([STILL])), (3, _a([rec(0, 0, 8, 8, 0, 0, 1)])), (2, _a(bi))],
                  {"list0": {1: _flat(0x10), 3: _flat(0x20), 2: _flat(0x20)}, "near": {1: _flat(0x10), 3: _flat(0x20), 2: _flat(0x20)},
                   "mean": {1: _flat(0x10), 3: _flat(0x20), 2: mean}}))
    # list 0 everywhere with ref 1: the keyframe, 1 hop, two frames away; list 1 on the block into frame 3, one frame away, 3 hops
    bi_near = [rec(0, 0, 8, 8, 0, 0, 1, 0), rec(2, 2, 4, 4, 16, 0, -1, 1)]
    l1 = _patch(_patch(_flat(0x10), 2, 6, 2, 4, 0x30), 2, 6, 4, 6, 0x34)
    cases.append(("a bi block, NEAR takes the clamped list 1", 3, 4, [(1, _a([STILL])), (3, _a([rec(0, 0, 8, 8, 0, 0, 1)])), (2, _a(bi_near))],
                  {"list0": {1: _flat(0x10), 3: _flat(0x20), 2: _flat(0x10)}, "near": {1: _flat(0x10), 3: _flat(0x20), 2: l1},
                   "mean": {1: _flat(0x10), 3: _flat(0x20), 2: l1}}))
    # frame 2 has records on the block only: outside it uncovered (to frame 1: 2 hops); columns 2 and 3 are won by an unusable record
    cases.append(("an unusable winner over a usable lower index", 3, 3,
                  in_order([[STILL], [rec(2, 2, 4, 4, 0, 0, 0), rec(2, 2, 2, 4, 0, 0, 5)]]),
                  same({1: _flat(0x10), 2: _patch(_patch(_flat(0x22), 2, 6, 4, 6, 0x20), 2, 6, 2, 4, 0x21)})))
    # decode order 1 3 2, frames 3 and 2 without a record: both fall to p = 1, not to f - 1
    gap = _patch(_flat(0x22), 0, 2, 0, 2, 0x23)
    cases.append(("intra with a gap in D", 3, 4, [(1, _a([STILL, rec(0, 0, 2, 2, 0, 0, 9)])), (3, _a([])), (2, _a([]))],
                  same({1: _patch(_flat(0x10), 0, 2, 0, 2, 0x11), 3: gap, 2: gap})))
    return cases


def hand_expected(frames, gop):
    want = np.zeros((gop, 8, 8), dtype=np.uint8)
    for f, lit in frames.items():
        want[f] = np.array(lit, dtype=np.uint8)
    return want


def is_p_case(pushes):
    """In display order and every record in list 0: the P entry takes the case too."""
    return [f for f, _ in pushes] == list(range(1, len(pushes) + 1)) and not any((np.asarray(r).reshape(-1, 8)[:, 7] & 1).any() for _, r in pushes)


# ---- generated GOPs ----
GOP = 8
ORDERS = ((1, 2, 3, 4, 5, 6, 7), (3, 1, 2, 6, 4, 5, 7), (2, 1, 4, 3, 6, 5, 7))          # in order, and two B decode orders max_ref 3 can serve
SEED = 5                            # chosen on the CPU: with it the oracle alone meets the spread test_mv_link.py asserts
SHAPES = ((8, 8), (24, 40), (37, 53))
BANDED = (300, 200)                 # taller than the scatter's 256-row band


def _pick_ref(rng, f, D, max_ref):
    """A reference code: mostly one whose target is chained, a few whose target is not, a few out of range."""
    codes = list(range(-max_ref, max_ref))
    target = lambda r: max(0, f - r - 1) if r >= 0 else f - r
    ok = [r for r in codes if target(r) in D]
    undone = [r for r in codes if target(r) not in D]
    u = rng.random()
    if u < 0.03:
        return int(rng.choice([max_ref, max_ref + 2, -max_ref - 1, 90, -90]))
    if u < 0.06 and undone:
        return int(rng.choice(undone))
    return int(rng.choice(ok))


def make_gop(seed, H, W, order, max_ref, list1=True, gop=GOP):
    """[(f, int16 [n,8])] in the decode order `order`: 8x8 blocks each with no record (a hole), one list or both, vectors of up to 3.5 pixels
    (so that border blocks clamp), a few rectangles under and over the blocks, off-frame records, zero padding.  list1=False: every record
    in list 0 (what the P entry takes when the order is 1, 2, ...)."""
    rng = np.random.default_rng([seed, H, W, max_ref, int(list1)] + list(order))
    D, pushes = {0}, []
    for f in order:
        rows = []

        def one(x, y, w, h, l):
            hi = int(rng.integers(-8192, 8192)) * 2                  # bits 1..15 of reserved: ignored
            rows.append(rec(x, y, w, h, int(rng.integers(-14, 15)), int(rng.integers(-14, 15)), _pick_ref(rng, f, D, max_ref), hi | (l if list1 else 0)))

        one(int(rng.integers(-4, W)), int(rng.integers(-4, H)), int(rng.integers(1, 20)), int(rng.integers(1, 20)), int(rng.integers(0, 2)))
        for by in range(0, H, 8):
            for bx in range(0, W, 8):
                kind = int(rng.choice(4, p=[0.06, 0.44, 0.15, 0.35]))
                if kind in (1, 3):
                    one(bx, by, 8, 8, 0)
                if kind in (2, 3):
                    one(bx, by, 8, 8, 1)
                if rng.random() < 0.1:
                    rows.append([0] * 8)                              # padding between records
        for _ in range(2):                                            # these win over the blocks
            one(int(rng.integers(-4, W)), int(rng.integers(-4, H)), int(rng.integers(1, 10)), int(rng.integers(1, 10)), int(rng.integers(0, 2)))
        one(W, 3, 8, 8, 0)
        one(-9, -9, 9, 9, 1)                                          # wholly off the frame
        rows += [[0] * 8] * 3
        pushes.append((f, _a(rows)))
        D.add(f)
    return pushes


def banded_gop(max_ref):
    """Frames 1..3 at BANDED in display order, list 0 only, with a frame-sized record put first (the scatter cuts it into bands of 256 rows)."""
    H, W = BANDED
    out = []
    for i, (f, r) in enumerate(make_gop(SEED, H, W, (1, 2, 3), max_ref, list1=False, gop=4)):
        out.append((f, np.concatenate([_a([rec(-3, -3, W + 9, H + 9, 6 + i, -10, 0, 0)]), r])))
    return out


@functools.lru_cache(maxsize=None)
def generated(H, W, order, max_ref, policy, list1=True):
    """(pushes, link) of the generated GOP; computed once per process and shared (treat as read-only)."""
    pushes = make_gop(SEED, H, W, order, max_ref, list1)
    link = chain(pushes, H, W, GOP, max_ref, policy)
    link.setflags(write=False)
    return pushes, link


@functools.lru_cache(maxsize=None)
def generated_banded(max_ref):
    pushes = banded_gop(max_ref)
    link = chain_p([r for _, r in pushes], BANDED[0], BANDED[1], 4, max_ref)
    link.setflags(write=False)
    return pushes, link


# ---- the linked consistency form ----
TC_NSTATS = 3 + 3 * 32


def consistency_linked(labels, ref, mv_q, n_cls, link, link_mask):
    """labels uint8 [N,H,W], ref uint8 [R,H,W] (R == 1: shared), mv_q int16 [N,H,W,2], link uint8 [N,H,W] -> (change uint8 [N,H,W], stats int64
    [N,TC_NSTATS], unlinked int64 [N]).  Per pixel, in this order: unlinked (link & link_mask), outside, void, agree / differ."""
    labels, ref, mv_q, link = (np.asarray(a) for a in (labels, ref, mv_q, link))
    N, H, W = labels.shape
    change = np.zeros((N, H, W), dtype=np.uint8)
    st = np.zeros((N, TC_NSTATS), dtype=np.int64)
    unlinked = np.zeros(N, dtype=np.int64)
    for n in range(N):
        r_plane = ref[n if ref.shape[0] > 1 else 0]
        for y in range(H):
            for x in range(W):
                if int(link[n, y, x]) & link_mask:
                    change[n, y, x] = 128
                    unlinked[n] += 1
                    continue
                tx = x + round(int(mv_q[n, y, x, 0]) / 4)
                ty = y + round(int(mv_q[n, y, x, 1]) / 4)
                if not (0 <= tx < W and 0 <= ty < H):
                    change[n, y, x] = 128
                    st[n, 1] += 1
                    continue
                k, r = int(labels[n, y, x]), int(r_plane[ty, tx])
                if r >= n_cls or k >= n_cls:
                    change[n, y, x] = 128
                    st[n, 2] += 1
                    continue
                st[n, 0] += 1
                st[n, 3 + k] += 1
                st[n, 35 + r] += 1
                if k == r:
                    st[n, 67 + k] += 1
                else:
                    change[n, y, x] = 255
    return change, st, unlinked
