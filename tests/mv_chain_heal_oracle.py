"""Loop oracle of the chain healing (include/arseg_hip.h, arseg_mv_chain_heal_fwd), written straight from the words of the contract: per block
the flagged pixels counted one by one, the centres as a list, the candidates as a set, the winner as the smallest (cost, dy, dx) tuple,
SAD_flagged as a loop over the flagged pixels, the corrected link row as a recount of the plane before and after -- no keys, no masks, no
vectorisation over blocks.  tests/test_mv_chain_heal.py holds ingest.mv_chain_heal_numpy to it, tests/test_gpu_mv_chain_heal.py the two
launches.  Also the case generators both files share and the two capability scenes."""
import functools

import numpy as np

import block_motion_anchor_oracle as bma
import block_motion_oracle as bmo

SEED = 20271
NSTATS, LINK_NSTATS = 6, 20
INTRA, UNCOVERED, CLAMPED = 1, 2, 4
TOTAL = bma.TOTAL                                                      # cur[y][x] = key[y - 3][x + 5] on the noise windows
geometry = bma.geometry


def recount(plane):
    """The row of link counters a plane gives: pixels with INTRA, UNCOVERED, CLAMPED, any flag, then the 16 hop bins."""
    v = np.asarray(plane).astype(np.int64).reshape(-1)
    return np.array([int((v & 1).sum()), int(((v >> 1) & 1).sum()), int(((v >> 2) & 1).sum()), int(((v & 7) != 0).sum())]
                    + [int(((v >> 4) == hops).sum()) for hops in range(16)], dtype=np.int64)


def is_flagged(link, x, y, mask):
    return (int(link[y, x]) & mask) != 0


def flagged_pixels(b, link, H, W, B, mask):
    _, _, x0, y0, w, h = geometry(b, H, W, B)
    return [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w) if is_flagged(link, x, y, mask)]


def vector_at(merged, x, y):
    return int(merged[y, x, 0]) >> 2, int(merged[y, x, 1]) >> 2        # Python's >> on a negative int is the arithmetic shift


def centres(b, merged, link, H, W, B, mask):
    by, bx = -(-H // B), -(-W // B)
    bi, bj, x0, y0, w, h = geometry(b, H, W, B)
    cs = [(0, 0), vector_at(merged, x0 + w // 2, y0 + h // 2)]
    for qi, qj in ((bi, bj - 1), (bi, bj + 1), (bi - 1, bj), (bi + 1, bj)):
        if 0 <= qi < by and 0 <= qj < bx:
            _, _, qx0, qy0, qw, qh = geometry(qi * bx + qj, H, W, B)
            if not is_flagged(link, qx0 + qw // 2, qy0 + qh // 2, mask):
                cs.append(vector_at(merged, qx0 + qw // 2, qy0 + qh // 2))
    for y in range(y0, y0 + h):
        row = [x for x in range(x0, x0 + w) if not is_flagged(link, x, y, mask)]
        if row:
            cs.append(vector_at(merged, row[0], y))
            break
    return cs


def winner(b, cur, key, merged, link, B, r, lam, mask, count=None):
    """(dx, dy, SAD_flagged, drift, SAD_all) of the winning candidate of block b."""
    H, W = cur.shape
    _, _, x0, y0, w, h = geometry(b, H, W, B)
    cs = centres(b, merged, link, H, W, B, mask)
    c1x, c1y = cs[1]
    block = cur[y0:y0 + h, x0:x0 + w]
    best = None
    cands = bma.candidates(cs, r, x0, y0, w, h, H, W)
    for dx, dy in cands:
        sad = int(np.abs(block - key[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w]).sum())
        t = (sad + lam * (abs(dx - c1x) + abs(dy - c1y)), dy, dx, sad)
        if best is None or t[:3] < best[:3]:
            best = t
    _, dy, dx, sad_all = best
    sad_fl = 0
    for x, y in flagged_pixels(b, link, H, W, B, mask):
        sad_fl += abs(int(cur[y, x]) - int(key[y + dy, x + dx]))
    if count is not None:
        count.append(len(cands))
    return dx, dy, sad_fl, abs(dx - c1x) + abs(dy - c1y), sad_all


def winners(cur, key, merged, link, B, r, lam, mask):
    """{b: winner} for every block with at least one flagged pixel (what any min_flagged may examine)."""
    cur, key = np.asarray(cur).astype(np.int64), np.asarray(key).astype(np.int64)
    H, W = cur.shape
    return {b: winner(b, cur, key, merged, link, B, r, lam, mask) for b in range(-(-H // B) * -(-W // B)) if flagged_pixels(b, link, H, W, B, mask)}


def outputs(win, merged, link, B, intra, mask, min_flagged, row=None):
    """(merged_f, link_f, decisions int16 [n,8], sad int64 [n] with -1 for a skipped block, stats int64 [6], corrected row or None) from
    ``winners``."""
    H, W = link.shape
    n_blocks = -(-H // B) * -(-W // B)
    m, l = np.array(merged, dtype=np.int16), np.array(link, dtype=np.uint8)
    dec = np.zeros((n_blocks, 8), dtype=np.int16)
    sad = np.full(n_blocks, -1, dtype=np.int64)
    st = [0] * NSTATS
    for b in range(n_blocks):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        px = flagged_pixels(b, link, H, W, B, mask)
        if len(px) < min_flagged:
            dec[b] = (x0, y0, w, h, 0, 0, 2, len(px))
            st[4] += len(px)
            continue
        dx, dy, sad_fl, drift, _ = win[b]
        healed = sad_fl <= intra * len(px)
        dec[b] = (x0, y0, w, h, 4 * dx, 4 * dy, 0 if healed else 1, len(px))
        sad[b] = sad_fl
        st[0] += 1
        st[2] += len(px)
        if healed:
            st[1] += 1
            st[3] += len(px)
            st[5] += drift
            for x, y in px:
                m[y, x] = (4 * dx, 4 * dy)
                l[y, x] = 0x10
    new_row = None if row is None else np.asarray(row, dtype=np.int64) - recount(link) + recount(l)
    return m, l, dec, sad, np.array(st, dtype=np.int64), new_row


def heal(cur, key, merged, link, B, r, lam, intra, mask, min_flagged, row=None):
    """The whole entry point on the loops."""
    merged, link = np.asarray(merged), np.asarray(link)
    return outputs(winners(cur, key, merged, link, B, r, lam, mask), merged, link, B, intra, mask, min_flagged, row)


def same(got, want):
    return len(got) == len(want) and all((g is None and w is None) or (g is not None and w is not None and np.array_equal(g, w)) for g, w in zip(got, want))


# ---- the grid of cases ----
SIZES = bmo.SIZES                                                      # 5 x 7: one clipped block; 16 x 16: one block, no neighbours; 37 x 53
KINDS = bma.KINDS                                                      # noise windows TOTAL apart, a constant image, stripes of period 4
FLAGSETS = ("blocks", "rects", "pixels", "centres", "all")
BLOCKS, REFINES, LAMS, INTRAS, MASKS, MIN_FLAGGED = (8, 16), (1, 2, 3), (0, 3), (0, 20, 255), (1, 3, 7), (1, 5, 64)


def flag_set(which, H, W, B, g):
    """bool [H,W]: whole blocks of the grid, rectangles off it, single pixels, the centre pixel of some blocks, or everything."""
    out = np.zeros((H, W), dtype=bool)
    n = -(-H // B) * -(-W // B)
    if which == "all":
        out[...] = True
    elif which == "blocks":
        for b in range(n):
            if b == 0 or g.integers(0, 3) == 0:
                _, _, x0, y0, w, h = geometry(b, H, W, B)
                out[y0:y0 + h, x0:x0 + w] = True
    elif which == "rects":
        for _ in range(1 + n // 6):
            y, x = int(g.integers(0, H)), int(g.integers(0, W))
            out[y:y + int(g.integers(1, 14)), x:x + int(g.integers(1, 14))] = True
    elif which == "pixels":
        out[g.integers(0, 12, (H, W)) == 0] = True
        out[0, 0] = True
    elif which == "centres":
        for b in range(n):
            if b % 2 == 0:
                _, _, x0, y0, w, h = geometry(b, H, W, B)
                out[y0 + h // 2, x0 + w // 2] = True
    else:
        raise ValueError(which)
    return out


@functools.lru_cache(maxsize=None)
def case(kind, H, W, B, which):
    """(cur, key, merged, link, row) of a grid case.  merged is 4 TOTAL on most unflagged pixels, so that the noise windows heal at SAD 0
    wherever the displaced block is inside; a fifth of the blocks are off by a few pixels, a tenth of the samples carry low bits (the shift),
    flagged pixels carry zero motion or anything.  Link bytes: hops 1 .. 15; a flagged pixel has one to three flags, so that the masks 1, 3 and
    7 see different sets; a twentieth of the others carry CLAMPED alone.  row: a recount of link plus a constant (rows are accumulated into)."""
    g = np.random.Generator(np.random.PCG64(SEED + 1000 * H + 10 * W + B + 7 * FLAGSETS.index(which)))
    cur, key = bma.planes(kind, H, W)
    m = np.empty((H, W, 2), dtype=np.int64)
    m[...] = (4 * TOTAL[0], 4 * TOTAL[1])
    for b in range(-(-H // B) * -(-W // B)):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        if g.integers(0, 5) == 0:
            m[y0:y0 + h, x0:x0 + w] += 4 * g.integers(-4, 5, 2)
    low = g.integers(0, 10, (H, W)) == 0
    m[low] += g.integers(-3, 4, (int(low.sum()), 2))
    fl = flag_set(which, H, W, B, g)
    wild = fl & (g.integers(0, 4, (H, W)) == 0)
    m[fl] = 0
    m[wild] = g.integers(-200, 201, (int(wild.sum()), 2))
    link = (g.integers(1, 16, (H, W)) << 4).astype(np.int64)
    link[fl] |= g.integers(1, 8, int(fl.sum()))
    link[~fl & (g.integers(0, 20, (H, W)) == 0)] |= CLAMPED
    link = link.astype(np.uint8)
    return cur, key, m.astype(np.int16), link, recount(link) + 1000


def grid_cases():
    return [(kind, H, W, B, which) for kind in KINDS for (H, W) in SIZES for B in BLOCKS for which in FLAGSETS]


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def winners_of(kind, H, W, B, which, r, lam, mask):
    cur, key, m, link, _ = case(kind, H, W, B, which)
    return winners(cur, key, m, link, B, r, lam, mask)


def grid_params():
    return [(r, lam, intra, mask, mf) for r in REFINES for lam in LAMS for intra in INTRAS for mask in MASKS for mf in MIN_FLAGGED]


# ---- hand-built cases ----
def _frame(seed=SEED + 5, H=48, W=56):
    """Noise windows TOTAL apart, 3 x 4 blocks of 16 (the last column clipped to 8): block 5 = row 1, column 1 is interior.  merged = 4 TOTAL,
    link = 0x20 everywhere (two hops, no flags)."""
    cur, key = bma.planes("noise", H, W, seed)
    m = np.empty((H, W, 2), dtype=np.int16)
    m[...] = (4 * TOTAL[0], 4 * TOTAL[1])
    return cur, key, m, np.full((H, W), 0x20, dtype=np.uint8)


def hand_cases():
    """name -> dict(cur, key, merged, link, B, r, lam, intra, mask, min_flagged).  Block 5 of _frame() is rows 16 .. 31, columns 16 .. 31."""
    out = {}
    base = dict(B=16, r=2, lam=2, intra=20, mask=3, min_flagged=1)
    # one block that fills the frame: every candidate but (0, 0) is off the frame, whatever the centres say
    k1 = bmo.canvas(SEED + 6, 16, 16)
    m1 = np.full((16, 16, 2), 400, dtype=np.int16)
    out["only (0, 0) remains"] = dict(base, cur=k1.copy(), key=k1, merged=m1, link=np.full((16, 16), 0x31, dtype=np.uint8))
    # merged is the truth everywhere, flagged pixels included: seven centres, two distinct
    cur, key, m, link = _frame()
    link[18:27, 19:30] = 0x21
    out["coinciding centres"] = dict(base, cur=cur, key=key, merged=m, link=link)
    # every neighbour's centre pixel, the block's own centre and its first pixel say something else; rows 16 .. 23 of the block stay unflagged
    cur, key, m, link = _frame()
    for (y, x), d in (((24, 24), (1, 0)), ((24, 8), (-6, 2)), ((24, 40), (0, -7)), ((8, 24), (7, 7)), ((40, 24), (-3, -9)), ((16, 16), (2, -5))):
        m[y, x] = (4 * (TOTAL[0] + d[0]), 4 * (TOTAL[1] + d[1]))
    link[24:32, 16:32] = 0x42
    out["seven different centres"] = dict(base, cur=cur, key=key, merged=m, link=link, r=1)
    # merged is wrong by (10, 10) everywhere; only the left neighbour's centre pixel (24, 8) knows the truth
    for name, byte in (("a flagged neighbour centre", 0x21), ("the same neighbour centre, unflagged", 0x20)):
        cur, key, m, link = _frame()
        m[...] = (4 * (TOTAL[0] + 10), 4 * (TOTAL[1] + 10))
        m[24, 8] = (4 * TOTAL[0], 4 * TOTAL[1])
        link[16:32, 16:32] = 0x21
        link[24, 8] = byte
        out[name] = dict(base, cur=cur, key=key, merged=m, link=link)
    # the whole block flagged: no C6; with one pixel spared it proposes the truth, which nothing else does
    for name, spare in (("no unflagged pixel in the block", False), ("one unflagged pixel in the block", True)):
        cur, key, m, link = _frame()
        m[...] = (4 * (TOTAL[0] - 9), 4 * (TOTAL[1] + 9))
        m[29, 23] = (4 * TOTAL[0], 4 * TOTAL[1])
        link[16:32, 16:32] = 0x12
        if spare:
            link[29, 23] = 0x10
        out[name] = dict(base, cur=cur, key=key, merged=m, link=link)
    # 23 >> 2 = 5, -11 >> 2 = -3 (not -2): the centre is the truth only under the arithmetic shift; the neighbours sit at +-4 * 8191
    cur, key, m, link = _frame()
    m[...] = (4 * 8191, -4 * 8191)
    m[:, 28:] = (-4 * 8191, 4 * 8191)
    m[24, 24] = (4 * TOTAL[0] + 3, 4 * TOTAL[1] + 1)
    link[16:32, 16:32] = 0xf1
    out["low bits, negative values and +-4 * 8191"] = dict(base, cur=cur, key=key, merged=m, link=link, r=1)
    # acceptance is about the flagged pixels: a fresh 4 x 4 patch under the flags in a block that otherwise matches exactly ...
    cur, key, m, link = _frame()
    cur, key = cur // 2, key // 2
    patch = np.random.Generator(np.random.PCG64(SEED + 8)).integers(128, 256, (4, 4), dtype=np.uint8)
    occluded = cur.copy()
    occluded[20:24, 20:24] = patch
    link[20:24, 20:24] = 0x21
    out["passes on the block, fails on the flagged pixels"] = dict(base, cur=occluded, key=key, merged=m, link=link)
    # ... and flagged pixels that match exactly in a block whose rest is 30 brighter
    brighter = cur.copy()
    brighter[16:32, 16:32] += 30
    brighter[20:24, 20:24] -= 30
    out["fails on the block, passes on the flagged pixels"] = dict(base, cur=brighter, key=key, merged=m, link=link)
    # hop nibbles 1, 7 and 15 and every flag under the healed pixels
    cur, key, m, link = _frame()
    link[17, 17:20], link[18, 17:21], link[19, 17:22] = 0x11, 0x72, 0xf7
    link[40, 40] = 0x24                                                # CLAMPED alone: outside the mask 3, so block 10 is not examined
    out["hop nibbles 1, 7 and 15"] = dict(base, cur=cur, key=key, merged=m, link=link)
    # exactly five flagged pixels
    cur, key, m, link = _frame()
    link[30, 17:22] = 0x32
    out["five flagged pixels"] = dict(base, cur=cur, key=key, merged=m, link=link, min_flagged=5)
    out["five flagged pixels, min_flagged 6"] = dict(base, cur=cur, key=key, merged=m, link=link, min_flagged=6)
    return out


def bound_case(extra):
    """One 16 x 16 block that fills the frame, so (0, 0) is the only candidate; ten flagged pixels 3 brighter than the keyframe: SAD_flagged =
    30 = intra n(b) exactly at intra = 3.  ``extra`` raises one of them by that much more.  The unflagged rest is 40 brighter: it must not count."""
    key = bmo.canvas(SEED + 9, 16, 16) // 2
    cur = key + 40
    cur[7, 3:13] = key[7, 3:13] + 3
    cur[7, 9] += extra
    link = np.full((16, 16), 0x30, dtype=np.uint8)
    link[7, 3:13] = 0x31
    return dict(cur=cur.astype(np.uint8), key=key.astype(np.uint8), merged=np.full((16, 16, 2), 8, dtype=np.int16), link=link, B=16, r=1, lam=1, intra=3,
                mask=1, min_flagged=1)


def run_case(fn, c, row=None, **kw):
    c = dict(c, **kw)
    return fn(c["cur"], c["key"], c["merged"], c["link"], c["B"], c["r"], c["lam"], c["intra"], c["mask"], c["min_flagged"], row)


def tiles_case(H=100, W=150, B=16, seed=SEED + 21, share=0.3):
    """Noise windows TOTAL apart with +-2 of noise and a rectangle of fresh noise; ``share`` of the blocks carry flagged pixels -- whole blocks,
    halves and sprinkles --, merged near the truth with a tenth of its blocks off."""
    g = np.random.Generator(np.random.PCG64(seed))
    cur, key = bma.planes("noise", H, W, seed)
    cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    cur[H // 4:H // 2, W // 3:W // 2] = g.integers(0, 256, (H // 2 - H // 4, W // 2 - W // 3), dtype=np.uint8)
    m = np.empty((H, W, 2), dtype=np.int64)
    m[...] = (4 * TOTAL[0], 4 * TOTAL[1])
    link = (g.integers(1, 16, (H, W)) << 4).astype(np.int64)
    n = -(-H // B) * -(-W // B)
    pick, how = g.random(n) < share, g.integers(0, 3, n)
    for b in range(n):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        if g.integers(0, 10) == 0:
            m[y0:y0 + h, x0:x0 + w] += 4 * g.integers(-5, 6, 2)
        if pick[b]:
            fl = np.zeros((h, w), dtype=bool)
            if how[b] == 0:
                fl[...] = True
            elif how[b] == 1:
                fl[h // 2:] = True
            else:
                fl[g.integers(0, 6, (h, w)) == 0] = True
            link[y0:y0 + h, x0:x0 + w][fl] |= g.integers(1, 4, int(fl.sum()))
            m[y0:y0 + h, x0:x0 + w][fl] = 0
    link = link.astype(np.uint8)
    return cur, key, m.astype(np.int16), link, recount(link)


# ---- the capability ----
CAP = dict(bma.CAP, mask=INTRA | UNCOVERED, min_flagged=1)
PAN = bma.PAN


def leaves_frame(f, H, W, B=16):
    """bool [H,W]: the pixels of the grid blocks of frame f whose position displaced by f PAN is not inside the keyframe."""
    out = np.zeros((H, W), dtype=bool)
    for b in range(-(-H // B) * -(-W // B)):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        dx, dy = f * PAN[0], f * PAN[1]
        if not (0 <= x0 + dx and x0 + w + dx <= W and 0 <= y0 + dy and y0 + h + dy <= H):
            out[y0:y0 + h, x0:x0 + w] = True
    return out


def off_truth(merged_f, f, where):
    """The number of pixels of the mask ``where`` whose merged value is not exactly 4 f PAN."""
    return int(((merged_f != (4 * f * PAN[0], 4 * f * PAN[1])).any(axis=-1) & where).sum())


def run_chain(pushes, frames, gop, max_ref, heal_fn=None, bidirectional=False):
    """The host chain (ingest.chain_records_numpy) over ``pushes`` = [(f, records)], with ``heal_fn(cur, key, merged_f, link_f, row)`` ->
    the oracle's tuple after every push.  Returns (merged, link, {f: stats of the heal}, {f: corrected row})."""
    from arseg_amd import ingest

    H, W = frames[0].shape
    stats, rows = {}, {}

    def after(f, m, l):
        if heal_fn is None:
            return m, l
        m2, l2, _, _, st, row = heal_fn(frames[f], frames[0], m, l, recount(l))
        stats[f], rows[f] = st, row
        return m2, l2

    merged, link = ingest.chain_records_numpy(pushes, H, W, gop, max_ref, return_link=True, after_push=after)
    return merged, link, stats, rows


def cap_heal(fn):
    return lambda cur, key, m, l, row: fn(cur, key, m, l, CAP["B"], CAP["r"], CAP["lam"], CAP["intra"], CAP["mask"], CAP["min_flagged"], row)


@functools.lru_cache(maxsize=None)
def scene1_pushes():
    """Scene 1: the panned GOP of tests/block_motion_anchor_oracle.py (96 x 128, an occluder in frame 2) as PLAIN hop records of the full search."""
    from arseg_amd import ingest

    frames = bma.gop_frames()
    return tuple((f, ingest.block_motion_numpy(frames[f], frames[f - 1], B=CAP["B"], R=CAP["R"], lam=CAP["lam"], intra=CAP["intra"])[0])
                 for f in range(1, bma.GOP))


# Scene 2: the same pan over 20 frames as a software decoder would describe it: prediction units off the grid, of mixed sizes, some intra,
# B-frames that reference a later frame, pushed in decode order
GOP2, MAX_REF2, LAST_INTRA2 = 20, 3, 17
ORDER2 = (1, 2, 3, 5, 4) + tuple(range(6, 20))                        # 4 is a B-frame: pushed after frame 5, which it looks ahead to


@functools.lru_cache(maxsize=None)
def scene2_frames():
    g = np.random.Generator(np.random.PCG64(11))
    H, W, m = bma.CAP["H"], bma.CAP["W"], 64
    cv = g.integers(0, 256, (H + 2 * m, W + 2 * m), dtype=np.uint8)
    return tuple(bmo.window(cv, m + PAN[1] * f, m + PAN[0] * f, H, W).copy() for f in range(GOP2))


@functools.lru_cache(maxsize=None)
def scene2_pushes():
    """[(f, records)] in ORDER2.  Per frame: 32 x 32 units from the origin (-12, -4), then 16 x 8 and 8 x 8 units at origins that are no multiples
    of 16, which win where they overlap.  A unit predicts from the previous frame (ref 0), from two frames back (ref 1) or, in a B-frame, from
    the next frame (ref -1: usable only because that frame was pushed first) with the pan times the distance; a unit whose prediction would
    reach outside the reference frame is intra, as an encoder codes content that enters the picture, and up to frame LAST_INTRA2 a sixth
    of the others are intra too although their content is in view (ref -1 in a P-frame, or an index out of range)."""
    H, W = bma.CAP["H"], bma.CAP["W"]
    g = np.random.Generator(np.random.PCG64(12))
    pushes = []
    for f in ORDER2:
        units = [(x, y, 32, 32) for y in range(-4, H, 32) for x in range(-12, W, 32)]
        for _ in range(40):
            w, h = ((16, 8), (8, 8))[int(g.integers(0, 2))]
            units.append((4 * int(g.integers(0, (W - w) // 4)) + 2 * int(g.integers(0, 2)), 4 * int(g.integers(0, (H - h) // 4)) + 1, w, h))
        forward = f == 4
        rows = []
        for x, y, w, h in units:
            choice = int(g.integers(0, 3))
            if forward and choice == 0:
                ref, dist = -1, -1                                      # the next frame
            elif (choice == 1 and f >= 2) or f == 5:                    # frame 5 is pushed before frame 4: it cannot look at it
                ref, dist = 1, 2
            else:
                ref, dist = 0, 1
            dx, dy = dist * PAN[0], dist * PAN[1]
            xa, xb, ya, yb = max(x, 0), min(x + w, W), max(y, 0), min(y + h, H)
            inside = 0 <= xa + dx and xb + dx <= W and 0 <= ya + dy and yb + dy <= H
            if not inside or (f <= LAST_INTRA2 and g.integers(0, 6) == 0):
                ref, dx, dy = (-1, 0, 0) if not forward and g.integers(0, 2) else (90, 0, 0)
            rows.append((x, y, w, h, 4 * dx, 4 * dy, ref, 0))
        pushes.append((f, np.array(rows, dtype=np.int16)))
    return tuple(pushes)


# ---- the C ABI's refusals ----
def abi_cases():
    """(name, arguments, expected status) for arseg_mv_chain_heal_fwd: every refusal the header lists, on pointers that are never dereferenced
    because validation comes before any launch."""
    import ctypes

    P = ctypes.c_void_p
    good = dict(cur=0x1000, cur_pitch=64, key=0x3000, key_pitch=56, H=37, W=53, B=16, r=2, lam=2, intra=20, mask=3, mf=1, merged=0x100000, link=0x200001,
                dec=0x20000, sad=0x30000, stats=0x40000, row=0x50000)
    order = ("cur", "cur_pitch", "key", "key_pitch", "H", "W", "B", "r", "lam", "intra", "mask", "mf", "merged", "link", "dec", "sad", "stats", "row")
    bad = [("null cur", dict(cur=0)), ("null key", dict(key=0)), ("null merged_f", dict(merged=0)), ("null link_f", dict(link=0)), ("null decisions", dict(dec=0)),
           ("H = 0", dict(H=0)), ("H = 8193", dict(H=8193)), ("W = 0", dict(W=0)), ("W = 8193", dict(W=8193, cur_pitch=8196, key_pitch=8196)),
           ("B = 4", dict(B=4)), ("B = 12", dict(B=12)), ("B = 32", dict(B=32)), ("r = 0", dict(r=0)), ("r = 4", dict(r=4)), ("lambda = -1", dict(lam=-1)),
           ("lambda = 256", dict(lam=256)), ("intra = -1", dict(intra=-1)), ("intra = 256", dict(intra=256)), ("flag_mask = 0", dict(mask=0)),
           ("flag_mask = 8", dict(mask=8)), ("flag_mask = -1", dict(mask=-1)), ("min_flagged = 0", dict(mf=0)), ("min_flagged = 65", dict(mf=65)),
           ("cur base not 4-byte aligned", dict(cur=0x1002)), ("key base not 4-byte aligned", dict(key=0x3001)),
           ("cur pitch no multiple of 4", dict(cur_pitch=62)), ("key pitch no multiple of 4", dict(key_pitch=57)),
           ("cur pitch below (W + 3) & ~3", dict(cur_pitch=52)), ("key pitch below (W + 3) & ~3", dict(key_pitch=52)), ("negative pitch", dict(cur_pitch=-64)),
           ("merged_f not 4-byte aligned", dict(merged=0x100002)), ("decisions not 16-byte aligned", dict(dec=0x20008)),
           ("sad not 4-byte aligned", dict(sad=0x30002)), ("stats not 8-byte aligned", dict(stats=0x40004)),
           ("link_stats_row not 8-byte aligned", dict(row=0x50004))]
    out = []
    for name, kw in bad:
        v = dict(good, **kw)
        out.append((name, tuple(P(v[k]) if k in ("cur", "key", "merged", "link", "dec", "sad", "stats", "row") else v[k] for k in order) + (P(0),), -1))
    return out
