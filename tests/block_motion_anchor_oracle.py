"""Loop oracle of the keyframe anchoring (include/arseg_hip.h, arseg_block_motion_anchor_fwd), written straight from the words of the contract:
per block the centre list as a list, the candidates as a set, the winner as the smallest (cost, dy, dx) tuple -- no keys, no ranks, no
vectorisation over blocks.  tests/test_block_motion_anchor.py holds ingest.block_motion_anchor_numpy to it, tests/test_gpu_block_motion_anchor.py
the kernel.  Also the case generators both files share."""
import functools

import numpy as np

import block_motion_oracle as bmo

SEED = 20263
INTRA_REF, NSTATS = 16, 4


def round_half_even_div4(v):
    v = int(v)
    b, r = v >> 2, v & 3
    return b + (1 if r > 2 or (r == 2 and b & 1) else 0)


def geometry(b, H, W, B):
    bx = -(-W // B)
    bi, bj = divmod(b, bx)
    x0, y0 = bj * B, bi * B
    return bi, bj, x0, y0, min(B, W - x0), min(B, H - y0)


def hop(record):
    """((hx, hy), usable) of a block's input record."""
    if int(record[6]) != 0:
        return (0, 0), False
    return (round_half_even_div4(record[4]), round_half_even_div4(record[5])), True


def pred(b, records, mp, H, W, B):
    _, _, x0, y0, w, h = geometry(b, H, W, B)
    (hx, hy), _ = hop(records[b])
    xc, yc = x0 + w // 2, y0 + h // 2
    px, py = min(max(xc + hx, 0), W - 1), min(max(yc + hy, 0), H - 1)
    return hx + (int(mp[py, px, 0]) >> 2), hy + (int(mp[py, px, 1]) >> 2)


def centres(b, records, mp, H, W, B):
    by, bx = -(-H // B), -(-W // B)
    bi, bj, x0, y0, w, h = geometry(b, H, W, B)
    xc, yc = x0 + w // 2, y0 + h // 2
    cs = [(0, 0), pred(b, records, mp, H, W, B), (int(mp[yc, xc, 0]) >> 2, int(mp[yc, xc, 1]) >> 2)]
    for qi, qj in ((bi, bj - 1), (bi, bj + 1), (bi - 1, bj), (bi + 1, bj)):
        if 0 <= qi < by and 0 <= qj < bx and hop(records[qi * bx + qj])[1]:
            cs.append(pred(qi * bx + qj, records, mp, H, W, B))
    return cs


def candidates(cs, r, x0, y0, w, h, H, W):
    out = set()
    for cx, cy in cs:
        for oy in range(-r, r + 1):
            for ox in range(-r, r + 1):
                dx, dy = cx + ox, cy + oy
                if 0 <= x0 + dx and x0 + w + dx <= W and 0 <= y0 + dy and y0 + h + dy <= H:
                    out.add((dx, dy))
    assert (0, 0) in out
    return out


def winners(cur, key, records, mp, B, r, lam, counts=None):
    """Per block (dx, dy, sad, drift, hop usable) of the winning candidate.  ``counts``: a list that receives the number of candidates per block."""
    cur, key = np.asarray(cur).astype(np.int64), np.asarray(key).astype(np.int64)
    H, W = cur.shape
    out = []
    for b in range(-(-H // B) * -(-W // B)):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        cs = centres(b, records, mp, H, W, B)
        c1x, c1y = cs[1]
        block = cur[y0:y0 + h, x0:x0 + w]
        best = None
        cands = candidates(cs, r, x0, y0, w, h, H, W)
        for dx, dy in cands:
            sad = int(np.abs(block - key[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w]).sum())
            drift = abs(dx - c1x) + abs(dy - c1y)
            t = (sad + lam * drift, dy, dx, sad, drift)
            if best is None or t[:3] < best[:3]:
                best = t
        if counts is not None:
            counts.append(len(cands))
        out.append((best[2], best[1], best[3], best[4], hop(records[b])[1]))
    return out


def outputs(win, records, f, intra, H, W, B):
    """(records_out int16 [n,8], sad_of_anchored int64 [n] with -1 for a block kept on its hop, stats int64 [4]) from ``winners``."""
    rec = np.array(records, dtype=np.int16).copy()
    sad_a = np.full(len(win), -1, dtype=np.int64)
    st = [0, 0, 0, 0]
    for b, (dx, dy, sad, drift, usable) in enumerate(win):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        if sad <= intra * w * h:
            rec[b] = (x0, y0, w, h, 4 * dx, 4 * dy, f - 1, 0)
            sad_a[b] = sad
            st[0] += 1
            st[1] += not usable
            st[3] += drift
        else:
            st[2] += 1
    return rec, sad_a, np.array(st, dtype=np.int64)


def anchor(cur, key, records, mp, f, B, r, lam, intra):
    """The whole entry point on the loops."""
    H, W = np.asarray(cur).shape
    if f == 1:
        n = len(records)
        return np.array(records, dtype=np.int16).copy(), np.full(n, -1, dtype=np.int64), np.zeros(NSTATS, dtype=np.int64)
    return outputs(winners(cur, key, records, mp, B, r, lam), records, f, intra, H, W, B)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- the grid of cases ----
SIZES = bmo.SIZES                                                      # 5 x 7: one clipped block; 16 x 16: one block, no neighbours; 37 x 53
KINDS = ("noise", "constant", "stripes")
BLOCKS, REFINES, LAMS, INTRAS, FRAMES = (8, 16), (1, 2, 3), (0, 3), (0, 20, 255), (2, 5, 16)
TOTAL, HOP = (5, -3), (2, -1)                                          # cur[y][x] = key[y - 3][x + 5]; the hop's share of it


def grid_records(H, W, B, mvx=0, mvy=0, ref=0):
    n = -(-H // B) * -(-W // B)
    rec = np.zeros((n, 8), dtype=np.int16)
    for b in range(n):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        rec[b] = (x0, y0, w, h, mvx, mvy, ref, 0)
    return rec


def planes(kind, H, W, seed=SEED):
    """(cur, key): noise windows of one canvas TOTAL apart, a constant image (cost alone decides; at lam = 0 the smallest dy, then dx) or
    stripes of period 4 (every dx = 1 mod 4 ties at SAD 0)."""
    if kind == "noise":
        return bmo.shifted_pair(H, W, TOTAL[0], TOTAL[1], seed)
    if kind == "constant":
        return np.full((H, W), 93, np.uint8), np.full((H, W), 93, np.uint8)
    if kind == "stripes":
        row = lambda s: np.ascontiguousarray(np.broadcast_to(np.where((np.arange(W) + s) % 4 < 2, 40, 200).astype(np.uint8), (H, W)))
        return row(TOTAL[0]), row(0)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(kind, H, W, B):
    """(cur, key, records, merged_prev) of a grid case: most hops are HOP and most of merged_prev is 4 (TOTAL - HOP), so that the noise windows
    anchor at SAD 0 wherever the displaced block is inside; a fifth of the hops carry quarter-pel jitter (the rounding), a tenth are intra
    and a tenth point at another frame (both unusable); a fifth of merged_prev's blocks are off by a few pixels and a tenth of its samples
    carry low bits (the shift)."""
    g = np.random.Generator(np.random.PCG64(SEED + 1000 * H + 10 * W + B))
    cur, key = planes(kind, H, W)
    rec = grid_records(H, W, B, 4 * HOP[0], 4 * HOP[1])
    n = len(rec)
    what = g.integers(0, 10, n)
    for b in range(n):
        if what[b] in (0, 1):
            rec[b, 4:6] += g.integers(-3, 4, 2).astype(np.int16)
        elif what[b] == 2:
            rec[b, 4:7] = (0, 0, INTRA_REF)
        elif what[b] == 3:
            rec[b, 4:7] = (int(g.integers(-20, 21)), int(g.integers(-20, 21)), 3)
    mp = np.empty((H, W, 2), dtype=np.int64)
    mp[...] = (4 * (TOTAL[0] - HOP[0]), 4 * (TOTAL[1] - HOP[1]))
    for b in range(n):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        if g.integers(0, 5) == 0:
            mp[y0:y0 + h, x0:x0 + w] += 4 * g.integers(-4, 5, 2)
    low = g.integers(0, 10, (H, W)) == 0
    mp[low] += g.integers(-3, 4, (int(low.sum()), 2))
    return cur, key, rec, mp.astype(np.int16)


def grid_cases():
    return [(kind, H, W, B) for kind in KINDS for (H, W) in SIZES for B in BLOCKS]


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def winners_of(kind, H, W, B, r, lam):
    cur, key, rec, mp = case(kind, H, W, B)
    return winners(cur, key, rec, mp, B, r, lam)


# ---- hand-built cases ----
def hand_cases():
    """name -> dict(cur, key, records, mp, f, B, r, lam, intra).  All on noise windows TOTAL apart unless said otherwise."""
    out = {}
    H, W = 48, 56
    cur, key = planes("noise", H, W, SEED + 5)
    base = dict(cur=cur, key=key, f=3, B=16, r=2, lam=2, intra=20)
    true_prev = np.empty((H, W, 2), dtype=np.int16)
    true_prev[...] = (4 * (TOTAL[0] - HOP[0]), 4 * (TOTAL[1] - HOP[1]))
    hops = grid_records(H, W, 16, 4 * HOP[0], 4 * HOP[1])
    # one block that fills the frame: every centre's candidates but (0, 0) are off the frame
    c1, k1 = planes("noise", 16, 16, SEED + 6)
    mp1 = np.full((16, 16, 2), 400, dtype=np.int16)
    out["only (0, 0) remains"] = dict(base, cur=c1, key=k1, records=grid_records(16, 16, 16, 40, -36), mp=mp1, intra=255)
    # predictions far outside the frame, both signs
    far = np.full((H, W, 2), 4 * 8191, dtype=np.int16)
    far[:, W // 2:] = -4 * 8191
    out["predictions far outside"] = dict(base, records=grid_records(H, W, 16, 32764, -32768), mp=far, intra=255, r=3)
    out["predictions far outside, B = 8"] = dict(base, records=grid_records(H, W, 8, -32768, 32767), mp=far, intra=255, r=1, B=8)
    # a static scene: all seven centres are (0, 0)
    out["coinciding centres"] = dict(base, cur=key.copy(), records=grid_records(H, W, 16), mp=np.zeros((H, W, 2), dtype=np.int16))
    out["coinciding centres, moving"] = dict(base, records=hops, mp=true_prev)
    # unusable hops, as the block itself and as a neighbour: block 5 is interior (row 1, col 1 of 3 x 4)
    bad = hops.copy()
    bad[5, 4:7] = (0, 0, INTRA_REF)
    bad[6, 4:7] = (-12, 8, 3)
    bad[1, 4:7] = (8, 8, -1)
    odd = true_prev.copy()
    odd[8:40, 8:40] += np.int16(8)                                      # what the unusable blocks' neighbours propose differs from the co-located vector
    out["unusable hops"] = dict(base, records=bad, mp=odd, f=4)
    out["unusable hops, r = 1, lam = 0"] = dict(base, records=bad, mp=odd, f=4, r=1, lam=0)
    # halves: 6 / 4 -> 2, 10 / 4 -> 2, -6 / 4 -> -2, -10 / 4 -> -2 (half to even)
    half = hops.copy()
    half[:, 4], half[:, 5] = 6, -10
    half[::2, 4], half[::2, 5] = 10, -6
    prev_half = np.empty((H, W, 2), dtype=np.int16)
    prev_half[...] = (4 * (TOTAL[0] - 2), 4 * (TOTAL[1] + 2))
    out["hop fields 6 and 10"] = dict(base, records=half, mp=prev_half, r=1)
    # merged_prev -3 -> -1 and 5 -> 1 (arithmetic shift): TOTAL - (-1, 1) by the hop
    shift = np.empty((H, W, 2), dtype=np.int16)
    shift[...] = (5, -3)
    out["merged_prev -3 and 5"] = dict(base, records=grid_records(H, W, 16, 4 * (TOTAL[0] - 1), 4 * (TOTAL[1] + 1)), mp=shift, r=1)
    # one row and one column of blocks: no upper / lower, no left / right neighbour
    cr, kr = planes("noise", 8, 44, SEED + 7)
    out["one row of blocks"] = dict(base, cur=cr, key=kr, records=grid_records(8, 44, 8, 4 * HOP[0], 0), B=8,
                                    mp=np.broadcast_to(np.array((4 * (TOTAL[0] - HOP[0]), 0), dtype=np.int16), (8, 44, 2)).copy(), intra=255)
    cc, kc = planes("noise", 44, 8, SEED + 8)
    out["one column of blocks"] = dict(base, cur=cc, key=kc, records=grid_records(44, 8, 8, 0, 4 * HOP[1]), B=8,
                                       mp=np.broadcast_to(np.array((0, 4 * (TOTAL[1] - HOP[1])), dtype=np.int16), (44, 8, 2)).copy(), intra=255)
    return out


def bound_case(extra):
    """One 16 x 16 block that fills the frame, so (0, 0) is the only candidate: cur = key + 3 has SAD 3 * 256 = intra w h exactly at intra = 3;
    ``extra`` raises one sample by that much more."""
    key = bmo.canvas(SEED + 9, 16, 16) // 2
    cur = key + 3
    cur[7, 9] += extra
    return dict(cur=cur.astype(np.uint8), key=key.astype(np.uint8), records=grid_records(16, 16, 16, 8, 8), mp=np.zeros((16, 16, 2), dtype=np.int16),
                f=2, B=16, r=1, lam=1, intra=3)


def tiles_case(H=100, W=150, B=16, seed=SEED + 21):
    """Several workgroups' worth of blocks at 360 x 480: noise windows TOTAL apart with +-2 of noise, a rectangle of fresh noise, hops and
    merged_prev near the truth with a tenth of the blocks unusable and a tenth of merged_prev's blocks off."""
    g = np.random.Generator(np.random.PCG64(seed))
    cur, key = planes("noise", H, W, seed)
    cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    cur[H // 4:H // 2, W // 3:W // 2] = g.integers(0, 256, (H // 2 - H // 4, W // 2 - W // 3), dtype=np.uint8)
    rec = grid_records(H, W, B, 4 * HOP[0], 4 * HOP[1])
    n = len(rec)
    pick = g.integers(0, 10, n)
    rec[pick == 0, 4:7] = (0, 0, INTRA_REF)
    rec[pick == 1, 4] += np.int16(8)
    mp = np.empty((H, W, 2), dtype=np.int64)
    mp[...] = (4 * (TOTAL[0] - HOP[0]), 4 * (TOTAL[1] - HOP[1]))
    for b in np.nonzero(g.integers(0, 10, n) == 0)[0]:
        _, _, x0, y0, w, h = geometry(int(b), H, W, B)
        mp[y0:y0 + h, x0:x0 + w] += 4 * g.integers(-5, 6, 2)
    return cur, key, rec, mp.astype(np.int16)


# ---- the capability: a panned GOP with an occluder in one frame ----
GOP, PAN, OCC = 6, (3, -2), (32, 64, 48, 80)                           # frames; merged[f] = 4 f PAN; the occluder's rows and columns in frame 2
CAP = dict(H=96, W=128, B=16, R=8, lam=2, intra=20, r=2, max_ref=16)
INTERIOR = (slice(16, 80), slice(16, 96))


@functools.lru_cache(maxsize=None)
def gop_frames():
    """GOP frames 96 x 128 of one PCG64(7) byte-noise canvas: frame_f[y][x] = frame_0[y - 2 f][x + 3 f]; a 32 x 32 rectangle of fresh noise in
    frame 2 only."""
    g = np.random.Generator(np.random.PCG64(7))
    H, W, m = CAP["H"], CAP["W"], 24
    cv = g.integers(0, 256, (H + 2 * m, W + 2 * m), dtype=np.uint8)
    frames = [bmo.window(cv, m + PAN[1] * f, m + PAN[0] * f, H, W).copy() for f in range(GOP)]
    y0, y1, x0, x1 = OCC
    frames[2][y0:y1, x0:x1] = g.integers(0, 256, (y1 - y0, x1 - x0), dtype=np.uint8)
    return tuple(frames)


def leaves_frame(f):
    """bool [H,W]: the pixels of the blocks of frame f whose position displaced by f PAN is not inside the keyframe."""
    H, W, B = CAP["H"], CAP["W"], CAP["B"]
    out = np.zeros((H, W), dtype=bool)
    for b in range((H // B) * (W // B)):
        _, _, x0, y0, w, h = geometry(b, H, W, B)
        dx, dy = f * PAN[0], f * PAN[1]
        if not (0 <= x0 + dx and x0 + w + dx <= W and 0 <= y0 + dy and y0 + h + dy <= H):
            out[y0:y0 + h, x0:x0 + w] = True
    return out


def off_truth(merged_f, f):
    """The number of interior pixels whose merged value is not exactly 4 f PAN."""
    return int((merged_f[INTERIOR] != (4 * f * PAN[0], 4 * f * PAN[1])).any(axis=-1).sum())


def run_gop(hop_fn, anchor_fn=None, corrupt=None):
    """The GOP on the host: per frame ``hop_fn(cur, prev)`` -> records, optionally ``corrupt(f, records)``, optionally
    ``anchor_fn(cur, key, records, merged[f - 1], f)`` -> (records, sad, stats); the chain is ingest.chain_records_numpy with max_ref = 16 and
    links.  Returns (merged, link, pushes, [stats per frame])."""
    from arseg_amd import ingest

    frames = gop_frames()
    H, W = frames[0].shape
    pushes, stats = [], [None]
    merged = np.zeros((GOP, H, W, 2), dtype=np.int16)
    link = None
    for f in range(1, GOP):
        rec = hop_fn(frames[f], frames[f - 1])
        if corrupt is not None:
            rec = corrupt(f, rec)
        st = None
        if anchor_fn is not None:
            rec, _, st = anchor_fn(frames[f], frames[0], rec, merged[f - 1] if f >= 2 else None, f)
        stats.append(st)
        pushes.append((f, rec))
        merged, link = ingest.chain_records_numpy(pushes, H, W, GOP, CAP["max_ref"], return_link=True)
    return merged, link, pushes, stats


# ---- the C ABI's refusals ----
def abi_cases():
    """(name, arguments, expected status) for arseg_block_motion_anchor_fwd: every refusal the header lists, on pointers that are never
    dereferenced because validation comes before any launch.  37 x 53 in blocks of 16 is 12 records, 192 bytes."""
    import ctypes

    P = ctypes.c_void_p
    good = dict(cur=0x1000, cur_pitch=64, key=0x3000, key_pitch=56, H=37, W=53, B=16, r=2, lam=2, intra=20, f=2, rin=0x10000, mp=0x100000, rout=0x20000,
                sad=0x30000, stats=0x40000)
    order = ("cur", "cur_pitch", "key", "key_pitch", "H", "W", "B", "r", "lam", "intra", "f", "rin", "mp", "rout", "sad", "stats")
    bad = [("null cur", dict(cur=0)), ("null key", dict(key=0)), ("null records_in", dict(rin=0)), ("null records_out", dict(rout=0)),
           ("null merged_prev at f = 2", dict(mp=0)), ("null key at f = 1", dict(key=0, f=1)), ("H = 0", dict(H=0)), ("H = 8193", dict(H=8193)), ("W = 0", dict(W=0)),
           ("W = 8193", dict(W=8193, cur_pitch=8196, key_pitch=8196)), ("B = 4", dict(B=4)), ("B = 12", dict(B=12)), ("B = 32", dict(B=32)), ("r = 0", dict(r=0)),
           ("r = 4", dict(r=4)), ("lambda = -1", dict(lam=-1)), ("lambda = 256", dict(lam=256)), ("intra = -1", dict(intra=-1)), ("intra = 256", dict(intra=256)),
           ("f = 0", dict(f=0)), ("f = 17", dict(f=17)), ("f = -1", dict(f=-1)), ("cur base not 4-byte aligned", dict(cur=0x1002)),
           ("key base not 4-byte aligned", dict(key=0x3001)), ("cur pitch no multiple of 4", dict(cur_pitch=62)), ("key pitch no multiple of 4", dict(key_pitch=57)),
           ("cur pitch below (W + 3) & ~3", dict(cur_pitch=52)), ("key pitch below (W + 3) & ~3", dict(key_pitch=52)), ("negative pitch", dict(cur_pitch=-64)),
           ("records_in not 16-byte aligned", dict(rin=0x10008)), ("records_out not 16-byte aligned", dict(rout=0x20004)),
           ("merged_prev not 4-byte aligned", dict(mp=0x100002)), ("sad not 4-byte aligned", dict(sad=0x30002)), ("stats not 8-byte aligned", dict(stats=0x40004)),
           ("records in place", dict(rout=0x10000)), ("records_out inside records_in", dict(rout=0x10000 + 176)), ("records_in inside records_out", dict(rout=0x10000 - 176)),
           ("records in place at f = 1", dict(rout=0x10000, f=1)), ("unaligned plane at f = 1", dict(cur=0x1001, f=1))]
    out = []
    for name, kw in bad:
        v = dict(good, **kw)
        out.append((name, tuple(P(v[k]) if k in ("cur", "key", "rin", "mp", "rout", "sad", "stats") else v[k] for k in order) + (P(0),), -1))
    return out
