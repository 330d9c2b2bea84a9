"""Loop oracle of the quad-tree split (include/arseg_hip.h, arseg_block_motion_split_fwd), written straight from the words of the contract: per
parent the usability test, per child the centre list as a list, the candidates as a set, the winner as the smallest (cost, rank) tuple, the
decision as the two sums -- no keys, no vectorisation over blocks.  tests/test_block_motion_split.py holds ingest.block_motion_split_numpy
to it, tests/test_gpu_block_motion_split.py the kernel.  Also the case generators both files share."""
import functools

import numpy as np

import block_motion_oracle as bmo

SEED = 20265
INTRA_REF, NSTATS, MAX_V = 16, 6, 500


def round_half_even_div4(v):
    v = int(v)
    b, r = v >> 2, v & 3
    return b + (1 if r > 2 or (r == 2 and b & 1) else 0)


def grid(H, W):
    return -(-H // 16), -(-W // 16)


def parent_vector(records, bi, bj, H, W, ref_index):
    """(P, usable) of parent (bi, bj), which is in the grid."""
    by, bx = grid(H, W)
    q = records[bi * bx + bj]
    P = (round_half_even_div4(q[4]), round_half_even_div4(q[5]))
    x0, y0 = 16 * bj, 16 * bi
    w, h = min(16, W - x0), min(16, H - y0)
    inside = 0 <= x0 + P[0] and x0 + w + P[0] <= W and 0 <= y0 + P[1] and y0 + h + P[1] <= H
    return P, int(q[6]) == ref_index and abs(P[0]) <= MAX_V and abs(P[1]) <= MAX_V and inside


def child_geometry(bi, bj, q, H, W):
    qx, qy = q & 1, q >> 1
    x0, y0 = 16 * bj + 8 * qx, 16 * bi + 8 * qy
    return x0, y0, min(8, W - x0), min(8, H - y0)


def centres(records, bi, bj, q, H, W, ref_index):
    by, bx = grid(H, W)
    qx, qy = q & 1, q >> 1
    cs = [(0, 0)]
    P, usable = parent_vector(records, bi, bj, H, W, ref_index)
    if usable:
        cs.append(P)
    for ni, nj in ((bi, bj + (1 if qx else -1)), (bi + (1 if qy else -1), bj)):
        if 0 <= ni < by and 0 <= nj < bx:
            N, ok = parent_vector(records, ni, nj, H, W, ref_index)
            if ok:
                cs.append(N)
    return cs


def rank(dx, dy):
    return 0 if (dx, dy) == (0, 0) else 1 + (dy + 511) * 1023 + (dx + 511)


def search(cur, ref, records, r, lam, ref_index=0):
    """Per parent (usable, P, [child or None] * 4), child = (x0, y0, w, h, dx, dy, sad, cost, S(P) or None)."""
    cur, ref = np.asarray(cur).astype(np.int64), np.asarray(ref).astype(np.int64)
    H, W = cur.shape
    by, bx = grid(H, W)
    out = []
    for bi in range(by):
        for bj in range(bx):
            P, usable = parent_vector(records, bi, bj, H, W, ref_index)
            kids = []
            for q in range(4):
                x0, y0, w, h = child_geometry(bi, bj, q, H, W)
                if w <= 0 or h <= 0:
                    kids.append(None)
                    continue
                block = cur[y0:y0 + h, x0:x0 + w]
                cands = set()
                for cx, cy in centres(records, bi, bj, q, H, W, ref_index):
                    for oy in range(-r, r + 1):
                        for ox in range(-r, r + 1):
                            dx, dy = cx + ox, cy + oy
                            if 0 <= x0 + dx and x0 + w + dx <= W and 0 <= y0 + dy and y0 + h + dy <= H:
                                cands.add((dx, dy))
                assert (0, 0) in cands and (not usable or P in cands)
                sads = {d: int(np.abs(block - ref[y0 + d[1]:y0 + d[1] + h, x0 + d[0]:x0 + d[0] + w]).sum()) for d in cands}
                best = min(cands, key=lambda d: (sads[d] + lam * (abs(d[0]) + abs(d[1])), rank(*d)))
                kids.append((x0, y0, w, h, best[0], best[1], sads[best], sads[best] + lam * (abs(best[0]) + abs(best[1])), sads[P] if usable else None))
            out.append((usable, P, kids))
    return out


def outputs(found, lam, intra, split_gain, ref_index=0):
    """(children int16 [4 nb,8], child_sad uint32 [4 nb], stats int64 [6]) from ``search``."""
    rows, sads, st = [], [], [0] * NSTATS
    for usable, P, kids in found:
        live = [k for k in kids if k is not None]
        matched = [k is not None and k[6] <= intra * k[2] * k[3] for k in kids]
        if usable:
            lhs = sum(k[8] for k in live) + lam * (abs(P[0]) + abs(P[1])) - sum(k[7] for k in live)
            split = lhs > split_gain
        else:
            split = any(matched)
        if split:
            st[0] += 1
            if usable:
                st[4] += lhs
            else:
                st[1] += 1
        for k, m in zip(kids, matched):
            sads.append(0 if k is None else k[6])
            if not split or k is None:
                rows.append((0,) * 8)
            elif m:
                rows.append((k[0], k[1], k[2], k[3], 4 * k[4], 4 * k[5], ref_index, 0))
                st[2] += 1
                st[5] += k[2] * k[3]
            else:
                rows.append((k[0], k[1], k[2], k[3], 0, 0, INTRA_REF, 0))
                st[3] += 1
    return np.array(rows, dtype=np.int16).reshape(-1, 8), np.array(sads, dtype=np.uint32), np.array(st, dtype=np.int64)


def recount(children, ref_index=0):
    """What of stats a recount of the child rows alone gives: [0], [2], [3] and [5] (which parents were unusable and the gain are not in the rows)."""
    c = np.asarray(children).astype(np.int64).reshape(-1, 4, 8)
    written = c[..., 2] > 0
    matched = written & (c[..., 6] == ref_index)
    return int(written.any(axis=1).sum()), int(matched.sum()), int((written & (c[..., 6] == INTRA_REF)).sum()), int((c[..., 2] * c[..., 3])[matched].sum())


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def grid_records(H, W, mvx=0, mvy=0, ref=0, B=16):
    by, bx = -(-H // B), -(-W // B)
    rec = np.zeros((by * bx, 8), dtype=np.int16)
    for b in range(by * bx):
        x0, y0 = (b % bx) * B, (b // bx) * B
        rec[b] = (x0, y0, min(B, W - x0), min(B, H - y0), mvx, mvy, ref, 0)
    return rec


# ---- the two-layer scene: two noise canvases that meet at a straight border mid-block, each translated parallel to the border ----
LEFT, RIGHT = (0, 3), (0, -2)                                          # cur[y][x] = ref[y + dy][x + dx] per layer; nothing is occluded


def two_layer_frames(H, W, border, n=2, seed=SEED + 1, axis="x"):
    """n frames uint8 [H,W]: frame f of the layer below ``border`` is the layer's canvas moved f times by LEFT, the other by RIGHT; frame f is the
    current frame to frame f - 1.  axis "y": the border is a row and the vectors are transposed (the layers slide horizontally)."""
    if axis == "y":
        return tuple(np.ascontiguousarray(f.T) for f in two_layer_frames(W, H, border, n, seed))
    assert border % 16 == 8
    g = np.random.Generator(np.random.PCG64(seed))
    m = 3 * n + 3
    a, b = (g.integers(0, 256, (H + 2 * m, W), dtype=np.uint8) for _ in range(2))
    left = np.arange(W)[None, :] < border
    return tuple(np.where(left, a[m + LEFT[1] * f:m + LEFT[1] * f + H], b[m + RIGHT[1] * f:m + RIGHT[1] * f + H]) for f in range(n))


def true_field(H, W, border, hops=1, axis="x"):
    """int16 [H,W,2] in quarter pixels: the vector of every pixel from frame f to frame f - hops."""
    out = np.zeros((H, W, 2), dtype=np.int16)
    if axis == "y":
        out[:border], out[border:] = (4 * hops * LEFT[1], 4 * hops * LEFT[0]), (4 * hops * RIGHT[1], 4 * hops * RIGHT[0])
    else:
        out[:, :border], out[:, border:] = (4 * hops * LEFT[0], 4 * hops * LEFT[1]), (4 * hops * RIGHT[0], 4 * hops * RIGHT[1])
    return out


def interior_parents(H, W):
    """Parents (bi, bj) away from the frame border: not in the first or last row or column of the grid."""
    by, bx = grid(H, W)
    return [(bi, bj) for bi in range(1, by - 1) for bj in range(1, bx - 1)]


SCENE = dict(H=80, W=112, border=56, R=6, lam=2, r=2, split_gain=32)   # 5 x 7 parents; column 3 straddles the border


# ---- seeded noise cases with hand-planted records ----
NOISE_SIZES = ((37, 53), (48, 64), (100, 150))
NOMINAL = dict(r=2, lam=3, intra=20, split_gain=32, ref_index=0)      # where the spread of a noise case is asserted


@functools.lru_cache(maxsize=None)
def noise_case(H, W, ref_index=0):
    """(cur, ref, records_in): two layers with a border mid-block and +-2 of sensor noise, a rectangle of fresh noise (children that match
    nothing), and hand-planted parent records: most carry the left layer's vector (right of the border the children's neighbours know
    better), a tenth quarter-pel jitter, a tenth are intra (healed where a child matches), the rest of a fifth point at another frame, carry
    500 or 501 pixels, or lead out of the frame."""
    g = np.random.Generator(np.random.PCG64(SEED + 1000 * H + W))
    border = (W // 32) * 16 + 8
    ref, cur = two_layer_frames(H, W, border, 2, SEED + H)
    cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    cur[H // 2:H // 2 + 12, 4:24] = g.integers(0, 256, (12, 20), dtype=np.uint8)
    by, bx = grid(H, W)
    rec = grid_records(H, W, 4 * LEFT[0], 4 * LEFT[1], ref_index)
    for b in range(by * bx):
        bj = b % bx
        if 16 * bj >= border + 24:                                     # two columns right of the border know their own layer
            rec[b, 4:6] = (4 * RIGHT[0], 4 * RIGHT[1])
    what = g.integers(0, 20, by * bx)
    what[:6] = (2, 4, 5, 6, 7, 3)                                      # every kind at least once, whatever the draw
    for b in range(by * bx):
        k = what[b]
        if k in (0, 1):
            rec[b, 4:6] += g.integers(-3, 4, 2).astype(np.int16)
        elif k in (2, 3):
            rec[b, 4:7] = (0, 0, INTRA_REF)
        elif k == 4:
            rec[b, 4:7] = (int(g.integers(-20, 21)), int(g.integers(-20, 21)), ref_index + 1)
        elif k == 5:
            rec[b, 4:6] = (4 * 500, -4 * 500)
        elif k == 6:
            rec[b, 4:6] = (-4 * 501, 8) if b % 2 else (8, 4 * 501)
        elif k == 7:
            rec[b, 4:6] = (-4 * (16 * bj + 1), 0)                       # one pixel past the left edge
    return cur, ref, rec


def noise_cases():
    return [(H, W) for (H, W) in NOISE_SIZES]


@functools.lru_cache(maxsize=None)
def noise_found(H, W, r, lam):
    cur, ref, rec = noise_case(H, W)
    return search(cur, ref, rec, r, lam)


# ---- the grid of small sizes: records from the estimators' host forms and hand-planted ----
SIZES = ((5, 7), (16, 16), (37, 53), (48, 64))                         # only child 0; one parent, no neighbours; clipped children at both edges
REFINES, LAMS, INTRAS, GAINS = (1, 2, 3), (0, 3), (0, 20, 255), (0, 32, 65535)
SOURCES = ("full", "pyr", "planted")


@functools.lru_cache(maxsize=None)
def grid_case(source, H, W):
    """(cur, ref, records_in): ``full`` / ``pyr`` search a two-layer pair with sensor noise on the host (intra 20: the straddling parents come out
    intra at some sizes and matched at others); ``planted`` is the noise case's content cut to size with its kinds of records."""
    from arseg_amd import ingest

    if source == "planted":
        if (H, W) in NOISE_SIZES:
            return noise_case(H, W)
        cur, ref, rec = noise_case(48, 64)
        keep = [b for b in range(len(rec)) if rec[b, 0] < W and rec[b, 1] < H]
        return np.ascontiguousarray(cur[:H, :W]), np.ascontiguousarray(ref[:H, :W]), np.ascontiguousarray(rec[keep])
    g = np.random.Generator(np.random.PCG64(SEED + 7 * H + W))
    ref, cur = two_layer_frames(H, W, 8 if W < 40 else 24, 2, SEED + 3 * H)
    cur = np.clip(cur.astype(np.int64) + g.integers(-2, 3, cur.shape), 0, 255).astype(np.uint8)
    if source == "full":
        return cur, ref, ingest.block_motion_numpy(cur, ref, B=16, R=6, lam=2, intra=20)[0]
    return cur, ref, ingest.block_motion_pyr_numpy(cur, ref, B=16, Rt=2, r=1, lam=2, intra=40, levels=2)[0]


def grid_cases():
    return [(s, H, W) for s in SOURCES for (H, W) in SIZES]


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def grid_found(source, H, W, r, lam):
    cur, ref, rec = grid_case(source, H, W)
    return search(cur, ref, rec, r, lam)


def rank_cases():
    """name -> (cur, ref, records_in, r, lam): a constant image (every candidate ties: (0, 0), rank 0, wins at lam = 0 too) and vertical stripes
    of period 4 moved by one column with parents that carry (-3, 0): SAD 0 at every dx = 1 mod 4 and at every dy; the smallest dy, then dx."""
    H, W = 48, 64
    flat = np.full((H, W), 93, np.uint8)
    row = lambda s: np.ascontiguousarray(np.broadcast_to(np.where((np.arange(W) + s) % 4 < 2, 40, 200).astype(np.uint8), (H, W)))
    return {"constant": (flat, flat.copy(), grid_records(H, W, 8, -4), 2, 0),
            "constant, lam 3": (flat, flat.copy(), grid_records(H, W, 8, -4), 3, 3),
            "stripes": (row(1), row(0), grid_records(H, W, -12, 0), 3, 0),
            "stripes, r 1": (row(1), row(0), grid_records(H, W, 4, 4), 1, 0)}


# ---- the C ABI's refusals ----
def abi_cases():
    """(name, arguments, expected status) for arseg_block_motion_split_fwd: every refusal the header lists, on pointers that are never
    dereferenced because validation comes before any launch.  37 x 53 is 12 parents: 192 bytes of records_in, 768 of children."""
    import ctypes

    P = ctypes.c_void_p
    good = dict(cur=0x1000, cur_pitch=64, ref=0x3000, ref_pitch=56, H=37, W=53, r=2, lam=2, intra=20, gain=32, ref_index=0, rin=0x10000, kids=0x20000,
                sad=0x30000, stats=0x40000)
    order = ("cur", "cur_pitch", "ref", "ref_pitch", "H", "W", "r", "lam", "intra", "gain", "ref_index", "rin", "kids", "sad", "stats")
    bad = [("null cur", dict(cur=0)), ("null ref", dict(ref=0)), ("null records_in", dict(rin=0)), ("null children", dict(kids=0)), ("H = 0", dict(H=0)),
           ("H = 8193", dict(H=8193)), ("W = 0", dict(W=0)), ("W = 8193", dict(W=8193, cur_pitch=8196, ref_pitch=8196)), ("r = 0", dict(r=0)), ("r = 4", dict(r=4)),
           ("lambda = -1", dict(lam=-1)), ("lambda = 256", dict(lam=256)), ("intra = -1", dict(intra=-1)), ("intra = 256", dict(intra=256)),
           ("split_gain = -1", dict(gain=-1)), ("split_gain = 65536", dict(gain=65536)), ("ref_index = -1", dict(ref_index=-1)), ("ref_index = 16", dict(ref_index=16)),
           ("cur base not 4-byte aligned", dict(cur=0x1002)), ("ref base not 4-byte aligned", dict(ref=0x3001)), ("cur pitch no multiple of 4", dict(cur_pitch=62)),
           ("ref pitch no multiple of 4", dict(ref_pitch=57)), ("cur pitch below (W + 3) & ~3", dict(cur_pitch=52)), ("ref pitch below (W + 3) & ~3", dict(ref_pitch=52)),
           ("negative pitch", dict(cur_pitch=-64)), ("records_in not 16-byte aligned", dict(rin=0x10008)), ("children not 16-byte aligned", dict(kids=0x20004)),
           ("child_sad not 4-byte aligned", dict(sad=0x30002)), ("stats not 8-byte aligned", dict(stats=0x40004)), ("children in place", dict(kids=0x10000)),
           ("children start inside records_in", dict(kids=0x10000 + 176)), ("records_in inside children", dict(kids=0x10000 - 752)),
           ("records_in is the children's last row", dict(kids=0x10000 - 576))]
    out = []
    for name, kw in bad:
        v = dict(good, **kw)
        out.append((name, tuple(P(v[k]) if k in ("cur", "ref", "rin", "kids", "sad", "stats") else v[k] for k in order) + (P(0),), -1))
    return out
