"""Plain-Python oracle of the block search (include/arseg_hip.h, arseg_block_motion_fwd) and the cases the CPU and GPU tests share.  Written
from the definition alone -- a loop per block and per candidate -- and independent of ingest.block_motion_numpy, which it checks."""
import functools

import numpy as np

INTRA_REF, NSTATS = 16, 4
RGB8, NV12, I420, P010, I010 = 0, 1, 2, 3, 4
SEED = 20261


def luma8(plane, fmt=NV12):
    p = np.asarray(plane)
    if fmt == RGB8:
        c = p.astype(np.int64)
        return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)
    if fmt == P010:
        return (p.astype(np.uint16).astype(np.int64) >> 8).astype(np.uint8)
    if fmt == I010:
        return ((p.astype(np.uint16).astype(np.int64) & 0x3ff) >> 2).astype(np.uint8)
    assert p.dtype == np.uint8
    return p


def search(cur8, ref8, B, R, lam):
    """Per block in record order: (x0, y0, w, h, dx, dy, sad) of the winner, by the definition: every candidate in turn, the smallest (cost, rank)."""
    a, b = np.asarray(cur8).astype(np.int64), np.asarray(ref8).astype(np.int64)
    H, W = a.shape
    out = []
    for bi in range(-(-H // B)):
        for bj in range(-(-W // B)):
            x0, y0 = bj * B, bi * B
            w, h = min(B, W - x0), min(B, H - y0)
            blk = a[y0:y0 + h, x0:x0 + w]
            best = None
            for dy in range(-R, R + 1):
                if y0 + dy < 0 or y0 + h + dy > H:
                    continue
                for dx in range(-R, R + 1):
                    if x0 + dx < 0 or x0 + w + dx > W:
                        continue
                    sad = int(np.abs(blk - b[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w]).sum())
                    rank = 0 if (dx, dy) == (0, 0) else 1 + (dy + R) * (2 * R + 1) + (dx + R)
                    cand = (sad + lam * (abs(dx) + abs(dy)), rank, dx, dy, sad)
                    if best is None or cand[:2] < best[:2]:
                        best = cand
            out.append((x0, y0, w, h, best[2], best[3], best[4]))
    return out


def outputs(winners, intra, ref_index=0):
    """(records int16 [n,8], sad uint32 [n], stats int64 [4]) of search()'s winners under an intra bound."""
    rec, sads, st = [], [], [0, 0, 0, 0]
    for x0, y0, w, h, dx, dy, sad in winners:
        sads.append(sad)
        if sad > intra * w * h:
            rec.append((x0, y0, w, h, 0, 0, INTRA_REF, 0))
            st[0] += 1
        else:
            rec.append((x0, y0, w, h, 4 * dx, 4 * dy, ref_index, 0))
            st[1] += (dx, dy) == (0, 0)
            st[2] += sad
            st[3] += w * h
    return np.array(rec, dtype=np.int16).reshape(-1, 8), np.array(sads, dtype=np.uint32), np.array(st, dtype=np.int64)


# ---- frame contents ----
def canvas(seed=SEED, H=160, W=224):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W), dtype=np.uint8)


def window(cv, y, x, H, W):
    return np.ascontiguousarray(cv[y:y + H, x:x + W])


def shifted_pair(H, W, sx, sy, seed=SEED, margin=40):
    """cur[y][x] = ref[y + sy][x + sx]: two windows of one noise canvas."""
    cv = canvas(seed, H + 2 * margin, W + 2 * margin)
    return window(cv, margin + sy, margin + sx, H, W), window(cv, margin, margin, H, W)


def content(kind, H, W):
    """(cur, ref) uint8 luma planes [H,W]."""
    if kind == "noise":                                               # windows of one i.i.d. canvas, 2 right and 1 up of each other
        return shifted_pair(H, W, 2, -1)
    if kind == "constant":                                            # every candidate ties: the zero vector (rank 0) must win
        return np.full((H, W), 93, np.uint8), np.full((H, W), 93, np.uint8)
    if kind == "stripes":                                             # vertical stripes of period 4: every dx = 0 mod 4 and every dy tie at SAD 0
        row = np.where(np.arange(W) % 4 < 2, 40, 200).astype(np.uint8)
        f = np.ascontiguousarray(np.broadcast_to(row, (H, W)))
        return f, f.copy()
    if kind == "texture":                                             # smooth, quantised to 8 bits: many near-ties
        from arseg_amd import synth

        t = synth._texture(np.random.Generator(np.random.PCG64(SEED + 3)), H + 8, W + 8)[..., 1]
        q = np.clip(np.floor(t * 255.0 + 0.5), 0, 255).astype(np.uint8)
        return window(q, 3, 5, H, W), window(q, 4, 2, H, W)
    raise ValueError(kind)


def format_planes(fmt, H, W, seed=SEED + 11):
    """(cur, ref) as format ``fmt`` holds them, the frames 3 right and 2 down of each other: uint8 [H,W] (NV12 / I420), uint8 [H,W,3] (RGB8),
    uint16 [H,W] with every bit the format ignores -- and the code bits luma8 drops -- random (P010, I010)."""
    g = np.random.Generator(np.random.PCG64(seed + fmt))
    m = 8
    if fmt == RGB8:
        cv = g.integers(0, 256, (H + 2 * m, W + 2 * m, 3), dtype=np.uint8)
    elif fmt in (NV12, I420):
        cv = g.integers(0, 256, (H + 2 * m, W + 2 * m), dtype=np.uint8)
    else:
        cv = g.integers(0, 1 << 16, (H + 2 * m, W + 2 * m), dtype=np.uint16)
    cur, ref = np.ascontiguousarray(cv[m + 2:m + 2 + H, m + 3:m + 3 + W]), np.ascontiguousarray(cv[m:m + H, m:m + W])
    noise = g.integers(-2, 3, cur.shape)                               # a little sensor noise: the winner's SAD is not 0
    if cur.dtype == np.uint16:
        s = 8 if fmt == P010 else 2                                    # the eight bits luma8 keeps start here
        v = cur.astype(np.int64)
        v = (v & ~(0xff << s)) | (np.clip(((v >> s) & 0xff) + noise, 0, 255) << s)
        # what luma8 does not look at differs between the frames
        cur = (v ^ (g.integers(0, 1 << 16, cur.shape) & (0x00ff if fmt == P010 else 0xfc03))).astype(np.uint16)
    else:
        cur = np.clip(cur.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return cur, ref


FORMATS = (RGB8, NV12, I420, P010, I010)
SIZES = ((5, 7), (16, 16), (37, 53))
BLOCKS, RADII, LAMS, INTRAS = (8, 16), (1, 6, 32), (0, 3), (0, 20, 255)
KINDS = ("noise", "constant", "stripes", "texture")


def search_cases():
    """(kind, H, W, B, R, lam) of every searched case: all sizes x blocks x radii x lams x contents; stripes at lam = 0 only (the rank rule)."""
    return [(k, H, W, B, R, lam) for k in KINDS for (H, W) in SIZES for B in BLOCKS for R in RADII for lam in LAMS if not (k == "stripes" and lam)]


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def winners_of(kind, H, W, B, R, lam):
    cur, ref = content(kind, H, W)
    return tuple(search(cur, ref, B, R, lam))


@functools.lru_cache(maxsize=None)
def gop_frames(H=64, W=96, n=5, seed=SEED + 7):
    """n luma frames: windows of one canvas panned by (2, 1) per frame, frame 3 with a rectangle of fresh noise (nothing in frame 2 matches it)."""
    cv = canvas(seed)
    frames = [window(cv, 30 + f, 30 + 2 * f, H, W).copy() for f in range(n)]
    g = np.random.Generator(np.random.PCG64(seed + 1))
    frames[3][16:40, 32:64] = g.integers(0, 256, (24, 32), dtype=np.uint8)
    return tuple(frames)


def abi_cases():
    """(name, arguments of arseg_block_motion_fwd, expected status): every refusal the header lists, on pointers that are never dereferenced
    because validation comes before any launch.  The workspace need is 0, so no size can be too small: ARSEG_EWORKSPACE has no case."""
    import ctypes

    EINVAL = -1
    good = dict(cur=0x1000, cur_pitch=64, ref=0x2000, ref_pitch=64, fmt=NV12, H=32, W=48, B=16, R=8, lam=2, intra=255, ref_index=0, records=0x3000,
                sad=0x4000, stats=0x5000, ws=0, ws_bytes=0)
    order = ("cur", "cur_pitch", "ref", "ref_pitch", "fmt", "H", "W", "B", "R", "lam", "intra", "ref_index", "records", "sad", "stats", "ws", "ws_bytes")

    def args(**kw):
        v = dict(good, **kw)
        return tuple(ctypes.c_void_p(v[k]) if k in ("cur", "ref", "records", "sad", "stats", "ws") else v[k] for k in order) + (ctypes.c_void_p(0),)

    bad = [("null cur", dict(cur=0)), ("null ref", dict(ref=0)), ("null records", dict(records=0)),
           ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H = 8193", dict(H=8193)), ("W = 8193", dict(W=8193, cur_pitch=8193, ref_pitch=8193)),
           ("B = 4", dict(B=4)), ("B = 12", dict(B=12)), ("B = 32", dict(B=32)), ("R = 0", dict(R=0)), ("R = 33", dict(R=33)),
           ("lambda = -1", dict(lam=-1)), ("lambda = 256", dict(lam=256)), ("intra = -1", dict(intra=-1)), ("intra = 256", dict(intra=256)),
           ("ref_index = -1", dict(ref_index=-1)), ("ref_index = 16", dict(ref_index=16)), ("format 5", dict(fmt=5)), ("format -1", dict(fmt=-1)),
           ("cur pitch below a row", dict(cur_pitch=47)), ("ref pitch below a row", dict(ref_pitch=47)),
           ("P010 pitch below 2 W", dict(fmt=P010, cur_pitch=94, ref_pitch=96)), ("RGB8 pitch below 3 W", dict(fmt=RGB8, cur_pitch=144, ref_pitch=143)),
           ("I010 odd pitch", dict(fmt=I010, cur_pitch=97, ref_pitch=96)), ("P010 odd ref pitch", dict(fmt=P010, cur_pitch=96, ref_pitch=97)),
           ("P010 odd cur pointer", dict(fmt=P010, cur_pitch=96, ref_pitch=96, cur=0x1001)),
           ("I010 odd ref pointer", dict(fmt=I010, cur_pitch=96, ref_pitch=96, ref=0x2001)),
           ("records not 16-byte aligned", dict(records=0x3008)), ("sad not 4-byte aligned", dict(sad=0x4002)),
           ("stats not 8-byte aligned", dict(stats=0x5004))]
    return [(name, args(**kw), EINVAL) for name, kw in bad]
