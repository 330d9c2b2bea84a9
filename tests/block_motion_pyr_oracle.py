"""Plain-Python oracle of the hierarchical block search (include/arseg_hip.h, arseg_luma_pyramid_fwd and arseg_block_motion_pyr_fwd) and the
cases the CPU and GPU tests share.  Written from the definition alone -- a loop per pixel, per block, per centre and per candidate, the
tie-break as the words of the header and not as its rank formula -- and independent of ingest.luma_pyramid_numpy and
ingest.block_motion_pyr_numpy, which it checks.  The top level is block_motion_oracle.search, as the definition says."""
import functools

import numpy as np

import block_motion_oracle as bmo

INTRA_REF, NSTATS = bmo.INTRA_REF, bmo.NSTATS
SEED = 20262


# ---- pyramid ----
def pyramid(p0, levels):
    """[P_0 .. P_levels] of a luma8 plane, uint8 each: the rounded mean of 2 x 2, rows and columns clamped to the last."""
    out = [np.asarray(p0, dtype=np.uint8)]
    for _ in range(levels):
        src = out[-1].astype(np.int64).tolist()
        H, W = len(src), len(src[0])
        dst = [[(src[min(2 * y, H - 1)][min(2 * x, W - 1)] + src[min(2 * y, H - 1)][min(2 * x + 1, W - 1)] + src[min(2 * y + 1, H - 1)][min(2 * x, W - 1)]
                 + src[min(2 * y + 1, H - 1)][min(2 * x + 1, W - 1)] + 2) >> 2 for x in range((W + 1) >> 1)] for y in range((H + 1) >> 1)]
        out.append(np.array(dst, dtype=np.uint8))
    return out


def layout(H, W, levels):
    """([(offset, pitch, H_l, W_l)], total) of the pyramid buffer."""
    out, off = [], 0
    for _ in range(levels + 1):
        pitch = (W + 15) // 16 * 16
        out.append((off, pitch, H, W))
        off += pitch * H
        H, W = (H + 1) // 2, (W + 1) // 2
    return out, off


def levels_of(buffer, H, W, levels):
    """The [H_l, W_l] pixels of every level of a flat pyramid buffer (numpy uint8): padding left out."""
    lay, total = layout(H, W, levels)
    assert buffer.size >= total
    return [buffer[off:off + pitch * h].reshape(h, pitch)[:, :w] for off, pitch, h, w in lay]


# ---- parents, centres, candidates ----
def centres(bi, bj, parent_v, pby, pbx):
    """The centres of block (bi, bj), in the header's order; parent_v[(pi, pj)] = (dx, dy) at the level above."""
    pi, pj = bi >> 1, bj >> 1
    assert 0 <= pi < pby and 0 <= pj < pbx                             # the parent always exists
    out = [(0, 0), tuple(2 * v for v in parent_v[(pi, pj)])]
    nj = pj + (1 if bj & 1 else -1)
    if 0 <= nj < pbx:
        out.append(tuple(2 * v for v in parent_v[(pi, nj)]))
    ni = pi + (1 if bi & 1 else -1)
    if 0 <= ni < pby:
        out.append(tuple(2 * v for v in parent_v[(ni, pj)]))
    return out


def candidates(cs, r, x0, y0, w, h, H, W):
    """The union of centre + (ox, oy) over the centres, each vector once, that keep the displaced block inside the H x W level."""
    seen, out = set(), []
    for cx, cy in cs:
        for oy in range(-r, r + 1):
            for ox in range(-r, r + 1):
                dx, dy = cx + ox, cy + oy
                if (dx, dy) in seen:
                    continue
                seen.add((dx, dy))
                if 0 <= x0 + dx and x0 + w + dx <= W and 0 <= y0 + dy and y0 + h + dy <= H:
                    out.append((dx, dy))
    assert (0, 0) in out
    return out


def refine(cur, ref, parents, pby, pbx, B, r, lam, counts=None):
    """One level: parents = the winners of the level above, row-major over its pby x pbx grid -> this level's winners, row-major,
    (x0, y0, w, h, dx, dy, sad).  counts, a list, receives the number of candidates per block."""
    a, b = np.asarray(cur).astype(np.int64), np.asarray(ref).astype(np.int64)
    H, W = a.shape
    pv = {(i, j): (parents[i * pbx + j][4], parents[i * pbx + j][5]) for i in range(pby) for j in range(pbx)}
    out = []
    for bi in range(-(-H // B)):
        for bj in range(-(-W // B)):
            x0, y0 = bj * B, bi * B
            w, h = min(B, W - x0), min(B, H - y0)
            blk = a[y0:y0 + h, x0:x0 + w]
            best = None
            cands = candidates(centres(bi, bj, pv, pby, pbx), r, x0, y0, w, h, H, W)
            if counts is not None:
                counts.append(len(cands))
            for dx, dy in cands:
                sad = int(np.abs(blk - b[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w]).sum())
                # smallest cost; among equal costs (0, 0) first, then the smallest dy, then the smallest dx
                order = (sad + lam * (abs(dx) + abs(dy)), (dx, dy) != (0, 0), dy, dx)
                if best is None or order < best[0]:
                    best = (order, dx, dy, sad)
            out.append((x0, y0, w, h, best[1], best[2], best[3]))
    return out


def search(cur8, ref8, B, L, Rt, r, lam, counts=None):
    """The winners of level 0, per block in record order: the full search on level L, then L refinements."""
    pc, pr = pyramid(cur8, L), pyramid(ref8, L)
    win = bmo.search(pc[L], pr[L], B, Rt, lam)
    for l in range(L - 1, -1, -1):
        ph, pw = pc[l + 1].shape
        win = refine(pc[l], pr[l], win, -(-ph // B), -(-pw // B), B, r, lam, counts if l == 0 else None)
    return win


outputs = bmo.outputs

# ---- cases ----
SIZES = bmo.SIZES                                                      # 5 x 7: one clipped block, H_3 = 1; 37 x 53: odd at every level (37 -> 19 -> 10 -> 5)
BLOCKS, LEVELS, REFINES, LAMS, INTRAS = (8, 16), (1, 2, 3), (1, 2, 3), (0, 3), (0, 20, 255)
KINDS = ("noise", "constant", "stripes")
RT = 2                                                                 # the top level's radius in the grid of cases (the full search has its own tests)


def content(kind, H, W):
    if kind == "noise":                                                # windows of one canvas 7 right and 5 up of each other: beyond Rt at level 1, within it above
        return bmo.shifted_pair(H, W, 7, -5, seed=SEED)
    return bmo.content(kind, H, W)


def search_cases():
    """(kind, H, W, B, L, r, lam) of every searched case."""
    return [(k, H, W, B, L, r, lam) for k in KINDS for (H, W) in SIZES for B in BLOCKS for L in LEVELS for r in REFINES for lam in LAMS]


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def winners_of(kind, H, W, B, L, r, lam):
    cur, ref = content(kind, H, W)
    return tuple(search(cur, ref, B, L, RT, r, lam))


@functools.lru_cache(maxsize=None)
def tiles_pair():
    """100 x 150: several pyramid tiles and workgroups of blocks, every edge clipped at some level.  Noise moved by (-11, 6), a rectangle of
    fresh noise (intra at a moderate bound), smooth texture in the lower half (near-ties)."""
    H, W = 100, 150
    cur, ref = (p.copy() for p in bmo.shifted_pair(H, W, -11, 6, seed=SEED + 21))
    tc, tr = bmo.content("texture", 50, W)
    cur[50:], ref[50:] = tc, tr
    cur[20:45, 70:110] = bmo.canvas(SEED + 22, 25, 40)
    return cur, ref


@functools.lru_cache(maxsize=None)
def tiles_winners(B, L, Rt, r, lam):
    cur, ref = tiles_pair()
    return tuple(search(cur, ref, B, L, Rt, r, lam))


@functools.lru_cache(maxsize=None)
def gop_frames(H=128, W=192, n=5, seed=SEED + 7):
    """n luma frames: windows of one canvas panned by (-12, 4) per frame -- beyond a full search of 8, whole pixels at level 2 -- frame 3 with a
    rectangle of fresh noise (nothing in frame 2 matches it)."""
    cv = bmo.canvas(seed, H + 24, W + 56)
    frames = [bmo.window(cv, 4 + 4 * f, 52 - 12 * f, H, W).copy() for f in range(n)]
    g = np.random.Generator(np.random.PCG64(seed + 1))
    frames[3][32:80, 64:128] = g.integers(0, 256, (48, 64), dtype=np.uint8)
    return tuple(frames)


# ---- the capability: a translation beyond the full search's reach ----
def interior(H, W, B, L, sx, sy):
    """Record indices of the whole blocks whose level-L ancestor -- the B 2^L-aligned square around them -- displaced by (sx, sy) lies inside
    the frame."""
    S, bx = B << L, -(-W // B)
    out = []
    for bi in range(-(-H // B)):
        for bj in range(bx):
            x0, y0 = bj * B, bi * B
            ax, ay = x0 // S * S, y0 // S * S
            if x0 + B <= W and y0 + B <= H and ax + sx >= 0 and ax + S + sx <= W and ay + sy >= 0 and ay + S + sy <= H:
                out.append(bi * bx + bj)
    return out


def translation_pair(H, W, sx, sy, seed=SEED + 41):
    """cur[y][x] = ref[y + sy][x + sx] on uniform byte noise, any shift up to 64."""
    return bmo.shifted_pair(H, W, sx, sy, seed=seed, margin=64)


def recovered(records, sad, idx, sx, sy):
    """How many of the blocks idx came back with exactly (4 sx, 4 sy), reference 0 and SAD 0."""
    r = np.asarray(records).astype(np.int64)[idx]
    return int(((r[:, 4] == 4 * sx) & (r[:, 5] == 4 * sy) & (r[:, 6] == 0) & (np.asarray(sad)[idx] == 0)).sum())


# ---- the C ABI's refusals ----
def abi_cases():
    """(name, function name, arguments, expected status): every refusal the header lists, on pointers that are never dereferenced because
    validation comes before any launch."""
    import ctypes

    EINVAL, EWORKSPACE = -1, -3
    P = ctypes.c_void_p
    out = []
    good_p = dict(plane=0x1000, pitch=64, fmt=bmo.NV12, H=32, W=48, levels=2, pyramid=0x10000, nbytes=1 << 20)
    order_p = ("plane", "pitch", "fmt", "H", "W", "levels", "pyramid", "nbytes")
    bad_p = [("null plane", dict(plane=0)), ("null pyramid", dict(pyramid=0)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H = 8193", dict(H=8193)),
             ("W = 8193", dict(W=8193, pitch=8193)), ("levels = 0", dict(levels=0)), ("levels = 4", dict(levels=4)), ("format 5", dict(fmt=5)),
             ("format -1", dict(fmt=-1)), ("pitch below a row", dict(pitch=47)), ("P010 pitch below 2 W", dict(fmt=bmo.P010, pitch=94)),
             ("RGB8 pitch below 3 W", dict(fmt=bmo.RGB8, pitch=143)), ("I010 odd pitch", dict(fmt=bmo.I010, pitch=97)),
             ("P010 odd pointer", dict(fmt=bmo.P010, pitch=96, plane=0x1001)), ("pyramid not 16-byte aligned", dict(pyramid=0x10008)),
             ("pyramid_bytes one short", dict(nbytes=48 * 32 + 32 * 16 + 16 * 8 - 1))]
    for name, kw in bad_p:
        v = dict(good_p, **kw)
        out.append((name, "arseg_luma_pyramid_fwd", tuple(P(v[k]) if k in ("plane", "pyramid") else v[k] for k in order_p) + (P(0),), EINVAL))
    good_s = dict(cur=0x10000, ref=0x20000, H=32, W=48, levels=2, B=16, Rt=8, r=1, lam=2, intra=255, ref_index=0, records=0x3000, sad=0x4000, stats=0x5000,
                  ws=0x6000, ws_bytes=1 << 16)
    order_s = ("cur", "ref", "H", "W", "levels", "B", "Rt", "r", "lam", "intra", "ref_index", "records", "sad", "stats", "ws", "ws_bytes")
    bad_s = [("null cur", dict(cur=0)), ("null ref", dict(ref=0)), ("null records", dict(records=0)), ("null workspace", dict(ws=0)),
             ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H = 8193", dict(H=8193)), ("W = 8193", dict(W=8193)), ("levels = 0", dict(levels=0)),
             ("levels = 4", dict(levels=4)), ("B = 4", dict(B=4)), ("B = 12", dict(B=12)), ("B = 32", dict(B=32)), ("Rt = 0", dict(Rt=0)), ("Rt = 33", dict(Rt=33)),
             ("r = 0", dict(r=0)), ("r = 4", dict(r=4)), ("lambda = -1", dict(lam=-1)), ("lambda = 256", dict(lam=256)), ("intra = -1", dict(intra=-1)),
             ("intra = 256", dict(intra=256)), ("ref_index = -1", dict(ref_index=-1)), ("ref_index = 16", dict(ref_index=16)),
             ("cur not 16-byte aligned", dict(cur=0x10004)), ("ref not 16-byte aligned", dict(ref=0x20008)),
             ("workspace not 16-byte aligned", dict(ws=0x6008)), ("records not 16-byte aligned", dict(records=0x3008)),
             ("sad not 4-byte aligned", dict(sad=0x4002)), ("stats not 8-byte aligned", dict(stats=0x5004))]
    # 32 x 48, B = 16: level 1 is 16 x 24 = 1 x 2 blocks, level 2 is 8 x 12 = 1 block: 48 bytes
    short = [("workspace one byte short", dict(ws_bytes=47)), ("workspace of 0 bytes", dict(ws_bytes=0))]
    for name, kw, want in [(n, k, EINVAL) for n, k in bad_s] + [(n, k, EWORKSPACE) for n, k in short]:
        v = dict(good_s, **kw)
        out.append((name, "arseg_block_motion_pyr_fwd", tuple(P(v[k]) if k in ("cur", "ref", "records", "sad", "stats", "ws") else v[k] for k in order_s) + (P(0),),
                    want))
    return out
