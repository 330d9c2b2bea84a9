"""numpy oracle of arseg_segment_consistency_fwd / arseg_labels_consistency_fwd (include/arseg_hip.h), written from the contract: a train-id
plane, the reference's train-id plane(s), mv_q and n_cls in, the change plane and the rows of statistics out.  Everything is an integer, so
the GPU tests compare with it exactly.  Also the seeded inputs both test files use (tests/test_consistency.py shows on the CPU that every
one of them exercises all four outcomes and every class)."""
import numpy as np
import torch
import torch.nn.functional as F

TC_NSTATS = 3 + 3 * 32
CUR, REF, INTER = 3, 35, 67
AGREE, DIFFER, NOT_COMPARED = 0, 255, 128

# (name, seed, N, n_cls, h, w, H, W, align_corners, shared reference plane): the shapes of tests/confidence_oracle.py -- the smallest at which
# each route can go wrong: same size; per-pixel bilinear; the run route at x2 / x4 / x8 on an odd-sized map narrower than a wave (first and
# last half-runs in play); 32 classes.  Shared (one keyframe plane for all frames) and per-frame reference planes alternate.
CASES = [
    ("same", 203, 2, 12, 24, 40, 24, 40, True, False),
    ("bilinear", 448, 2, 19, 17, 20, 136, 160, True, True),
    ("x2", 281, 3, 19, 9, 11, 18, 22, False, True),
    ("x4", 236, 3, 19, 9, 11, 36, 44, False, False),
    ("x8", 243, 3, 19, 9, 11, 72, 88, False, True),
    ("same-32", 251, 2, 32, 24, 40, 24, 40, True, True),
    ("x8-32", 262, 2, 32, 9, 11, 72, 88, False, False),
]
CASE_IDS = [c[0] for c in CASES]


def round_half_even_div4(v):
    """np.round(v / 4) of integers in integer arithmetic: v = 4 b + r (floor division); r < 2 -> b, r > 2 -> b + 1, r == 2 -> the even one."""
    v = np.asarray(v).astype(np.int64)
    b, r = v >> 2, v & 3
    return np.where(r < 2, b, np.where(r > 2, b + 1, b + (b & 1)))


def consistency(labels, ref, mv_q, n_cls, lut=None):
    """labels [N,H,W] integers (train ids; >= n_cls: void, plane form), ref uint8 [R,H,W] with R == 1 (shared) or N, mv_q int16 [N,H,W,2]
    -> (change uint8 [N,H,W], stats int64 [N,TC_NSTATS], labels8 uint8 [N,H,W] = lut[labels] or labels)."""
    labels, ref, mv_q = np.asarray(labels).astype(np.int64), np.asarray(ref), np.asarray(mv_q)
    N, H, W = labels.shape
    assert ref.dtype == np.uint8 and ref.shape[1:] == (H, W) and ref.shape[0] in (1, N)
    assert mv_q.dtype == np.int16 and mv_q.shape == (N, H, W, 2) and 1 <= n_cls <= 32
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    change = np.empty((N, H, W), dtype=np.uint8)
    stats = np.zeros((N, TC_NSTATS), dtype=np.int64)
    for n in range(N):
        tx, ty = xs + round_half_even_div4(mv_q[n, ..., 0]), ys + round_half_even_div4(mv_q[n, ..., 1])
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        r = np.full((H, W), 255, dtype=np.int64)
        r[inside] = ref[n if ref.shape[0] > 1 else 0][ty[inside], tx[inside]]
        k = labels[n]
        compared = inside & (r < n_cls) & (k < n_cls)
        agree = compared & (r == k)
        change[n] = np.where(compared, np.where(agree, AGREE, DIFFER), NOT_COMPARED)
        stats[n, 0], stats[n, 1], stats[n, 2] = compared.sum(), (~inside).sum(), (inside & ~compared).sum()
        stats[n, CUR:CUR + n_cls] = np.bincount(k[compared], minlength=n_cls)
        stats[n, REF:REF + n_cls] = np.bincount(r[compared], minlength=n_cls)
        stats[n, INTER:INTER + n_cls] = np.bincount(k[agree], minlength=n_cls)
    if lut is None:
        labels8 = labels.astype(np.uint8)
    else:
        labels8 = np.asarray(lut, dtype=np.uint8)[np.minimum(labels, n_cls - 1)]
    return change, stats, labels8


def tc_rows(stats, n_cls):
    """(agreement, tc_miou, compared_share) per row, from the two formulas of the contract, in plain Python."""
    out = []
    for row in np.asarray(stats):
        compared, total = int(row[0]), int(row[0] + row[1] + row[2])
        ious = []
        for k in range(n_cls):
            union = int(row[CUR + k] + row[REF + k] - row[INTER + k])
            if union > 0:
                ious.append(int(row[INTER + k]) / union)
        out.append((sum(int(row[INTER + k]) for k in range(n_cls)) / compared if compared else float("nan"),
                    sum(ious) / len(ious) if ious else float("nan"), compared / total if total else float("nan")))
    return out


def labels_f64(logits, H, W, align_corners):
    """The float64 argmax of the logits resized to H x W: the labels the CPU spread check uses (the GPU tests feed the oracle the tail's pred)."""
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32)).double()
    if tuple(x.shape[-2:]) != (H, W):
        x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align_corners))
    return x.argmax(dim=1).numpy()


def make_logits(g, N, n_cls, h, w):
    """Blob-like fp32 logits with |x| <= 8: low-resolution noise (about half the map's size, one scene for the N frames plus a little
    noise per frame, every class with a home cell of its own where there are enough cells) resized up, so that the classes form regions."""
    gh, gw = max(2, (h + 1) // 2), max(2, (w + 1) // 2)
    base = g.standard_normal((n_cls, gh, gw))
    if gh * gw >= n_cls:
        cells = g.permutation(gh * gw)[:n_cls]
        for k in range(n_cls):
            base[k].reshape(-1)[cells[k]] += 2.5
    noise = base[None] + 0.3 * g.standard_normal((N, n_cls, gh, gw))
    x = F.interpolate(torch.from_numpy(noise), size=(h, w), mode="bilinear", align_corners=True).numpy()
    return np.clip(3.0 * x, -8.0, 8.0).astype(np.float32)


def build(case):
    """The seeded input of a case -> dict(logits fp32 [N,n_cls,h,w], ref uint8 [R,H,W], mv int16 [N,H,W,2], labels int64 [N,H,W] = labels_f64).
    The reference plane is the scene displaced by a block-constant field (a forward scatter: collisions and holes are natural disagreements);
    mv_q points back (4 d plus a quarter-pel jitter that rounds away), except in a seeded fifth of the blocks, where it is off by 1.5 .. 3.5
    pixels (halves: the rounding rule is in play); the vectors of a border band point off the frame; three rectangles of the reference are 255."""
    _, seed, N, n_cls, h, w, H, W, align, shared = case
    g = np.random.Generator(np.random.PCG64(seed))
    logits = make_logits(g, N, n_cls, h, w)
    labels = labels_f64(logits, H, W, align)
    bs = max(2, min(H, W) // 6)
    by, bx = (H + bs - 1) // bs, (W + bs - 1) // bs
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    R = 1 if shared else N
    ref = np.empty((R, H, W), dtype=np.uint8)
    mv = np.empty((N, H, W, 2), dtype=np.int16)
    fields = []
    for n in range(N):
        if n < R:
            blocks = g.integers(-2, 3, (by, bx, 2))
            d = blocks[ys // bs, xs // bs]                      # [H,W,2] (dx, dy) in pixels
            fields.append(d)
            src = labels[n]
            plane = src.copy()
            tx, ty = xs + d[..., 0], ys + d[..., 1]
            ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            plane[ty[ok], tx[ok]] = src[ok]
            rh, rw = max(2, H // 8), max(2, W // 8)
            for _ in range(3):
                y0, x0 = int(g.integers(2, H - rh - 1)), int(g.integers(2, W - rw - 1))
                plane[y0:y0 + rh, x0:x0 + rw] = 255
            ref[n] = plane.astype(np.uint8)
        d = fields[n if n < R else 0]
        q = 4 * d + g.integers(-1, 2, (H, W, 2))
        wrong = g.random((by, bx)) < 0.2
        off = g.choice(np.array([-14, -10, -6, 6, 10, 14]), (by, bx, 2))
        q = np.where(wrong[ys // bs, xs // bs][..., None], 4 * d + off[ys // bs, xs // bs], q)
        bw = max(1, min(H, W) // 16)
        extra = g.integers(0, 8, (H, W, 2))
        q[..., 0] = np.where(xs < bw, -4 * (xs + 1) - extra[..., 0], np.where(xs >= W - bw, 4 * (W - xs) + extra[..., 0], q[..., 0]))
        q[..., 1] = np.where(ys < bw, -4 * (ys + 1) - extra[..., 1], np.where(ys >= H - bw, 4 * (H - ys) + extra[..., 1], q[..., 1]))
        mv[n] = q.astype(np.int16)
    return {"logits": logits, "ref": ref, "mv": mv, "labels": labels}


def spread(case):
    """Per frame of a case, on the float64 labels: (agree / compared, differ / HW, outside / HW, void / HW, min over classes of cur, ref, inter)."""
    b = build(case)
    n_cls, H, W = case[3], case[6], case[7]
    _, stats, _ = consistency(b["labels"], b["ref"], b["mv"], n_cls)
    rows = []
    for s in stats:
        agree = int(s[INTER:INTER + n_cls].sum())
        rows.append((agree / int(s[0]), (int(s[0]) - agree) / (H * W), int(s[1]) / (H * W), int(s[2]) / (H * W),
                     int(min(s[CUR:CUR + n_cls].min(), s[REF:REF + n_cls].min(), s[INTER:INTER + n_cls].min()))))
    return rows
