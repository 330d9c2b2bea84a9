"""numpy oracle of arseg_labels_rle_fwd / arseg_rle_decode_fwd (include/arseg_hip.h), written from the contract: uint8 planes in, row_start
and the run words out, and back, with the capacity rule.  Everything is an integer, so the GPU tests compare with it exactly.  Also the
seeded planes and the hand-made rows both test files use (tests/test_rle.py shows on the CPU that the seeded planes have few-run rows,
single-run rows and starts on and next to the 16-pixel pieces of the kernel)."""
import numpy as np

import consistency_oracle

GUARD_WORD = 0xA5A5A5A5


def encode(planes):
    """planes uint8 [N,H,W] -> (row_start int32 [N,H+1], [runs uint32 [row_start[n,H]]] per frame).  A run begins at x = 0 and wherever a
    byte differs from the one to its left; its word is (x_first << 8) | value."""
    planes = np.asarray(planes)
    assert planes.dtype == np.uint8 and planes.ndim == 3
    N, H, W = planes.shape
    row_start = np.zeros((N, H + 1), dtype=np.int32)
    runs = []
    for n in range(N):
        words = []
        for y in range(H):
            row = planes[n, y]
            first = np.flatnonzero(np.concatenate(([True], row[1:] != row[:-1])))
            words.append((first.astype(np.uint32) << 8) | row[first].astype(np.uint32))
            row_start[n, y + 1] = row_start[n, y] + len(first)
        runs.append(np.concatenate(words).astype(np.uint32))
    return row_start, runs


def decode(row_start, runs, H, W, prefill):
    """One frame: row_start [H+1] and the STORED words runs [cap] (cap may be below row_start[H]: an overflowed buffer) over a copy of
    ``prefill`` uint8 [H,W].  A stored run covers [x_first, the next run of its row or W); of a stored run whose successor in the row is
    not stored only the first pixel is known, and only that one is written; the pixels of runs that are not stored keep the prefill."""
    out = np.array(prefill, dtype=np.uint8, copy=True)
    assert out.shape == (H, W)
    cap = len(runs)
    for y in range(H):
        a, b = int(row_start[y]), int(row_start[y + 1])
        for i in range(a, min(b, cap)):
            x0, v = int(runs[i]) >> 8, int(runs[i]) & 0xFF
            if i + 1 >= b:
                x1 = W
            elif i + 1 < cap:
                x1 = int(runs[i + 1]) >> 8
            else:
                x1 = x0 + 1
            out[y, x0:x1] = v
    return out


# (name, seed, N, H, W, classes, h, w): blob-like planes -- consistency_oracle's low-resolution-noise scenes of h x w, argmax'ed at H x W and
# mapped to byte values that include 0 and 255.  Odd sizes that are no multiple of the 16-pixel piece; the second spans several pieces per
# row and several workgroups of rows.  (The scenes are coarse enough for some rows to be one run; seeds chosen so that tests/test_rle.py's
# spread conditions hold.)
CASES = [
    ("blobs-37x53", 101, 2, 37, 53, 6, 4, 6),
    ("blobs-72x88", 139, 3, 72, 88, 9, 6, 7),
]
CASE_IDS = [c[0] for c in CASES]


def build(case):
    """The seeded planes of a case: uint8 [N,H,W]."""
    _, seed, N, H, W, n_cls, h, w = case
    g = np.random.Generator(np.random.PCG64(seed))
    logits = consistency_oracle.make_logits(g, N, n_cls, h, w)
    labels = consistency_oracle.labels_f64(logits, H, W, True)
    values = np.concatenate(([0, 255], g.permutation(np.arange(1, 255))[:n_cls - 2])).astype(np.uint8)
    return np.ascontiguousarray(values[labels])


def blob_planes(seed, N, H, W, n_cls=19, cell=32):
    """Planes of any size from the same construction (scenes of about ``cell``-pixel features): the full-size test and the benchmark."""
    g = np.random.Generator(np.random.PCG64(seed))
    logits = consistency_oracle.make_logits(g, N, n_cls, max(3, H // cell), max(3, W // cell))
    return np.ascontiguousarray(consistency_oracle.labels_f64(logits, H, W, True).astype(np.uint8))


def _w(x, v):
    return (x << 8) | v


# Hand-made planes with the expected answer written out: (name, plane rows, row_start, words)
HAND = [
    ("constant", [[7] * 40], [0, 1], [_w(0, 7)]),
    ("alternating-0-255", [[0, 255] * 10], [0, 20],
     [_w(0, 0), _w(1, 255), _w(2, 0), _w(3, 255), _w(4, 0), _w(5, 255), _w(6, 0), _w(7, 255), _w(8, 0), _w(9, 255), _w(10, 0), _w(11, 255),
      _w(12, 0), _w(13, 255), _w(14, 0), _w(15, 255), _w(16, 0), _w(17, 255), _w(18, 0), _w(19, 255)]),
    ("boundary-at-16", [[3] * 16 + [9] * 24], [0, 2], [_w(0, 3), _w(16, 9)]),
    ("boundary-at-15", [[3] * 15 + [9] * 25], [0, 2], [_w(0, 3), _w(15, 9)]),
    ("boundary-at-17", [[3] * 17 + [9] * 23], [0, 2], [_w(0, 3), _w(17, 9)]),
    ("boundary-at-1024", [[1] * 1024 + [2] * 76], [0, 2], [_w(0, 1), 0x040002]),
    ("row-ends-as-the-next-begins", [[5, 5, 8, 8], [8, 8, 8, 2], [2, 2, 2, 2]], [0, 2, 4, 5], [_w(0, 5), _w(2, 8), _w(0, 8), _w(3, 2), _w(0, 2)]),
    ("single-pixel-255-then-0", [[255], [0]], [0, 1, 2], [255, 0]),
]
HAND_IDS = [h[0] for h in HAND]


def hand_plane(h):
    return np.array(h[1], dtype=np.uint8)[None]
