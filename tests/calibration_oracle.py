"""Direct-definition oracle of arseg_calibration_fwd (include/arseg_hip.h): a loop over the pixels, the code of each from
tests/confidence_oracle.py (exact / codes: float64 resize and softmax), its class from a float64 argmax written out (the first maximum wins,
a NaN counts as the maximum), the label rule of the evaluator tail.  Also the literal hand cases with their tables written out, the seeded
labels both test files use, and the torch composition of the confidence launch's planes the GPU tests hold the kernel to."""
import numpy as np
import torch
import torch.nn.functional as F

import confidence_oracle as oracle


def classes(logits, H, W, align_corners):
    """fp32 logits [N,n_cls,h,w] -> k* int64 [N,H,W] by the definition, in float64."""
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32)).double()
    if tuple(x.shape[-2:]) != (H, W):
        x = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=bool(align_corners))
    x = x.numpy()
    N, n_cls = x.shape[:2]
    out = np.zeros((N, H, W), np.int64)
    for n in range(N):
        for y in range(H):
            for c in range(W):
                best, bi = -np.inf, 0
                for k in range(n_cls):
                    v = x[n, k, y, c]
                    if v != v:
                        bi = k
                        break
                    if v > best:
                        best, bi = v, k
                out[n, y, c] = bi
    return out


def table(logits, label, H, W, n_cls, groups=None, n_groups=1, ignore_label=255, kind="top1", align_corners=True):
    """int64 [n_groups, n_cls, 256, 2] by the definition: one pixel at a time."""
    logits = np.asarray(logits, dtype=np.float32)
    label = np.asarray(label)
    q = oracle.codes(oracle.exact(logits, H, W, align_corners, kind))
    k = classes(logits, H, W, align_corners)
    N = logits.shape[0]
    ids = [0] * N if groups is None else list(groups)
    out = np.zeros((n_groups, n_cls, 256, 2), np.int64)
    for n in range(N):
        g = int(ids[n])
        if not 0 <= g < n_groups:
            continue
        for y in range(H):
            for c in range(W):
                lab = int(label[n, y, c])
                if lab < 0 or lab >= n_cls or lab == ignore_label:
                    continue
                out[g, k[n, y, c], q[n, y, c], 0] += 1
                if lab == k[n, y, c]:
                    out[g, k[n, y, c], q[n, y, c], 1] += 1
    return out


def sparse(entries, n_groups, n_cls):
    """{(g, k, q): (pixels, right)} -> the dense table."""
    out = np.zeros((n_groups, n_cls, 256, 2), np.int64)
    for (g, k, q), (n, r) in entries.items():
        out[g, k, q] = (n, r)
    return out


# Hand cases: same-size frames of one row, so a pixel's values are its logits.  Two classes with logits (a, 0): p1 = 1 / (1 + e^-a).
#   a = ln 3 -> p = (3/4, 1/4): top1 code floor(191.25 + 0.5) = 191
#   a = ln 4 -> p = (4/5, 1/5): top1 code floor(204 + 0.5) = 204, margin code floor(153 + 0.5) = 153
#   a = 0    -> a tie: class 0 (the first maximum), top1 code floor(127.5 + 0.5) = 128, margin code 0
#   a = 40   -> p1 = 1 to every bit: 255 either way
# Three classes (0, 0, ln 6) -> p = (1/8, 1/8, 3/4): class 2, top1 code 191, margin code floor(159.375 + 0.5) = 159
# (every 255 c above is an integer, a quarter or 3/8 off one: the fp32 rounding of the logarithms moves no code)
LN3, LN4, LN6 = float(np.log(3.0)), float(np.log(4.0)), float(np.log(6.0))


def _px(*pixels):
    """pixels, each a tuple of class logits -> logits [1, n_cls, 1, len(pixels)]"""
    return np.array(pixels, np.float32).T[None, :, None, :]


# (name, logits [N,n_cls,1,W], labels [N,1,W], groups, n_groups, kind, {(g, k, q): (pixels, right)})
HAND = [
    ("one-pixel", _px((LN3, 0)), [[[0]]], None, 1, "top1", {(0, 0, 191): (1, 1)}),
    ("ignored-pixel", _px((LN3, 0), (LN3, 0)), [[[255, 0]]], None, 1, "top1", {(0, 0, 191): (1, 1)}),
    ("labels-below-and-above", _px((LN3, 0), (LN3, 0), (0, LN3)), [[[-1, 2, 1]]], None, 1, "top1", {(0, 1, 191): (1, 1)}),
    ("wrong-pixel", _px((LN3, 0), (LN3, 0), (40, 0)), [[[1, 0, 1]]], None, 1, "top1", {(0, 0, 191): (2, 1), (0, 0, 255): (1, 0)}),
    ("two-groups", np.concatenate([_px((LN3, 0), (0, 40)), _px((LN3, 0), (0, 40)), _px((0, 0), (0, 0))]), [[[0, 1]], [[1, 1]], [[0, 1]]],
     [1, 0, 1], 2, "top1", {(0, 0, 191): (1, 0), (0, 1, 255): (1, 1), (1, 0, 191): (1, 1), (1, 1, 255): (1, 1), (1, 0, 128): (2, 1)}),
    ("group-out-of-range", np.concatenate([_px((LN3, 0)), _px((LN3, 0)), _px((0, LN3))]), [[[0]], [[0]], [[1]]], [2, -1, 1], 2, "top1",
     {(1, 1, 191): (1, 1)}),
    ("nan-pixel", _px((0, np.nan, 5), (0, 0, LN6), (np.inf, 0, 0), (-np.inf, -np.inf, -np.inf)), [[[1, 2, 0, 0]]], None, 1, "top1",
     {(0, 1, 0): (1, 1), (0, 2, 191): (1, 1), (0, 0, 0): (2, 2)}),
    ("one-class", _px((-3.0,), (7.0,), (0.0,)), [[[0, 1, 0]]], None, 1, "top1", {(0, 0, 255): (2, 2)}),
    ("margin-vs-top1/top1", _px((LN4, 0), (0, 0), (40, 0)), [[[0, 1, 0]]], None, 1, "top1",
     {(0, 0, 204): (1, 1), (0, 0, 128): (1, 0), (0, 0, 255): (1, 1)}),
    ("margin-vs-top1/margin", _px((LN4, 0), (0, 0), (40, 0)), [[[0, 1, 0]]], None, 1, "margin",
     {(0, 0, 153): (1, 1), (0, 0, 0): (1, 0), (0, 0, 255): (1, 1)}),
    ("three-classes-margin", _px((0, 0, LN6)), [[[2]]], None, 1, "margin", {(0, 2, 159): (1, 1)}),
]
HAND_IDS = [h[0] for h in HAND]


def case_labels(case):
    """The seeded labels of a confidence_oracle case: the float64 reference prediction on 60 % of the pixels, a random class elsewhere, and
    a few labels that do not count (n_cls + 3, -1, 255)."""
    _, seed, N, n_cls, h, w, H, W, align = case
    k = classes(oracle.case_logits(case), H, W, align)
    g = np.random.Generator(np.random.PCG64(seed + 1000))
    r = g.random((N, H, W))
    lab = np.where(r < 0.6, k, g.integers(0, n_cls, (N, H, W))).astype(np.int64)
    lab[(r > 0.93) & (r <= 0.95)] = n_cls + 3
    lab[(r > 0.92) & (r <= 0.93)] = -1
    lab[r > 0.95] = 255
    return lab


def case_groups(case):
    return [1, 0, 1] if case[2] == 3 else [0, 1]


def from_planes(conf, labels8, label, groups, n_groups, n_cls, ignore_label=255):
    """The parent's composition, in torch on whatever device the planes are on: the confidence launch's conf8 and labels8 (identity lut)
    and the int64 labels -> the table by one bincount on the key (group, k, q, right)."""
    N = conf.shape[0]
    g = torch.as_tensor([0] * N if groups is None else list(groups), dtype=torch.int64, device=conf.device).reshape(N, 1, 1)
    k, q = labels8.long(), conf.long()
    counting = (label >= 0) & (label < n_cls) & (label != ignore_label) & (g >= 0) & (g < n_groups)
    key = ((g * n_cls + k) * 256 + q) * 2
    total = torch.bincount(key[counting], minlength=n_groups * n_cls * 512)
    right = torch.bincount(key[counting & (label == k)] + 1, minlength=n_groups * n_cls * 512)
    return (total + right).reshape(n_groups, n_cls, 256, 2)
