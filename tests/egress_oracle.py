"""numpy restatement of the overlay arithmetic of arseg_segment_egress_fwd (include/arseg_hip.h), written from the contract alone:

    RGB8, per channel c:     dst = (src (256 - a_k) + P[k][c] a_k + 128) >> 8
    4:2:0 luma, per pixel:   Y'  = (Y (256 - a_k) + P[k][0] a_k + 128) >> 8
    4:2:0 chroma, per sample over the four luma pixels i of its 2x2 block:  A = sum a_{k_i},
                             C'  = (C (1024 - A) + sum a_{k_i} P[k_i][c] + 512) >> 10

No torch, no arseg_amd import.  Plus a few adversarial label maps."""
import numpy as np


def paint(labels, planes, fmt, codes, weights):
    """labels int [N,H,W]; planes: the source planes as numpy uint8 -- "rgb8": ([N,H,W,3],), "nv12": (Y [N,H,W], CbCr [N,H/2,W/2,2]),
    "i420": (Y, Cb [N,H/2,W/2], Cr); codes uint8 [n_cls,3] in the destination's space; weights n_cls integers 0..256.  -> the painted planes."""
    k = np.asarray(labels).astype(np.int64)
    P = np.asarray(codes).astype(np.int64)
    a = np.asarray(weights).astype(np.int64)
    assert k.ndim == 3 and P.ndim == 2 and P.shape[1] == 3 and a.shape == (P.shape[0],) and a.min() >= 0 and a.max() <= 256
    ak = a[k]                                                     # [N,H,W]
    if fmt == "rgb8":
        (src,) = planes
        out = (src.astype(np.int64) * (256 - ak)[..., None] + P[k] * ak[..., None] + 128) >> 8
        return (out.astype(np.uint8),)
    N, H, W = k.shape
    assert H % 2 == 0 and W % 2 == 0
    y = (planes[0].astype(np.int64) * (256 - ak) + P[k, 0] * ak + 128) >> 8
    blocks = lambda v: v.reshape(N, H // 2, 2, W // 2, 2).sum(axis=(2, 4))
    A = blocks(ak)
    chroma = lambda c, ch: ((c.astype(np.int64) * (1024 - A) + blocks(ak * P[k, ch]) + 512) >> 10).astype(np.uint8)
    if fmt == "nv12":
        uv = planes[1]
        return y.astype(np.uint8), np.stack([chroma(uv[..., 0], 1), chroma(uv[..., 1], 2)], axis=-1)
    if fmt == "i420":
        return y.astype(np.uint8), chroma(planes[1], 1), chroma(planes[2], 2)
    raise ValueError(fmt)


def adversarial_labels(H=8, W=12):
    """(name, labels int64 [1,H,W], n_cls, weights) -- label maps that stress the chroma mixing and the weight extremes."""
    yy, xx = np.mgrid[0:H, 0:W]
    half = np.full(32, 128, dtype=np.int64)
    return [
        ("single class", np.full((1, H, W), 3, dtype=np.int64), 5, half[:5]),
        ("checkerboard", ((yy + xx) % 2)[None].astype(np.int64), 2, np.array([64, 200])),
        ("weight 0 next to 256", (xx % 2)[None].astype(np.int64), 2, np.array([0, 256])),
        ("all 32 classes", ((yy * W + xx) % 32)[None].astype(np.int64), 32, (np.arange(32) * 8 + 8).astype(np.int64)),
    ]
