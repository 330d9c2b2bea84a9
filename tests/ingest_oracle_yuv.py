"""fp64 oracle of the planar 4:2:0 / 10-bit frame ingest (include/arseg_hip.h, arseg_frame_ingest_yuv_fwd), written from its contract, numpy
only; everything the 8-bit contract already fixes (matrices, chroma siting, the downscale's taps, the normalisation) is tests/ingest_oracle.py.

Per format the stored samples become codes -- I420: the byte; P010: word >> 6; I010: word & 0x3ff -- of depth n = 8 / 10 / 10.  Chroma is
interpolated on the codes (cx = x / 2, cy = y / 2 - 0.25, clamped to the plane), then with f = 2^-(n-8) (limited range) or 255 / (2^n - 1)
(full range): Y8 = code_Y f, C8 - 128 = (C - 2^(n-1)) f, the matrix of the colour enum, clip to [0, 255], no rounding."""
import numpy as np

import ingest_oracle as base

FORMATS = ("i420", "p010", "i010")
DEPTH = {"i420": 8, "p010": 10, "i010": 10}


def codes(fmt, planes):
    """The stored planes of one format -> (Y [..,H,W], Cb [..,H/2,W/2], Cr [..,H/2,W/2]) integer codes."""
    if fmt == "i420":
        y, u, v = (np.asarray(p).astype(np.int64) for p in planes)
        assert max(y.max(), u.max(), v.max()) <= 255
    elif fmt == "i010":
        y, u, v = (np.asarray(p).astype(np.int64) & 0x3FF for p in planes)
    elif fmt == "p010":
        y, uv = (np.asarray(p).astype(np.int64) >> 6 for p in planes)
        u, v = uv[..., 0], uv[..., 1]
    else:
        raise ValueError(fmt)
    return y, u, v


def code_scale(n, full_range):
    return 255.0 / (2.0 ** n - 1.0) if full_range else 2.0 ** -(n - 8)


def yuv_to_rgb(fmt, planes, name="bt709", full_range=False):
    """-> float64 RGB [..,H,W,3] in the 0-255 scale at every luma pixel."""
    y, u, v = (c.astype(np.float64) for c in codes(fmt, planes))
    n = DEPTH[fmt]
    H, W = y.shape[-2:]
    k0, k1, wy = base._lerp_axis(H // 2, np.arange(H) / 2.0 - 0.25)
    j0, j1, wx = base._lerp_axis(W // 2, np.arange(W) / 2.0)
    wy, wx = wy[:, None], wx[None, :]

    def sample(c):
        r0, r1 = c[..., k0, :], c[..., k1, :]
        return (1 - wy) * ((1 - wx) * r0[..., j0] + wx * r0[..., j1]) + wy * ((1 - wx) * r1[..., j0] + wx * r1[..., j1])

    f, mid = code_scale(n, full_range), 2.0 ** (n - 1)
    y0, m = base.matrix(name, full_range)
    vec = np.stack([y * f - y0, (sample(u) - mid) * f, (sample(v) - mid) * f], axis=-1)
    return np.clip(vec @ m.T, 0.0, 255.0)


def ingest_yuv(fmt, planes, h, w, mean, std, name="bt709", full_range=False):
    return base.ingest(yuv_to_rgb(fmt, planes, name, full_range), h, w, mean, std)
