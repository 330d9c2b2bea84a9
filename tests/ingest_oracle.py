"""fp64 oracle of the 8-bit frame ingest (include/arseg_hip.h, arseg_frame_ingest_fwd), written from its contract, numpy only.

Per output pixel: the taps of F.interpolate(..., (h, w), mode='bilinear', align_corners=True) -- the sampling POSITION is the ingest
kernels' (part of the contract): scale = (in - 1) / (out - 1) in float32, the float32-rounded product scale * dst picks the two taps, and the
weight of the second is the unrounded product minus the first tap's index, rounded to float32 once (what the kernels' contracted
`scale * dst - i0` = fma(scale, dst, -i0) gives; ATen's unfused form differs by half an ulp of the position); everything after it is float64 --, RGB in the 0-255 scale at each tap
(NV12: bilinear chroma at cx = x / 2, cy = y / 2 - 0.25 clamped to the plane, the matrix of the colour enum, clip to [0, 255], no rounding),
blend, (v / 255 - mean) / std."""
import numpy as np

LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb)
COLOURS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]     # enum arseg_colour order


def matrix(name, full_range):
    """(y0, M) with RGB = M @ (Y - y0, Cb - 128, Cr - 128), derived from (Kr, Kb) and the range's scales."""
    kr, kb = LUMA[name]
    kg = 1.0 - kr - kb
    ky, s, y0 = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    m = np.array([[ky, 0.0, 2.0 * (1.0 - kr) * s],
                  [ky, -2.0 * kb * (1.0 - kb) / kg * s, -2.0 * kr * (1.0 - kr) / kg * s],
                  [ky, 2.0 * (1.0 - kb) * s, 0.0]])
    return y0, m


def _lerp_axis(n, pos):
    """indices and weight of the second tap for float64 positions ``pos`` clamped to [0, n - 1]"""
    pos = np.clip(pos, 0.0, n - 1.0)
    i0 = np.floor(pos).astype(np.int64)
    i0 = np.minimum(i0, n - 1)
    return i0, np.minimum(i0 + 1, n - 1), pos - i0


def nv12_to_rgb(y, uv, name="bt709", full_range=False):
    """luma uint8 [..,H,W], chroma uint8 [..,H/2,W/2,2] -> float64 RGB [..,H,W,3] in the 0-255 scale at every luma pixel."""
    y, uv = np.asarray(y, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    H, W = y.shape[-2:]
    k0, k1, wy = _lerp_axis(H // 2, np.arange(H) / 2.0 - 0.25)
    j0, j1, wx = _lerp_axis(W // 2, np.arange(W) / 2.0)
    wy, wx = wy[:, None, None], wx[None, :, None]
    rows0, rows1 = uv[..., k0, :, :], uv[..., k1, :, :]
    c = (1 - wy) * ((1 - wx) * rows0[..., j0, :] + wx * rows0[..., j1, :]) + wy * ((1 - wx) * rows1[..., j0, :] + wx * rows1[..., j1, :])
    y0, m = matrix(name, full_range)
    v = np.stack([y - y0, c[..., 0] - 128.0, c[..., 1] - 128.0], axis=-1)
    return np.clip(v @ m.T, 0.0, 255.0)


def _src_f32(n_in, n_out):
    """align_corners=True taps and weight as the ingest kernels form them (module docstring)."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    dst = np.arange(n_out)
    src = (scale * dst.astype(np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    exact = np.float64(scale) * dst.astype(np.float64)                 # 24-bit x small integer: exact in float64
    lam = np.clip((exact - i0).astype(np.float32), 0, 1).astype(np.float64)
    return i0, i1, lam


def ingest(rgb255, h, w, mean, std):
    """float RGB [N,H,W,3] in the 0-255 scale -> float64 [N,h,w,3]: downscale (identity when (h,w) == (H,W)), then normalise."""
    rgb255 = np.asarray(rgb255, dtype=np.float64)
    N, H, W, _ = rgb255.shape
    if (h, w) != (H, W):
        y0, y1, ly = _src_f32(H, h)
        x0, x1, lx = _src_f32(W, w)
        ly, lx = ly[None, :, None, None], lx[None, None, :, None]
        top, bot = rgb255[:, y0], rgb255[:, y1]
        rgb255 = (1 - ly) * ((1 - lx) * top[:, :, x0] + lx * top[:, :, x1]) + ly * ((1 - lx) * bot[:, :, x0] + lx * bot[:, :, x1])
    return (rgb255 / 255.0 - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)


def ingest_nv12(y, uv, h, w, mean, std, name="bt709", full_range=False):
    return ingest(nv12_to_rgb(y, uv, name, full_range), h, w, mean, std)
