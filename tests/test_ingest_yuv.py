"""CPU-side checks of the planar 4:2:0 / 10-bit frame ingest (I420, P010, I010 decoder frames into the fast paths): the entry point is
declared, bound and exported and refuses every bad argument before it launches anything, ``ingest.DecodedFrames.i420 / p010 / i010`` validate
what they are given, ``ingest.rgb_to_yuv420`` agrees with ``rgb_to_nv12`` and inverts the fp64 oracle (tests/ingest_oracle_yuv.py) within the
quantisation of each depth, and the oracle reduces to the NV12 oracle where the formats hold the same picture."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ingest_oracle as oracle
import ingest_oracle_yuv as yuv
from conftest import ROOT

MEAN, STD = (0.39068785, 0.40521392, 0.41434407), (0.29652068, 0.30514979, 0.30080369)


def test_entry_point_declared_bound_and_exported():
    from arseg_amd import _lib

    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    lib = _lib.load()
    assert "arseg_frame_ingest_yuv_fwd(" in header
    assert "arseg_frame_ingest_yuv_fwd" in _lib.PROTOTYPES
    assert hasattr(lib, "arseg_frame_ingest_yuv_fwd")
    for name, value in (("ARSEG_SRC_I420", 2), ("ARSEG_SRC_P010", 3), ("ARSEG_SRC_I010", 4)):
        assert f"{name} = {value}" in header
    assert (_lib.SRC_I420, _lib.SRC_P010, _lib.SRC_I010) == (2, 3, 4)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5                   # a backward-compatible addition
    assert "ingest.hip" in open(os.path.join(ROOT, "ar-seg_amd", "csrc", "Makefile")).read()


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from arseg_amd import _lib

    lib = _lib.load()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)          # (never dereferenced: validation returns first)
    odd = ctypes.c_void_p((1 << 20) + 1)
    f3, z3 = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.3, 0.0, 0.3)
    I420, P010, I010, BT = _lib.SRC_I420, _lib.SRC_P010, _lib.SRC_I010, _lib.COLOUR_BT709_LIMITED
    H, W = 16, 32
    rows = {I420: (W, W // 2, W // 2), P010: (2 * W, 2 * W, 0), I010: (2 * W, W, W)}          # bytes of a row of each plane

    def call(fmt, p0=fake, p1=fake, p2=fake, pitch=(None, None, None), ns=(None, None, None), colour=BT, out=fake, dt=_lib.DT_BF16, N=2, H=H, W=W,
             h=8, w=16, mean=f3, std=f3):
        pitch = [rows.get(fmt, rows[I420])[i] if v is None else v for i, v in enumerate(pitch)]
        ns = [pitch[i] * (H if i == 0 else H // 2) if v is None else v for i, v in enumerate(ns)]
        return lib.arseg_frame_ingest_yuv_fwd(p0, p1, p2, fmt, pitch[0], pitch[1], pitch[2], ns[0], ns[1], ns[2], colour, out, dt, N, H, W, h, w,
                                              mean, std, null)

    E = _lib.ARSEG_EINVAL

    def three(i, v):
        t = [None, None, None]
        t[i] = v
        return tuple(t)

    for fmt in (I420, P010, I010):
        planar = fmt != P010
        assert call(fmt, p0=null) == E and call(fmt, p1=null) == E and call(fmt, out=null) == E                       # null pointers
        if planar:
            assert call(fmt, p2=null) == E
        assert call(fmt, mean=None) == E and call(fmt, std=None) == E
        assert call(fmt, N=0) == E and call(fmt, H=0) == E and call(fmt, W=-2) == E and call(fmt, h=0) == E and call(fmt, w=-1) == E
        assert call(fmt, H=15) == E and call(fmt, W=31) == E                                                          # odd H / W
        for i in range(3 if planar else 2):                                                                          # pitch smaller than a row
            assert call(fmt, pitch=three(i, rows[fmt][i] - 2)) == E, (fmt, i)
            assert call(fmt, ns=three(i, -4)) == E, (fmt, i)                                                         # negative image stride
        assert call(fmt, std=z3) == E                                                                                 # zero std
        assert call(fmt, colour=4) == E and call(fmt, colour=-1) == E and call(fmt, dt=3) == E and call(fmt, dt=-1) == E
        assert call(fmt, out=ctypes.c_void_p((1 << 20) + 8)) == E                                                     # 16-byte stores
    for fmt in (P010, I010):                                                                                          # 16-bit planes: even everything
        assert call(fmt, p0=odd) == E and call(fmt, p1=odd) == E
        assert call(fmt, pitch=three(0, 2 * W + 1)) == E and call(fmt, pitch=three(1, 2 * W + 1)) == E
        assert call(fmt, ns=three(0, 2 * W * H + 1)) == E and call(fmt, ns=three(1, 2 * W * H + 1)) == E
    assert call(I010, p2=odd) == E and call(I010, pitch=three(2, W + 1)) == E and call(I010, ns=three(2, W * H + 1)) == E
    for fmt in (_lib.SRC_RGB8, _lib.SRC_NV12, 5, -1):                    # RGB8 / NV12 keep their own entry point
        assert call(fmt) == E


def test_decoded_frames_shape_views_indexing_equal():
    from arseg_amd import _lib, ingest

    D = ingest.DecodedFrames
    y, u, v = torch.zeros((3, 8, 16), dtype=torch.uint8), torch.full((3, 4, 8), 128, dtype=torch.uint8), torch.full((3, 4, 8), 128, dtype=torch.uint8)
    d = D.i420(y, u, v, MEAN, STD, matrix="bt601", full_range=True)
    assert d.shape == (3, 3, 8, 16) and len(d) == 3 and d.src_format == _lib.SRC_I420 and d.colour == _lib.COLOUR_BT601_FULL and not d.is_cuda
    assert len(d.planes) == 3 and all(a.data_ptr() == b.data_ptr() for a, b in zip(d.planes, (y, u, v)))
    assert D.i420(y, u, v).colour == _lib.COLOUR_BT709_LIMITED
    assert D.i420(y[0], u[0], v[0]).shape == (1, 3, 8, 16)                                   # one frame
    assert D.i420(np.zeros((8, 16), np.uint8), np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8)).shape == (1, 3, 8, 16)
    assert d[1].shape == (1, 3, 8, 16) and d[1:3].shape == (2, 3, 8, 16) and d[-1].shape == (1, 3, 8, 16)
    assert [tuple(p.shape) for p in d[1:3].planes] == [(2, 8, 16), (2, 4, 8), (2, 4, 8)]
    assert d.equal(D.i420(y.clone(), u.clone(), v.clone(), MEAN, STD, matrix="bt601", full_range=True))
    assert not d.equal(D.i420(y, u, v, MEAN, STD, matrix="bt709", full_range=True))
    assert not d.equal(D.i420(y, u, v + 1, MEAN, STD, matrix="bt601", full_range=True))
    py, pu = torch.zeros((2, 8, 24), dtype=torch.uint8)[:, :, :16], torch.zeros((2, 4, 12), dtype=torch.uint8)[:, :, :8]      # row pitches are kept as views
    dp = D.i420(py, pu, pu)
    assert dp.planes[0].data_ptr() == py.data_ptr() and dp.planes[1].data_ptr() == pu.data_ptr() and dp.planes[0].stride() == (192, 24, 1)

    y16, uv16 = torch.zeros((2, 8, 16), dtype=torch.uint16), torch.zeros((2, 4, 8, 2), dtype=torch.uint16)
    u16 = torch.zeros((2, 4, 8), dtype=torch.uint16)
    p = D.p010(y16, uv16, MEAN, STD, matrix="bt709", full_range=True)
    assert p.shape == (2, 3, 8, 16) and p.src_format == _lib.SRC_P010 and p.colour == _lib.COLOUR_BT709_FULL and len(p.planes) == 2
    assert p.planes[0].data_ptr() == y16.data_ptr() and p.planes[1].data_ptr() == uv16.data_ptr() and p.planes[0].dtype == torch.uint16
    assert D.p010(y16[0], uv16[0]).shape == (1, 3, 8, 16) and p[1].shape == (1, 3, 8, 16) and tuple(p[0:2].planes[1].shape) == (2, 4, 8, 2)
    assert D.p010(np.zeros((8, 16), np.uint16), np.zeros((4, 8, 2), np.uint16)).planes[0].dtype == torch.uint16
    assert p.equal(D.p010(y16.clone(), uv16.clone(), MEAN, STD, matrix="bt709", full_range=True)) and not p.equal(D.p010(y16, uv16, MEAN, STD))
    i = D.i010(y16, u16, u16, MEAN, STD)
    assert i.shape == (2, 3, 8, 16) and i.src_format == _lib.SRC_I010 and len(i.planes) == 3 and i.planes[1].dtype == torch.uint16
    assert i.equal(D.i010(y16.clone(), u16.clone(), u16.clone(), MEAN, STD)) and not i.equal(p)
    wide = torch.zeros((2, 8, 24), dtype=torch.uint16)[:, :, :16]
    assert D.i010(wide, u16, u16).planes[0].data_ptr() == wide.data_ptr()

    # int16 is the same bit pattern: 0xffc0 (code 1023 << 6) as int16 is -64
    s = torch.full((1, 8, 16), -64, dtype=torch.int16)
    suv = torch.full((1, 4, 8, 2), -32768, dtype=torch.int16)
    ps = D.p010(s, suv)
    assert ps.planes[0].dtype == torch.uint16 and ps.planes[0].data_ptr() == s.data_ptr()
    assert ps.planes[0].numpy().max() == 0xFFC0 and ps.planes[1].numpy().min() == 0x8000
    assert ps.equal(D.p010(torch.from_numpy(np.full((1, 8, 16), 0xFFC0, np.uint16)), torch.from_numpy(np.full((1, 4, 8, 2), 0x8000, np.uint16))))
    assert D.i010(s, suv[..., 0], suv[..., 1]).planes[2].dtype == torch.uint16


def test_decoded_frames_validation():
    from arseg_amd import _lib, ingest

    D = ingest.DecodedFrames
    y, u = torch.zeros((2, 8, 16), dtype=torch.uint8), torch.zeros((2, 4, 8), dtype=torch.uint8)
    y16, u16, uv16 = torch.zeros((2, 8, 16), dtype=torch.uint16), torch.zeros((2, 4, 8), dtype=torch.uint16), torch.zeros((2, 4, 8, 2), dtype=torch.uint16)
    with pytest.raises(ValueError, match="uint8"):
        D.i420(y, u, u.to(torch.int16))
    with pytest.raises(ValueError, match="uint8"):
        D.i420(y16, u, u)
    for bad in (torch.uint8, torch.int32, torch.float16, torch.float32):
        with pytest.raises(ValueError, match="uint16"):
            D.p010(torch.zeros((2, 8, 16), dtype=bad), uv16)
        with pytest.raises(ValueError, match="uint16"):
            D.i010(y16, u16, torch.zeros((2, 4, 8), dtype=bad))
    with pytest.raises(ValueError, match="uint16"):
        D.p010(np.zeros((8, 16), np.uint8), np.zeros((4, 8, 2), np.uint16))
    for ctor, lum, rest in ((D.i420, torch.uint8, (u, u)), (D.i010, torch.uint16, (u16, u16)), (D.p010, torch.uint16, (uv16,))):
        with pytest.raises(ValueError, match="even"):
            ctor(torch.zeros((2, 7, 16), dtype=lum), *rest)
        with pytest.raises(ValueError, match="even"):
            ctor(torch.zeros((2, 8, 15), dtype=lum), *rest)
        with pytest.raises(ValueError, match="bt601"):
            ctor(torch.zeros((2, 8, 16), dtype=lum), *rest, matrix="bt2020")
        with pytest.raises(ValueError, match="zero std"):
            ctor(torch.zeros((2, 8, 16), dtype=lum), *rest, MEAN, (0.3, 0.0, 0.3))
        with pytest.raises(ValueError, match="expects luma"):
            ctor(torch.zeros((2, 8, 16, 1), dtype=lum), *rest)
    with pytest.raises(ValueError, match="Cb plane"):
        D.i420(y, torch.zeros((2, 8, 8), dtype=torch.uint8), u)
    with pytest.raises(ValueError, match="Cr plane"):
        D.i420(y, u, torch.zeros((1, 4, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="Cr plane"):
        D.i010(y16, u16, torch.zeros((2, 4, 4), dtype=torch.uint16))
    with pytest.raises(ValueError, match="chroma plane"):
        D.p010(y16, torch.zeros((2, 4, 4, 2), dtype=torch.uint16))
    with pytest.raises(ValueError, match="chroma plane"):
        D.p010(y16, u16)                                                   # planar chroma handed to P010
    with pytest.raises(ValueError, match="one device"):
        D.i420(y, u, torch.zeros((2, 4, 8), dtype=torch.uint8, device="meta"))
    with pytest.raises(ValueError, match="one device"):
        D.i010(y16, torch.zeros((2, 4, 8), dtype=torch.uint16, device="meta"), u16)
    with pytest.raises(ValueError, match="one device"):
        D.p010(y16, torch.zeros((2, 4, 8, 2), dtype=torch.uint16, device="meta"))
    for d in (D.i420(y, u, u), D.p010(y16, uv16), D.i010(y16, u16, u16)):          # no CPU fallback: the kernel is the only route
        with pytest.raises(_lib.ArsegError, match="GPU only"):
            d.to_input(4, 8, torch.float32)
    with pytest.raises(ValueError, match="layout"):
        ingest.rgb_to_yuv420(np.zeros((8, 8, 3), np.uint8), "yv12")
    for layout in ("nv12", "i420", "p010", "i010"):
        with pytest.raises(ValueError):
            ingest.rgb_to_yuv420(np.zeros((7, 8, 3), np.uint8), layout)
        with pytest.raises(ValueError):
            ingest.rgb_to_yuv420(np.zeros((8, 8, 3), np.float32), layout)
        with pytest.raises(ValueError):
            ingest.rgb_to_yuv420(np.zeros((8, 8, 3), np.uint8), layout, matrix="bt2020")


@pytest.mark.parametrize("name,full", oracle.COLOURS)
def test_rgb_to_yuv420_layouts_agree(name, full):
    """The 8-bit layouts hold exactly rgb_to_nv12's samples; I010 is P010 >> 6 with the chroma de-interleaved; 10-bit codes use the low bits
    (they are not 4 x the 8-bit codes) and stay in the nominal range."""
    from arseg_amd import ingest

    g = np.random.Generator(np.random.PCG64(11))
    rgb = g.integers(0, 256, (2, 12, 20, 3), dtype=np.uint8)
    y, uv = ingest.rgb_to_nv12(rgb, name, full)
    ny, nuv = ingest.rgb_to_yuv420(rgb, "nv12", name, full)
    assert ny.dtype == nuv.dtype == np.uint8 and np.array_equal(ny, y) and np.array_equal(nuv, uv)
    iy, iu, iv = ingest.rgb_to_yuv420(rgb, "i420", name, full)
    assert iy.dtype == iu.dtype == iv.dtype == np.uint8 and iu.shape == iv.shape == (2, 6, 10)
    assert np.array_equal(iy, y) and np.array_equal(iu, uv[..., 0]) and np.array_equal(iv, uv[..., 1])
    py, puv = ingest.rgb_to_yuv420(rgb, "p010", name, full)
    ty, tu, tv = ingest.rgb_to_yuv420(rgb, "i010", name, full)
    assert py.dtype == puv.dtype == ty.dtype == tu.dtype == tv.dtype == np.uint16 and puv.shape == (2, 6, 10, 2) and tu.shape == (2, 6, 10)
    assert not (py & 63).any() and not (puv & 63).any()
    assert np.array_equal(ty, py >> 6) and np.array_equal(tu, puv[..., 0] >> 6) and np.array_equal(tv, puv[..., 1] >> 6)
    assert ty.max() <= 1023 and (ty & 3).any() and (tu & 3).any()                              # quantised once to 10 bits
    assert np.abs(ty.astype(np.int64) - 4 * y.astype(np.int64)).max() <= (6 if full else 3)                    # ... of the same picture
    if not full:
        assert ty.min() >= 64 and ty.max() <= 940 and tu.min() >= 64 and tu.max() <= 960
    one = ingest.rgb_to_yuv420(rgb[0], "i010", name, full)                                     # one frame [H,W,3]
    assert one[0].shape == (12, 20) and np.array_equal(one[0], ty[0])


STEP = {("i420", False): 1.0, ("i420", True): 1.0, ("p010", False): 0.25, ("i010", False): 0.25, ("p010", True): 255.0 / 1023.0, ("i010", True): 255.0 / 1023.0}


@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("name,full", oracle.COLOURS)
def test_colour_round_trip(name, full, fmt):
    """rgb_to_yuv420 then the oracle's YUV -> RGB on frames of one colour gives the colour back within the rounding of Y, Cb, Cr to the
    format's depth: each is off by at most half a code, i.e. half of `step` in the 8-bit scale (1 for 8 bits, 1/4 for 10-bit limited range,
    255/1023 for 10-bit full range), so channel c is off by at most 0.5 * step * sum_k |M[c,k]| (the derivation of test_colour_round_trip in
    tests/test_ingest_formats.py).  A grey ramp keeps R = G = B and the chroma at the centre code."""
    from arseg_amd import ingest

    _, m = oracle.matrix(name, full)
    bound = 0.5 * STEP[(fmt, full)] * np.abs(m).sum(axis=1) + 1e-9
    g = np.random.Generator(np.random.PCG64(5))
    colours = np.concatenate([g.integers(0, 256, (40, 3)), [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255]]])
    worst = np.zeros(3)
    for col in colours:
        rgb = np.broadcast_to(np.asarray(col, np.uint8), (4, 6, 3)).copy()
        planes = ingest.rgb_to_yuv420(rgb, fmt, name, full)
        back = yuv.yuv_to_rgb(fmt, planes, name, full)
        assert back.shape == (4, 6, 3)
        err = np.abs(back - rgb).reshape(-1, 3).max(axis=0)
        worst = np.maximum(worst, err)
        assert (err <= bound).all(), (col, err, bound)
    print(f"\n{fmt} {name} {'full' if full else 'limited'}: worst |RGB error| {worst}, bound {bound}")
    ramp = np.repeat(np.arange(0, 256, 4, dtype=np.uint8)[None, :, None], 3, axis=2).repeat(4, axis=0)          # [4,64,3] grey, left to right
    planes = ingest.rgb_to_yuv420(ramp, fmt, name, full)
    y, u, v = yuv.codes(fmt, planes)
    centre = 2 ** (yuv.DEPTH[fmt] - 1)
    assert (u == centre).all() and (v == centre).all()
    back = yuv.yuv_to_rgb(fmt, planes, name, full)
    assert np.abs(back - back[..., :1]).max() <= 1e-9 and np.abs(back - ramp).max() <= bound.max()
    if not full:
        lo = 16 * 2 ** (yuv.DEPTH[fmt] - 8)
        assert y.min() == lo and y.max() <= 235 * 2 ** (yuv.DEPTH[fmt] - 8)


@pytest.mark.parametrize("name,full", oracle.COLOURS)
def test_oracle_reduces_to_the_nv12_oracle(name, full):
    """fp64, exact to 1e-9: I420 from de-interleaved NV12 chroma is the NV12 oracle; P010 / I010 holding 4 x the NV12 bytes are too in limited
    range (4 x the levels); junk in the ignored bits (low 6 of P010, high 6 of I010) changes nothing."""
    g = np.random.Generator(np.random.PCG64(21))
    y = g.integers(0, 256, (2, 12, 20), dtype=np.uint8)
    uv = g.integers(0, 256, (2, 6, 10, 2), dtype=np.uint8)
    for (h, w) in ((12, 20), (6, 10), (18, 30)):
        want = oracle.ingest_nv12(y, uv, h, w, MEAN, STD, name, full)
        got = yuv.ingest_yuv("i420", (y, uv[..., 0], uv[..., 1]), h, w, MEAN, STD, name, full)
        assert np.abs(got - want).max() <= 1e-9
        if full:
            continue
        y4, uv4 = y.astype(np.uint16) * 4, uv.astype(np.uint16) * 4
        junk_lo = g.integers(0, 64, y4.shape, dtype=np.uint16), g.integers(0, 64, uv4.shape, dtype=np.uint16)
        junk_hi = g.integers(0, 64, y4.shape, dtype=np.uint16) << 10, g.integers(0, 64, uv4.shape, dtype=np.uint16) << 10
        got_p = yuv.ingest_yuv("p010", ((y4 << 6) | junk_lo[0], (uv4 << 6) | junk_lo[1]), h, w, MEAN, STD, name, full)
        got_i = yuv.ingest_yuv("i010", (y4 | junk_hi[0], uv4[..., 0] | junk_hi[1][..., 0], uv4[..., 1] | junk_hi[1][..., 1]), h, w, MEAN, STD, name, full)
        assert np.abs(got_p - want).max() <= 1e-9 and np.abs(got_i - want).max() <= 1e-9
    # full range: 10-bit code c stands for c * 255 / 1023, so codes 0 and 1023 are the 8-bit codes 0 and 255
    if full:
        ends = np.array([[0, 1023]], dtype=np.uint16).repeat(2, axis=0)
        mid = np.full((1, 1), 512, np.uint16)
        rgb10 = yuv.yuv_to_rgb("i010", (ends, mid, mid), name, True)
        rgb8 = yuv.yuv_to_rgb("i420", ((ends // 1023 * 255).astype(np.uint8), np.full((1, 1), 128, np.uint8), np.full((1, 1), 128, np.uint8)), name, True)
        assert np.abs(rgb10 - rgb8).max() <= 1e-9
