"""CPU-side checks of the 8-bit frame ingest (uint8 RGB / NV12 decoder frames into the fast paths): the entry point is declared, bound and
exported, refuses every bad argument before it launches anything, ``ingest.DecodedFrames`` validates what it is given, and the colour
matrices of ``ingest.rgb_to_nv12`` and of the fp64 oracle (tests/ingest_oracle.py) are each other's inverse for all four colour enums."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ingest_oracle as oracle
from conftest import ROOT

MEAN, STD = (0.39068785, 0.40521392, 0.41434407), (0.29652068, 0.30514979, 0.30080369)


def test_entry_point_declared_bound_and_exported():
    from arseg_amd import _lib

    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    lib = _lib.load()
    assert "arseg_frame_ingest_fwd(" in header
    assert "arseg_frame_ingest_fwd" in _lib.PROTOTYPES
    assert hasattr(lib, "arseg_frame_ingest_fwd")
    for name in ("ARSEG_SRC_RGB8", "ARSEG_SRC_NV12", "ARSEG_COLOUR_BT601_LIMITED", "ARSEG_COLOUR_BT601_FULL", "ARSEG_COLOUR_BT709_LIMITED",
                 "ARSEG_COLOUR_BT709_FULL"):
        assert name in header
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert "ingest.hip" in open(os.path.join(ROOT, "ar-seg_amd", "csrc", "Makefile")).read()


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from arseg_amd import _lib

    lib = _lib.load()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)          # (never dereferenced: validation returns first)
    f3, z3 = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.3, 0.0, 0.3)
    RGB, NV, BT = _lib.SRC_RGB8, _lib.SRC_NV12, _lib.COLOUR_BT709_LIMITED
    H, W = 16, 32

    def call(p0=fake, p1=fake, fmt=NV, pitch0=None, pitch1=W, ns0=None, ns1=H * W // 2, colour=BT, out=fake, dt=_lib.DT_BF16, N=2, H=H, W=W, h=8, w=16,
             mean=f3, std=f3):
        pitch0 = (W if fmt == NV else 3 * W) if pitch0 is None else pitch0
        ns0 = H * pitch0 if ns0 is None else ns0
        return lib.arseg_frame_ingest_fwd(p0, p1, fmt, pitch0, pitch1, ns0, ns1, colour, out, dt, N, H, W, h, w, mean, std, null)

    E = _lib.ARSEG_EINVAL
    assert call(p0=null) == E and call(out=null) == E and call(p1=null) == E and call(fmt=RGB, p0=null) == E      # null pointers
    assert call(mean=None) == E and call(std=None) == E
    assert call(std=z3) == E and call(fmt=RGB, std=z3) == E                                                        # zero std
    assert call(H=15) == E and call(W=31) == E                                                                     # odd H / W with NV12
    assert call(pitch0=W - 1) == E and call(pitch1=W - 2) == E and call(fmt=RGB, pitch0=3 * W - 1) == E            # pitch smaller than a row
    assert call(ns0=-1) == E and call(ns1=-4) == E
    assert call(fmt=2) == E and call(fmt=-1) == E and call(colour=4) == E and call(colour=-1) == E and call(dt=3) == E      # unknown enums
    assert call(N=0) == E and call(h=0) == E and call(w=-1) == E
    assert call(out=ctypes.c_void_p((1 << 20) + 8)) == E                                                           # 16-byte stores


def test_decoded_frames_shape_and_views():
    from arseg_amd import _lib, ingest

    rgb = torch.zeros((3, 8, 16, 3), dtype=torch.uint8)
    d = ingest.DecodedFrames.rgb8(rgb, MEAN, STD)
    N, C, H, W = d.shape
    assert (N, C, H, W) == (3, 3, 8, 16) and len(d) == 3 and d.src_format == _lib.SRC_RGB8 and not d.is_cuda and d.device == rgb.device
    assert ingest.DecodedFrames.rgb8(np.zeros((8, 16, 3), np.uint8)).shape == (1, 3, 8, 16)                # one frame, numpy
    assert d[1].shape == (1, 3, 8, 16) and d[1:3].shape == (2, 3, 8, 16) and d[-1].shape == (1, 3, 8, 16)
    padded = torch.zeros((2, 8, 24, 3), dtype=torch.uint8)[:, :, :16]                                      # a row pitch is kept as a view
    assert ingest.DecodedFrames.rgb8(padded).planes[0].data_ptr() == padded.data_ptr()
    y, uv = torch.zeros((2, 8, 16), dtype=torch.uint8), torch.full((2, 4, 8, 2), 128, dtype=torch.uint8)
    n = ingest.DecodedFrames.nv12(y, uv, MEAN, STD, matrix="bt601", full_range=True)
    assert n.shape == (2, 3, 8, 16) and n.src_format == _lib.SRC_NV12 and n.colour == _lib.COLOUR_BT601_FULL
    assert ingest.DecodedFrames.nv12(y, uv).colour == _lib.COLOUR_BT709_LIMITED
    assert ingest.DecodedFrames.nv12(y[0], uv[0]).shape == (1, 3, 8, 16)
    assert n.equal(ingest.DecodedFrames.nv12(y.clone(), uv.clone(), MEAN, STD, matrix="bt601", full_range=True))
    assert not n.equal(ingest.DecodedFrames.nv12(y, uv, MEAN, STD, matrix="bt709", full_range=True))


def test_decoded_frames_validation():
    from arseg_amd import _lib, ingest

    D = ingest.DecodedFrames
    with pytest.raises(ValueError, match="uint8"):
        D.rgb8(torch.zeros((1, 8, 16, 3), dtype=torch.float32))
    with pytest.raises(ValueError, match=r"\[N,H,W,3\]"):
        D.rgb8(torch.zeros((1, 3, 8, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="zero std"):
        D.rgb8(torch.zeros((1, 8, 16, 3), dtype=torch.uint8), MEAN, (0.3, 0.0, 0.3))
    y, uv = torch.zeros((2, 8, 16), dtype=torch.uint8), torch.zeros((2, 4, 8, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        D.nv12(y, uv.to(torch.int16))
    with pytest.raises(ValueError, match="even"):
        D.nv12(torch.zeros((2, 7, 16), dtype=torch.uint8), uv)
    with pytest.raises(ValueError, match="even"):
        D.nv12(torch.zeros((2, 8, 15), dtype=torch.uint8), uv)
    with pytest.raises(ValueError, match="chroma plane"):
        D.nv12(y, torch.zeros((2, 8, 8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="chroma plane"):
        D.nv12(y, torch.zeros((1, 4, 8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="one device"):
        D.nv12(y, torch.zeros((2, 4, 8, 2), dtype=torch.uint8, device="meta"))
    with pytest.raises(ValueError, match="bt601"):
        D.nv12(y, uv, matrix="bt2020")
    with pytest.raises(_lib.ArsegError, match="GPU only"):                  # no CPU fallback: the kernel is the only route
        D.rgb8(torch.zeros((1, 8, 16, 3), dtype=torch.uint8)).to_input(4, 8, torch.float32)
    with pytest.raises(ValueError):
        ingest.rgb_to_nv12(np.zeros((7, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        ingest.rgb_to_nv12(np.zeros((8, 8, 3), np.float32))


def test_ingest_input_refuses_what_is_neither_tensor_nor_decoded_frames():
    from arseg_amd import _lib, ops

    with pytest.raises(_lib.ArsegError, match="DecodedFrames"):
        ops.ingest_input([1, 2, 3], 4, 4)


@pytest.mark.parametrize("name,full", oracle.COLOURS)
def test_colour_round_trip(name, full):
    """rgb_to_nv12 then the oracle's NV12 -> RGB on frames of one colour gives the colour back within the 8-bit rounding of Y, Cb, Cr: each
    of the three is off by at most half a step, so channel c is off by at most 0.5 * sum_k |M[c,k]| (+ the clip never cuts a valid colour by
    more than that).  A grey ramp keeps R = G = B.  Pins the matrices against a sign or row mix-up."""
    from arseg_amd import ingest

    _, m = oracle.matrix(name, full)
    bound = 0.5 * np.abs(m).sum(axis=1) + 1e-9
    g = np.random.Generator(np.random.PCG64(5))
    colours = np.concatenate([g.integers(0, 256, (40, 3)), [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255]]])
    worst = np.zeros(3)
    for col in colours:
        rgb = np.broadcast_to(np.asarray(col, np.uint8), (4, 6, 3)).copy()
        y, uv = ingest.rgb_to_nv12(rgb, name, full)
        assert y.shape == (4, 6) and uv.shape == (2, 3, 2) and y.dtype == uv.dtype == np.uint8
        back = oracle.nv12_to_rgb(y, uv, name, full)
        err = np.abs(back - rgb).reshape(-1, 3).max(axis=0)
        worst = np.maximum(worst, err)
        assert (err <= bound).all(), (col, err, bound)
    print(f"\n{name} {'full' if full else 'limited'}: worst |RGB error| {worst}, bound {bound}")
    ramp = np.repeat(np.arange(0, 256, 4, dtype=np.uint8)[None, :, None], 3, axis=2).repeat(4, axis=0)          # [4,64,3] grey, left to right
    y, uv = ingest.rgb_to_nv12(ramp, name, full)
    assert (uv == 128).all()
    back = oracle.nv12_to_rgb(y, uv, name, full)
    assert np.abs(back - back[..., :1]).max() <= 1e-9 and np.abs(back - ramp).max() <= bound.max()
    if not full:
        assert y.min() == 16 and y.max() <= 235


def test_oracle_rgb_path_is_to_tensor_normalize_interpolate():
    """The oracle's RGB half against torch on the CPU (F.interpolate align_corners=True of ToTensor + Normalize in float64)."""
    import torch.nn.functional as F

    g = np.random.Generator(np.random.PCG64(6))
    img = g.integers(0, 256, (2, 20, 28, 3), dtype=np.uint8)
    norm = (torch.from_numpy(img).double().permute(0, 3, 1, 2) / 255.0 - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    want = F.interpolate(norm, (10, 14), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
    assert np.abs(oracle.ingest(img, 10, 14, MEAN, STD) - want).max() <= 1e-5          # (float32 sampling positions vs float64: 28-pixel rows)
    assert np.abs(oracle.ingest(img, 20, 28, MEAN, STD) - norm.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
