"""CPU-side checks of the segmentation egress: the numpy oracle's own invariants (tests/egress_oracle.py), egress.Palette (codes, weight
quantisation), the host layer's argument checks, and the argument validation of arseg_segment_egress_fwd, which happens before any launch."""
import ctypes

import numpy as np
import pytest

import egress_oracle as oracle


def _frame(seed, N, H, W):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(0, 256, (N, H, W), dtype=np.uint8), g.integers(0, 256, (N, H // 2, W // 2, 2), dtype=np.uint8),
            g.integers(0, 256, (N, H, W, 3), dtype=np.uint8))


def test_oracle_invariants():
    """All weights 0: the source comes back; all weights 256 and one class: luma = palette Y, chroma = palette C everywhere; a 2x2 block of
    one class: chroma follows the RGB8 formula; NV12 and I420 agree sample for sample."""
    y, uv, rgb = _frame(3, 2, 8, 12)
    g = np.random.Generator(np.random.PCG64(4))
    codes = g.integers(0, 256, (7, 3), dtype=np.uint8)
    labels = g.integers(0, 7, (2, 8, 12))
    zero = np.zeros(7, dtype=np.int64)
    oy, ouv = oracle.paint(labels, (y, uv), "nv12", codes, zero)
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv)
    assert np.array_equal(oracle.paint(labels, (rgb,), "rgb8", codes, zero)[0], rgb)
    one = np.full((2, 8, 12), 5)
    oy, ouv = oracle.paint(one, (y, uv), "nv12", codes, np.full(7, 256))
    assert (oy == codes[5, 0]).all() and (ouv[..., 0] == codes[5, 1]).all() and (ouv[..., 1] == codes[5, 2]).all()
    assert (oracle.paint(one, (rgb,), "rgb8", codes, np.full(7, 256))[0] == codes[5]).all()
    w = g.integers(0, 257, 7)
    blocky = np.repeat(np.repeat(g.integers(0, 7, (2, 4, 6)), 2, axis=1), 2, axis=2)          # every 2x2 block holds one class
    _, ouv = oracle.paint(blocky, (y, uv), "nv12", codes, w)
    kb = blocky[:, ::2, ::2]
    for ch in (0, 1):
        want = (uv[..., ch].astype(np.int64) * (256 - w[kb]) + codes[kb, ch + 1].astype(np.int64) * w[kb] + 128) >> 8
        assert np.array_equal(ouv[..., ch], want)
    py, pu, pv = oracle.paint(labels, (y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])), "i420", codes, w)
    ny, nuv = oracle.paint(labels, (y, uv), "nv12", codes, w)
    assert np.array_equal(py, ny) and np.array_equal(pu, nuv[..., 0]) and np.array_equal(pv, nuv[..., 1])


def test_adversarial_label_maps_do_what_their_names_say():
    cases = {name: (lab, n_cls, w) for name, lab, n_cls, w in oracle.adversarial_labels()}
    assert len(np.unique(cases["single class"][0])) == 1
    cb = cases["checkerboard"][0][0]
    assert (cb[::2, ::2] != cb[::2, 1::2]).all() and (cb[::2, ::2] != cb[1::2, ::2]).all()          # every 2x2 block mixes
    lab, _, w = cases["weight 0 next to 256"]
    assert sorted(np.unique(np.asarray(w)[lab]).tolist()) == [0, 256]
    assert len(np.unique(cases["all 32 classes"][0])) == 32
    for lab, n_cls, w in cases.values():
        assert lab.max() < n_cls and len(w) == n_cls


def test_palette_codes_and_weights():
    """RGB8 codes are the colours; NV12 / I420 codes equal ingest.rgb_to_nv12 of a 2x2 image of the colour, for all four colour enums;
    weights = clip(rint(alpha * 256), 0, 256)."""
    from arseg_amd import _lib, egress, ingest

    assert len(egress.CAMVID_PALETTE) == 12 and len(egress.CITYSCAPES_PALETTE) == 19
    pal = egress.Palette(egress.CITYSCAPES_PALETTE, 0.5)
    assert np.array_equal(pal.codes(_lib.SRC_RGB8), np.array(egress.CITYSCAPES_PALETTE, dtype=np.uint8))
    assert pal.weights.dtype == np.uint16 and (pal.weights == 128).all() and len(pal) == 19
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            enum = ingest.colour_enum(matrix, full)
            codes = pal.codes(_lib.SRC_NV12, enum)
            assert codes.shape == (19, 3) and codes.dtype == np.uint8 and np.array_equal(codes, pal.codes(_lib.SRC_I420, enum))
            for k, colour in enumerate(egress.CITYSCAPES_PALETTE):
                img = np.empty((2, 2, 3), dtype=np.uint8)
                img[:] = colour
                y, uv = ingest.rgb_to_nv12(img, matrix, full)
                assert (y == codes[k, 0]).all() and tuple(uv[0, 0]) == (codes[k, 1], codes[k, 2])
    assert not np.array_equal(pal.codes(_lib.SRC_NV12, _lib.COLOUR_BT601_FULL), pal.codes(_lib.SRC_NV12, _lib.COLOUR_BT709_LIMITED))
    alphas = [0.0, 1.0, -0.5, 7.0, 0.5, 1 / 512 + 1e-9, 0.25, 0.999, 1 / 3, 0.1, 0.9, 0.0019]
    w = egress.Palette(egress.CAMVID_PALETTE, alphas).weights
    assert w.tolist() == [0, 256, 0, 256, 128, 1, 64, 256, 85, 26, 230, 0]
    with pytest.raises(ValueError):
        pal.codes(_lib.SRC_P010)
    with pytest.raises(ValueError):
        egress.Palette(egress.CAMVID_PALETTE, [0.5] * 11)
    with pytest.raises(ValueError):
        egress.Palette(np.zeros((4, 4), dtype=np.uint8))


def test_overlay_argument_checks():
    """ValueError before anything touches a GPU: a palette shorter than n_cls, a 10-bit DecodedFrames, a float frame tensor."""
    import torch

    from arseg_amd import egress, ingest

    logits = torch.zeros((1, 12, 4, 6))
    y, uv, rgb = _frame(5, 1, 8, 12)
    frames = ingest.DecodedFrames.nv12(y, uv)
    with pytest.raises(ValueError):
        egress.overlay(logits, frames, egress.Palette(egress.CAMVID_PALETTE[:11]))
    y16 = torch.zeros((1, 8, 12), dtype=torch.int16)
    ten = ingest.DecodedFrames.p010(y16, torch.zeros((1, 4, 6, 2), dtype=torch.int16))
    with pytest.raises(ValueError):
        egress.overlay(logits, ten, egress.Palette(egress.CAMVID_PALETTE))
    ten = ingest.DecodedFrames.i010(y16, torch.zeros((1, 4, 6), dtype=torch.int16), torch.zeros((1, 4, 6), dtype=torch.int16))
    with pytest.raises(ValueError):
        egress.overlay(logits, ten, egress.Palette(egress.CAMVID_PALETTE))
    with pytest.raises(ValueError):
        egress.overlay(logits, torch.zeros((1, 3, 8, 12)), egress.Palette(egress.CAMVID_PALETTE))


def test_host_tables_and_render_argument_checks():
    """lut / palette / weights are taken as any integer sequence in range (a plain list included) and refused out of range; out= without a
    palette is a ValueError of alter_res_batch_render before anything runs."""
    from arseg_amd import evaluation as ev
    from arseg_amd.ops import egress as oe

    assert bytes(oe._host_u8([3, 0, 255], 3, "lut")) == bytes([3, 0, 255])
    assert bytes(oe._host_u8(np.arange(4, dtype=np.int64), 4, "lut")) == bytes([0, 1, 2, 3])
    assert bytes(oe._host_u8(np.array([[1, 2, 3], [4, 5, 6]], dtype=np.uint8), 6, "palette")) == bytes([1, 2, 3, 4, 5, 6])
    for bad in ([1, 2], [1, 2, 256], [1, -1, 2], [0.5, 1.0, 2.0]):
        with pytest.raises(ValueError):
            oe._host_u8(bad, 3, "lut")
    with pytest.raises(ValueError):
        ev.alter_res_batch_render(None, [], None, None, 0.5, palette=None, out=object())


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract comes back before any launch (device pointers are dummies and never dereferenced; the
    host tables are real)."""
    from arseg_amd import _lib

    lib = _lib.load()
    fn = lib.arseg_segment_egress_fwd
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    EINVAL = _lib.ARSEG_EINVAL
    n_cls, h, w, H, W = 19, 4, 6, 32, 48
    pal = (ctypes.c_uint8 * (3 * 32))(*([7] * 96))
    wt = (ctypes.c_uint16 * 32)(*([128] * 32))
    lut = (ctypes.c_uint8 * 32)(*range(32))

    def call(logits=one, N=2, n_cls=n_cls, h=h, w=w, H=H, W=W, align=0, lut=lut, lab=one, lab_pitch=W, lab_ns=H * W, fmt=_lib.SRC_NV12,
             src=(one, one, one), sp=(W, W, W), sn=(H * W, H * W // 2, H * W // 4), dst=(one, one, one), dp=(W, W, W),
             dn=(H * W, H * W // 2, H * W // 4), pal=pal, wt=wt):
        return fn(logits, N, n_cls, h, w, H, W, align, lut, lab, lab_pitch, lab_ns, fmt, *src, *sp, *sn, *dst, *dp, *dn, pal, wt, null)

    none3 = (null, null, null)
    assert call(logits=null) == EINVAL                                            # null logits
    assert call(lab=null, dst=none3) == EINVAL                                    # nothing to write
    assert call(src=none3) == EINVAL                                              # destination without source,
    assert call(pal=None) == EINVAL                                               # ... palette
    assert call(wt=None) == EINVAL                                                # ... or weights
    assert call(src=(one, null, null)) == EINVAL and call(dst=(one, null, null)) == EINVAL          # NV12 without its chroma plane
    assert call(fmt=_lib.SRC_I420, src=(one, one, null)) == EINVAL and call(fmt=_lib.SRC_I420, dst=(one, one, null)) == EINVAL
    for bad in (0, -1, 33):
        assert call(n_cls=bad) == EINVAL
        assert call(n_cls=bad, dst=none3) == EINVAL
    heavy = (ctypes.c_uint16 * 32)(*([128] * 18 + [257] + [0] * 13))
    assert call(wt=heavy) == EINVAL                                               # a weight above 256
    for name in ("N", "h", "w", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL       # a non-positive size
    for fmt in (_lib.SRC_NV12, _lib.SRC_I420):
        assert call(fmt=fmt, H=H + 1) == EINVAL and call(fmt=fmt, W=W + 1, sp=(W + 1,) * 3, dp=(W + 1,) * 3, lab_pitch=W + 1) == EINVAL
    assert call(lab_pitch=W - 1) == EINVAL                                        # a pitch smaller than a row
    assert call(sp=(W - 1, W, W)) == EINVAL and call(sp=(W, W - 1, W)) == EINVAL
    assert call(dp=(W - 1, W, W)) == EINVAL and call(dp=(W, W - 1, W)) == EINVAL
    assert call(fmt=_lib.SRC_I420, sp=(W, W // 2, W // 2 - 1)) == EINVAL and call(fmt=_lib.SRC_I420, dp=(W, W // 2 - 1, W // 2)) == EINVAL
    assert call(fmt=_lib.SRC_RGB8, sp=(3 * W - 1, 0, 0), dp=(3 * W, 0, 0)) == EINVAL
    assert call(fmt=_lib.SRC_RGB8, sp=(3 * W, 0, 0), dp=(3 * W - 1, 0, 0)) == EINVAL
    assert call(lab_ns=-1) == EINVAL                                              # a negative image stride
    assert call(sn=(-1, 0, 0)) == EINVAL and call(dn=(0, -1, 0)) == EINVAL and call(fmt=_lib.SRC_I420, sp=(W, W // 2, W // 2), dp=(W, W // 2, W // 2), dn=(0, 0, -1)) == EINVAL
    for fmt in (_lib.SRC_P010, _lib.SRC_I010, 5, -1):
        assert call(fmt=fmt) == EINVAL                                            # 10-bit and unknown formats are rejected
