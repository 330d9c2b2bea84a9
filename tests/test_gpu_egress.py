"""GPU checks of the segmentation egress (csrc/egress.hip, arseg_segment_egress_fwd; arseg_amd.egress): the label plane against the EXISTING
evaluator tail (ops.argmax_confusion, zero differing pixels), the overlay against the numpy oracle (tests/egress_oracle.py) painted over
the existing tail's labels, bit for bit."""
import numpy as np
import pytest
import torch

import egress_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# (name, n_cls, h, w, H, W, align_corners): the three routes of arseg_argmax_confusion_fwd
ROUTES = [("same", 12, 24, 40, 24, 40, True), ("bilinear", 19, 17, 20, 136, 160, True), ("x2", 19, 9, 11, 18, 22, False),
          ("x4", 19, 9, 11, 36, 44, False), ("x8", 19, 9, 11, 72, 88, False)]
FMTS = ["rgb8", "nv12", "i420"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _logits(seed, N, n_cls, h, w, dev):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal((N, n_cls, h, w)).astype(np.float32)).to(dev)


def _existing(logits, H, W, align):
    from arseg_amd import ops

    return ops.argmax_confusion(logits, None, H, W, align_corners=align)[0]


def _backed(a, pad, dev, fill=None):
    """numpy [N,H,W,...] -> (backing device buffer [N+1,H,W+pad,...] of GUARD bytes, its view [:N,:,:W] holding ``a`` or ``fill``)."""
    N, H, W = a.shape[:3]
    buf = np.full((N + 1, H, W + pad) + a.shape[3:], GUARD, dtype=np.uint8)
    buf[:N, :, :W] = a if fill is None else fill
    t = torch.from_numpy(buf).to(dev)
    return t, t[:N, :, :W]


def _guards_intact(backing, N, W):
    b = backing.cpu().numpy()
    return bool((b[:N, :, W:] == GUARD).all() and (b[N:] == GUARD).all())


def _np_planes(seed, fmt, N, H, W):
    g = np.random.Generator(np.random.PCG64(seed))
    if fmt == "rgb8":
        return (g.integers(0, 256, (N, H, W, 3), dtype=np.uint8),)
    y, uv = g.integers(0, 256, (N, H, W), dtype=np.uint8), g.integers(0, 256, (N, H // 2, W // 2, 2), dtype=np.uint8)
    return (y, uv) if fmt == "nv12" else (y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]))


def _decoded(fmt, views, colour=("bt709", False)):
    from arseg_amd import ingest

    if fmt == "rgb8":
        return ingest.DecodedFrames.rgb8(views[0])
    make = ingest.DecodedFrames.nv12 if fmt == "nv12" else ingest.DecodedFrames.i420
    return make(*views, matrix=colour[0], full_range=colour[1])


def _palette(n_cls, seed=9):
    from arseg_amd import egress

    g = np.random.Generator(np.random.PCG64(seed))
    alpha = g.random(n_cls)
    alpha[0], alpha[-1] = 0.0, 1.0
    return egress.Palette(g.integers(0, 256, (n_cls, 3), dtype=np.uint8), alpha)


def _fmt_enum(fmt):
    from arseg_amd import _lib

    return {"rgb8": _lib.SRC_RGB8, "nv12": _lib.SRC_NV12, "i420": _lib.SRC_I420}[fmt]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("pad", [0, 3])
def test_labels8_equal_the_existing_tail(dev, route, pad):
    """labels8 == ops.argmax_confusion's pred, no differing pixel, on every route; with a LUT == lut[pred]; a pitched output buffer keeps
    its guard bytes."""
    from arseg_amd import egress

    _, n_cls, h, w, H, W, align = route
    N = 3
    logits = _logits(17, N, n_cls, h, w, dev)
    pred = _existing(logits, H, W, align)
    backing, view = _backed(np.zeros((N, H, W), dtype=np.uint8), pad, dev, fill=7)
    got = egress.labels8(logits, H, W, out=view, align_corners=align)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W)
    diff = int((got.int() != pred).sum())
    print(f"\n{route[0]} pad {pad}: {diff} differing labels of {pred.numel()}")
    assert diff == 0 and _guards_intact(backing, N, W)
    lut = np.random.Generator(np.random.PCG64(2)).integers(0, 256, n_cls, dtype=np.uint8)
    mapped = egress.labels8(logits, H, W, lut=lut, align_corners=align)
    assert torch.equal(mapped, torch.from_numpy(lut).to(dev)[pred.long()])


@pytest.mark.parametrize("n_cls", [1, 32])
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
def test_labels8_class_count_extremes(dev, route, n_cls):
    from arseg_amd import egress

    _, _, h, w, H, W, align = route
    logits = _logits(23 + n_cls, 2, n_cls, h, w, dev)
    pred = _existing(logits, H, W, align)
    got = egress.labels8(logits, H, W, align_corners=align)
    assert int((got.int() != pred).sum()) == 0
    if n_cls == 32:
        assert len(torch.unique(got)) > 16


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
def test_labels8_ties_and_nans(dev, route):
    """Planted exact ties (the first maximum wins) and NaNs (a NaN counts as the maximum): the same labels as the existing kernel."""
    from arseg_amd import egress

    _, n_cls, h, w, H, W, align = route
    g = np.random.Generator(np.random.PCG64(31))
    x = g.standard_normal((2, n_cls, h, w)).astype(np.float32)
    x[:, 3, ::2, :] = 9.0
    x[:, 7, ::2, :] = 9.0                                        # exact ties between classes 3 and 7 on whole rows
    x[:, :, 1, 1::3] = 0.5                                       # all classes tie
    x[0, 5, 2, 2] = np.nan
    x[0, 9, 2, 2] = np.nan
    x[1, n_cls - 1, h - 1, :] = np.nan
    x[1, 2, :, 0] = np.inf
    logits = torch.from_numpy(x).to(dev)
    pred = _existing(logits, H, W, align)
    got = egress.labels8(logits, H, W, align_corners=align)
    assert int((got.int() != pred).sum()) == 0


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("fmt", FMTS)
def test_overlay_equals_the_oracle(dev, fmt, route, pad):
    """Every output plane == egress_oracle.paint(labels of the existing kernel): a frames[1:3] slice of pitched planes, guard bytes after
    each row and after the last image untouched, in place == out of place, labels + overlay from one launch == each alone."""
    from arseg_amd import egress

    _, n_cls, h, w, H, W, align = route
    N = 3
    logits = _logits(41, N, n_cls, h, w, dev)
    pred = _existing(logits[1:3], H, W, align).cpu().numpy()
    src_np = _np_planes(43, fmt, N, H, W)
    src_b = [_backed(a, pad, dev) for a in src_np]
    dst_b = [_backed(a, pad + 4, dev, fill=0) for a in src_np]                    # the destination has its own pitch
    src, dst = _decoded(fmt, [v for _, v in src_b]), _decoded(fmt, [v for _, v in dst_b])
    pal = _palette(n_cls)
    want = oracle.paint(pred, [a[1:3] for a in src_np], fmt, pal.codes(_fmt_enum(fmt), src.colour), pal.weights)

    out, none = egress.overlay(logits[1:3].contiguous(), src[1:3], pal, out=dst[1:3], align_corners=align)
    assert none is None and out.src_format == src.src_format and out.shape == (2, 3, H, W)
    for i, (plane, w_np) in enumerate(zip(out.planes, want)):
        bad = int((plane.cpu().numpy() != w_np).sum())
        print(f"\n{fmt} {route[0]} pad {pad} plane {i}: {bad} differing samples of {w_np.size}")
        assert bad == 0
    for (backing, view), a in zip(dst_b, src_np):
        assert _guards_intact(backing, N, a.shape[2]) and bool((view[0] == 0).all())          # frame 0 is outside the slice
    for (backing, view), a in zip(src_b, src_np):
        assert _guards_intact(backing, N, a.shape[2]) and np.array_equal(view.cpu().numpy(), a)      # the source is only read

    fresh, labels = egress.overlay(logits[1:3].contiguous(), src[1:3], pal, labels_out=True, align_corners=align)     # allocated outputs, both at once
    assert fresh.equal(out)
    assert torch.equal(labels, egress.labels8(logits[1:3].contiguous(), H, W, align_corners=align)) and np.array_equal(labels.cpu().numpy(), pred)

    same, _ = egress.overlay(logits[1:3].contiguous(), src[1:3], pal, out=src[1:3], align_corners=align)              # in place
    for plane, w_np in zip(same.planes, want):
        assert np.array_equal(plane.cpu().numpy(), w_np)
    for (backing, view), a in zip(src_b, src_np):
        assert _guards_intact(backing, N, a.shape[2]) and np.array_equal(view[0].cpu().numpy(), a[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_overlay_adversarial_label_maps(dev, fmt):
    """The oracle's adversarial label maps, forced through one-hot logits on the same-size route: single class, 1-pixel checkerboard (every
    chroma block mixes), weight 0 next to 256, all 32 classes."""
    from arseg_amd import egress

    for name, lab, n_cls, weights in oracle.adversarial_labels(8, 12):
        H, W = lab.shape[1:]
        onehot = np.zeros((1, n_cls, H, W), dtype=np.float32)
        np.put_along_axis(onehot, lab[:, None], 1.0, axis=1)
        logits = torch.from_numpy(onehot).to(dev)
        assert np.array_equal(_existing(logits, H, W, True).cpu().numpy(), lab)
        src_np = _np_planes(51, fmt, 1, H, W)
        src = _decoded(fmt, [torch.from_numpy(a).to(dev) for a in src_np], colour=("bt601", True))
        pal = _palette(n_cls, seed=12)
        pal.weights = np.asarray(weights, dtype=np.uint16)
        out, _ = egress.overlay(logits, src, pal)
        want = oracle.paint(lab, src_np, fmt, pal.codes(_fmt_enum(fmt), src.colour), weights)
        for plane, w_np in zip(out.planes, want):
            assert np.array_equal(plane.cpu().numpy(), w_np), name


def test_overlay_in_one_graph(dev):
    """egress.overlay(..., out=, labels_out=) captured once (one stream, no branches); the logits are refilled in place; each of two replays
    equals the eager result for its own logits."""
    from arseg_amd import egress

    _, n_cls, h, w, H, W, align = ROUTES[4]
    N = 2
    static = _logits(60, N, n_cls, h, w, dev)
    src_np = _np_planes(61, "nv12", N, H, W)
    src = _decoded("nv12", [torch.from_numpy(a).to(dev) for a in src_np])
    out = src._with([torch.zeros_like(p) for p in src.planes])
    labels = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    pal = _palette(n_cls)
    egress.overlay(static, src, pal, out=out, labels_out=labels, align_corners=align)          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        egress.overlay(static, src, pal, out=out, labels_out=labels, align_corners=align)
    for seed in (62, 63):
        fresh = _logits(seed, N, n_cls, h, w, dev)
        static.copy_(fresh)
        for p in out.planes:
            p.zero_()
        labels.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want, want_l = egress.overlay(fresh, src, pal, labels_out=True, align_corners=align)
        assert out.equal(want) and torch.equal(labels, want_l)
        assert np.array_equal(labels.cpu().numpy(), _existing(fresh, H, W, align).cpu().numpy())


@pytest.mark.parametrize("kind", ["psp", "bise"])
def test_alter_res_batch_render(dev, manifest, kind):
    """The small PSPNet (fp32) and BiSeNet (bf16, fused x8 tail) of tests/test_gpu_models.py: alter_res_batch_render's labels equal
    alter_res_batch_pred's pred; with a palette the painted NV12 frames equal the oracle over that pred, out of place and in place."""
    import test_gpu_ingest_formats as tf          # its _nets wraps test_gpu_models' _psp / _bise (+ bf16 storage), _u8_clip turns a synth clip into bytes
    from arseg_amd import egress, ingest, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, kind)
    H, W = (64, 96) if kind == "psp" else (128, 256)
    mean, std = synth.CAMVID_MEAN, synth.CAMVID_STD
    clip = synth.make_clip(9, H, W, gop=4, mean=mean, std=std)
    u8 = tf._u8_clip(clip, mean, std)
    mvs = torch.from_numpy(clip["mv"]).to(dev)
    y, uv = ingest.rgb_to_nv12(u8, "bt709", False)
    nv = ingest.DecodedFrames.nv12(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev), mean, std, matrix="bt709", full_range=False)
    pal = egress.Palette(egress.CAMVID_PALETTE, 0.4)
    lut = np.arange(12, dtype=np.uint8) * 3 + 1
    with torch.no_grad():
        out_k, feat_k = hr.forward_keyframe(nv[0:1])
        refs = [feat_k[0]] * 3
        pred, _ = ev.alter_res_batch_pred(lr, refs, nv[1:4], mvs[1:4], 0.5)
        labels, none = ev.alter_res_batch_render(lr, refs, nv[1:4], mvs[1:4], 0.5)
        assert none is None and labels.dtype == torch.uint8 and int((labels.int() != pred).sum()) == 0
        mapped, painted = ev.alter_res_batch_render(lr, refs, nv[1:4], mvs[1:4], 0.5, palette=pal, lut=lut)
        assert torch.equal(mapped, torch.from_numpy(lut).to(dev)[pred.long()])
        want = oracle.paint(pred.cpu().numpy(), (y[1:4], uv[1:4]), "nv12", pal.codes(nv.src_format, nv.colour), pal.weights)
        assert painted.src_format == nv.src_format and (painted.colour, painted.mean, painted.std) == (nv.colour, nv.mean, nv.std)
        for plane, w_np in zip(painted.planes, want):
            assert np.array_equal(plane.cpu().numpy(), w_np)
        key_painted, key_labels = egress.overlay(out_k.float(), nv[0:1], pal, labels_out=True)          # the keyframe of the GOP
        assert np.array_equal(key_labels.cpu().numpy(), _existing(out_k.float().contiguous(), H, W, True).cpu().numpy())
        inplace = nv[1:4]._with([p.clone() for p in nv[1:4].planes])
        _, same = ev.alter_res_batch_render(lr, refs, inplace, mvs[1:4], 0.5, palette=pal, out=inplace)
        assert same is inplace and same.equal(painted)


def test_full_size_x8_nv12(dev):
    """One 1024x2048 frame, 19 classes, x8 run route, NV12: labels == the existing tail, planes == the oracle."""
    from arseg_amd import egress

    H, W, n_cls = 1024, 2048, 19
    logits = _logits(71, 1, n_cls, H // 8, W // 8, dev)
    pred = _existing(logits, H, W, False)
    src_np = _np_planes(72, "nv12", 1, H, W)
    src = _decoded("nv12", [torch.from_numpy(a).to(dev) for a in src_np])
    pal = egress.Palette(egress.CITYSCAPES_PALETTE, 0.5)
    out, labels = egress.overlay(logits, src, pal, labels_out=True, align_corners=False)
    assert int((labels.int() != pred).sum()) == 0
    want = oracle.paint(pred.cpu().numpy(), src_np, "nv12", pal.codes(src.src_format, src.colour), pal.weights)
    for plane, w_np in zip(out.planes, want):
        assert np.array_equal(plane.cpu().numpy(), w_np)
