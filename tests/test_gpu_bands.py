"""GPU tests of the boundary bands (ops.label_bands, csrc/bands.hip) against tests/bands_oracle.py, which states the window definition
without the kernels' separable form, and of what is built on it (evaluation.alter_res_batch_bands, evaluation.EvalByBand).  Labels and
predictions come from numpy, so only bands.hip runs, except where the model is the point.  Every comparison is of integers and exact.

The kernels' sizes the shapes aim at: 64-pixel chunks and 1024-pixel segments of a row (the row launch), tiles of 64 x 64 pixels with a
halo of R rows (the column launch)."""
import numpy as np
import pytest
import torch

import bands_oracle as bo

pytestmark = pytest.mark.gpu

GUARD = 0xAB
TILE, SEG = 64, 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _preds(seed, label, n_cls, wrong=0.2):
    """The labels with a share of other values, some of them outside [0, n_cls)."""
    g = np.random.Generator(np.random.PCG64(seed))
    return np.where(g.random(label.shape) < wrong, g.integers(-2, n_cls + 2, label.shape), np.where(label == 255, 0, label)).astype(np.int32)


def run(dev, label, radii, n_cls, pred=None, groups=None, n_groups=1, ignore=255, band=True, hist0=None, pad=(0, 0)):
    """One guarded call: guard bytes behind band_out, hist and the workspace, the inputs compared after the call.  ``pad``: extra bytes
    per row and extra rows per image of band_out.  -> (bands uint8 [N,H,W] | None, hist int64 | None), numpy."""
    from arseg_amd import _lib, ops

    N, H, W = label.shape
    lab_t = torch.from_numpy(label).to(dev)
    pred_t = None if pred is None else torch.from_numpy(pred).to(dev)
    grp_t = groups if groups is None or isinstance(groups, list) else torch.tensor(groups, dtype=torch.int32, device=dev)
    grp_keep = None if not torch.is_tensor(grp_t) else grp_t.clone()
    need = _lib.load().arseg_label_bands_workspace_bytes(N, H, W)
    ws_all = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=dev)
    band_all = band_t = None
    if band:
        pitch, rows = W + pad[0], H + pad[1]
        band_all = torch.full((N * rows * pitch + 64,), GUARD, dtype=torch.uint8, device=dev)
        band_t = band_all[:N * rows * pitch].view(N, rows, pitch)[:, :H, :W]
    hist_all = hist_t = None
    if pred is not None:
        nb = len(radii) + 1
        hist_all = torch.full((n_groups + 2, nb, n_cls, n_cls), -7, dtype=torch.int64, device=dev)
        hist_t = hist_all[1:n_groups + 1]
        hist_t.copy_(torch.zeros_like(hist_t) if hist0 is None else torch.from_numpy(hist0).to(dev))
    got_b, got_h = ops.label_bands(lab_t, radii, pred=pred_t, groups=grp_t, n_groups=n_groups, n_cls=n_cls, hist=hist_t, ignore_label=ignore,
                                   band_out=band_t, workspace=ws_all[:need])
    torch.cuda.synchronize()
    assert bool((ws_all[need:] == GUARD).all()), "the workspace's guard"
    assert np.array_equal(lab_t.cpu().numpy(), label) and (pred is None or np.array_equal(pred_t.cpu().numpy(), pred))
    assert grp_keep is None or torch.equal(grp_keep, grp_t)
    if band:
        assert got_b.data_ptr() == band_t.data_ptr()
        seen = band_all.clone()
        seen[:N * rows * pitch].view(N, rows, pitch)[:, :H, :W] = GUARD
        assert bool((seen == GUARD).all()), "band_out's guard, padding included"
    else:
        assert got_b is None
    if pred is not None:
        assert got_h.data_ptr() == hist_t.data_ptr()
        assert bool((hist_all[0] == -7).all()) and bool((hist_all[-1] == -7).all()), "hist's guard groups"
    else:
        assert got_h is None
    return (None if not band else band_t.cpu().numpy()), (None if pred is None else hist_t.cpu().numpy())


def check(dev, label, radii, n_cls, pred=None, groups=None, n_groups=1, ignore=255, want_band=None, **kw):
    """``run`` against the oracle -> (bands, hist)."""
    if want_band is None:
        want_band = bo.label_bands(label, radii, n_cls, ignore, fast=True)
    got_b, got_h = run(dev, label, radii, n_cls, pred=pred, groups=groups, n_groups=n_groups, ignore=ignore, **kw)
    if got_b is not None:
        bad = np.argwhere(got_b != want_band)
        assert bad.size == 0, f"{len(bad)} bands differ, the first at (n, y, x) = {bad[0].tolist()}: {got_b[tuple(bad[0])]} for {want_band[tuple(bad[0])]}"
    if pred is not None:
        ids = [0] * label.shape[0] if groups is None else [int(g) for g in groups]
        want_h = bo.banded_hist(label, pred, want_band, ids, n_groups, len(radii), n_cls, ignore)
        if kw.get("hist0") is not None:
            want_h = want_h + kw["hist0"]
        assert np.array_equal(got_h, want_h)
    return got_b, got_h


@pytest.mark.parametrize("radii", [(1, 2, 3), (1, 3), (2,)], ids=str)
def test_hand_cases(dev, radii):
    same = [h for h in bo.HAND if np.array(h[1]).shape == (5, 5) and h[2] == 255]
    assert len(same) == 9
    label = np.stack([np.array(h[1], dtype=np.int64) for h in same])
    want = np.stack([bo.bands(np.array(h[3]), radii) for h in same])                         # from the literals
    pred = _preds(1, label, bo.HAND_N_CLS)
    check(dev, label, radii, bo.HAND_N_CLS, pred=pred, groups=[0, 1, 2, 0, 1, 2, 0, 1, 2], n_groups=3, want_band=want)
    for name, plane, ignore, d in bo.HAND:
        if (name, plane, ignore, d) not in same:
            lab = np.array(plane, dtype=np.int64)[None]
            check(dev, lab, radii, bo.HAND_N_CLS, pred=_preds(2, lab, bo.HAND_N_CLS), ignore=ignore, want_band=bo.bands(np.array(d), radii)[None])


# W = 1, 63, 64, 65, 129, 257 and around a row segment; H = 1, 2, 33 and taller than two tiles; one below, at and one above the tile in both
SHAPES = [(3, 1), (33, 63), (2, 64), (33, 65), (1, 129), (2, 257), (1, 1), (2 * TILE + 3, 5), (TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1),
          (2, SEG - 1), (1, SEG), (2, SEG + 1), (3, 2 * SEG + 65)]


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_shapes(dev, H, W):
    n_cls = 7
    label = np.stack([bo.block_plane(100 + H, H, W, n_cls), bo.noise_plane(200 + W, H, W, n_cls), bo.block_plane(300 + W, H, W, n_cls, cell=23)])
    pred = _preds(3, label, n_cls)
    for radii in ((1, 2, 4, 8), (3, 5, 32)):
        check(dev, label, radii, n_cls, pred=pred, groups=[1, 0, 1], n_groups=2)


def _odd_pixel_distance(H, W, py, px):
    """D of a constant plane with one other pixel at (py, px): the Chebyshev distance to it, and 1 at the pixel itself."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.maximum(np.abs(yy - py), np.abs(xx - px))
    d[py, px] = 1
    return d


@pytest.mark.parametrize("r", [1, 8, 32])
def test_pixels_at_exactly_r_and_r_plus_one(dev, r):
    """One differing pixel per frame, placed on the first and last row and column, either side of a 64-lane chunk seam, a tile seam and a
    row-segment seam: the pixels at Chebyshev distance exactly r of it are in band 0 and those at r + 1 are interior, horizontally, vertically
    and diagonally, whichever seam lies between -- the whole plane is compared, and the probes are named."""
    H, W = 2 * TILE + 2, SEG + 70
    spots = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (TILE - 1, TILE - 1), (TILE, TILE), (TILE - 1, SEG - 1), (TILE, SEG), (2 * TILE - 1, 3 * 64),
             (1, SEG - 64)]
    label = np.full((len(spots), H, W), 3, np.int64)
    for n, (py, px) in enumerate(spots):
        label[n, py, px] = 255 if n % 2 else 5
    want = np.stack([(_odd_pixel_distance(H, W, py, px) > r).astype(np.uint8) for py, px in spots])
    got, _ = check(dev, label, (r,), 6, want_band=want)
    for n, (py, px) in enumerate(spots):
        for sy, sx in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)):
            for dist, band in ((r, 0), (r + 1, 1)):
                y, x = py + sy * dist, px + sx * dist
                if 0 <= y < H and 0 <= x < W:
                    assert got[n, y, x] == band, (n, py, px, y, x)


def test_band_out_pitch_and_image_stride(dev):
    n_cls, radii = 5, (1, 2, 4, 8)
    label = np.stack([bo.block_plane(20, 37, 70, n_cls), bo.noise_plane(21, 37, 70, n_cls)])
    check(dev, label, radii, n_cls, pred=_preds(4, label, n_cls), pad=(7, 0))
    check(dev, label, radii, n_cls, pad=(0, 3))
    check(dev, label, radii, n_cls, pad=(13, 2))


def test_unlike_frames_in_both_orders(dev):
    n_cls, radii = 5, (2, 4)
    a, b = bo.block_plane(22, 70, 130, n_cls, cell=30), bo.noise_plane(23, 70, 130, n_cls)
    pa, pb = _preds(5, a, n_cls), _preds(6, b, n_cls, wrong=0.5)
    b1, h1 = check(dev, np.stack([a, b]), radii, n_cls, pred=np.stack([pa, pb]), groups=[0, 1], n_groups=2)
    b2, h2 = check(dev, np.stack([b, a]), radii, n_cls, pred=np.stack([pb, pa]), groups=[1, 0], n_groups=2)
    assert np.array_equal(b1[0], b2[1]) and np.array_equal(b1[1], b2[0]) and np.array_equal(h1, h2)
    assert not np.array_equal(h1[0], h1[1])


@pytest.mark.parametrize("n_cls", [1, 19, 32])
def test_groups_accumulation_and_optional_buffers(dev, n_cls):
    from arseg_amd import ops

    radii = (1, 2, 4, 8)
    N, H, W = 5, 35, 67
    label = np.stack([bo.block_plane(30 + n, H, W, n_cls, cell=11) for n in range(N)])
    pred = _preds(7, label, n_cls)                                                         # with predictions outside [0, n_cls)
    assert (pred < 0).any() and (pred >= n_cls).any()
    # ids on the device, two of them outside [0, n_groups): those frames get their bands and count nowhere
    ids = np.array([2, -1, 0, 3, 2], np.int32)
    band, hist = check(dev, label, radii, n_cls, pred=pred, groups=ids, n_groups=3)
    assert int(hist[1].sum()) == 0 and int(hist.sum()) == int(bo.confusion(label[[0, 2, 4]], pred[[0, 2, 4]], n_cls).sum())
    # a second call accumulates
    _, twice = check(dev, label, radii, n_cls, pred=pred, groups=[2, 1, 0, 1, 2], n_groups=3, hist0=hist)
    assert int(twice.sum()) > int(hist.sum())
    # no groups, one histogram; the sum over the bands is the plain confusion matrix
    _, one = check(dev, label, radii, n_cls, pred=pred)
    assert np.array_equal(one[0].sum(0), bo.confusion(label, pred, n_cls))
    # without the plane, and the plane alone
    none, again = check(dev, label, radii, n_cls, pred=pred, band=False)
    assert none is None and np.array_equal(again, one)
    alone, nothing = check(dev, label, radii, n_cls)
    assert nothing is None and np.array_equal(alone, band)
    # the defaults allocate: the stream's workspace, a fresh histogram, and without pred the plane
    lab_t, pred_t = torch.from_numpy(label).to(dev), torch.from_numpy(pred).to(dev)
    b0, h0 = ops.label_bands(lab_t, radii, pred=pred_t, n_cls=n_cls)
    assert b0 is None and np.array_equal(h0.cpu().numpy(), one)
    b1, h1 = ops.label_bands(lab_t, radii, n_cls=n_cls)
    assert h1 is None and np.array_equal(b1.cpu().numpy(), band)
    b2, h2 = ops.label_bands(lab_t, radii, pred=pred_t, hist=h0, band_out=True)
    assert h2 is h0 and np.array_equal(h0.cpu().numpy(), 2 * one) and np.array_equal(b2.cpu().numpy(), band)


def test_graph_capture_replayed_on_refilled_inputs(dev):
    from arseg_amd import _lib, ops

    n_cls, radii, N, H, W = 6, (1, 2, 4, 8), 2, 70, 131
    sets = []
    for s in (40, 50):
        label = np.stack([bo.block_plane(s, H, W, n_cls, cell=13), bo.noise_plane(s + 1, H, W, n_cls)])
        sets.append((label, _preds(s + 2, label, n_cls), np.array([1, 0] if s == 40 else [0, 2], np.int32)))
    lab_t, pred_t = torch.from_numpy(sets[0][0]).to(dev), torch.from_numpy(sets[0][1]).to(dev)
    grp_t = torch.from_numpy(sets[0][2]).to(dev)
    band_t = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    hist_t = torch.zeros((3, len(radii) + 1, n_cls, n_cls), dtype=torch.int64, device=dev)
    ws = torch.zeros((_lib.load().arseg_label_bands_workspace_bytes(N, H, W),), dtype=torch.uint8, device=dev)

    def call():
        ops.label_bands(lab_t, radii, pred=pred_t, groups=grp_t, n_groups=3, hist=hist_t, band_out=band_t, workspace=ws)

    call()                                                                                  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for which in (1, 0):
        label, pred, ids = sets[which]
        lab_t.copy_(torch.from_numpy(label))
        pred_t.copy_(torch.from_numpy(pred))
        grp_t.copy_(torch.from_numpy(ids))
        band_t.fill_(9)
        hist_t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = bo.label_bands(label, radii, n_cls, fast=True)
        assert np.array_equal(band_t.cpu().numpy(), want)
        assert np.array_equal(hist_t.cpu().numpy(), bo.banded_hist(label, pred, want, ids.tolist(), 3, len(radii), n_cls))


def test_bands_sum_to_the_grouped_tail(dev):
    """Property S: on random logits the sum over the bands is bit-equal to ops.argmax_confusion_grouped's histogram."""
    from arseg_amd import ops

    N, n_cls, H, W = 3, 12, 33, 65
    g = np.random.Generator(np.random.PCG64(60))
    logits = torch.from_numpy(g.standard_normal((N, n_cls, H, W)).astype(np.float32)).to(dev)
    label = np.stack([bo.block_plane(61 + n, H, W, n_cls) for n in range(N)])
    label[0, :2, :3] = 255
    lab_t = torch.from_numpy(label).to(dev)
    groups = [4, 0, 4]
    _, hist = ops.argmax_confusion_grouped(logits, lab_t, groups, 5, H, W, want_pred=False)
    pred, none = ops.argmax_confusion_grouped(logits, None, groups, 5, H, W)
    assert none is None
    for radii in ((1, 2, 4, 8), (32,)):
        _, banded = ops.label_bands(lab_t, radii, pred=pred, groups=groups, n_groups=5, n_cls=n_cls)
        assert tuple(banded.shape) == (5, len(radii) + 1, n_cls, n_cls)
        assert torch.equal(banded.sum(1), hist) and int(hist.sum()) > 0
        want = bo.banded_hist(label, pred.cpu().numpy(), bo.label_bands(label, radii, n_cls, fast=True), groups, 5, len(radii), n_cls)
        assert np.array_equal(banded.cpu().numpy(), want)


def test_with_the_model(dev, golden, manifest):
    """EvalByBand on the small PSPNet and the samples of test_gpu_eval_grouped: its total is EvalByDistance's histogram on the same loader,
    and alter_res_batch_bands is alter_res_batch_pred followed by ops.label_bands."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from test_gpu_eval_grouped import _g7_samples, labels
    from test_gpu_models import _psp

    hr, lr = _psp(manifest, dev, False), _psp(manifest, dev, True)
    by_d, keys = _g7_samples(golden, "psp")
    loader = [by_d[4][0] + (4,), keys[0], by_d[11][0] + (torch.tensor([11]),), by_d[1][0] + (1,)]
    radii = (1, 2, 4, 8)
    with torch.no_grad():
        plain = ev.EvalByDistance(scale=0.5, gop=12)(hr, torch.nn.DataParallel(lr), loader, 12)
        table = ev.EvalByBand(scale=0.5, gop=12, radii=radii)(hr, torch.nn.DataParallel(lr), loader, 12)
        assert isinstance(table, ev.BandTable) and tuple(table.hist.shape) == (12, 5, 12, 12) and table.radii == radii
        assert torch.equal(table.total().hist, plain.hist) and int(plain.hist.sum()) > 0
        assert np.array_equal(table.as_array()[-1], plain.as_array(), equal_nan=True) and table.as_array().shape == (6, 13)
        assert int(table.band(0).hist.sum()) > 0 and int(table.hist[[2, 3, 5]].sum()) == 0
        H, W = 48, 64
        clip = synth.make_clip(6, H, W, gop=4)
        frames, mvs = torch.from_numpy(clip["frames"]).to(dev), torch.from_numpy(clip["mv"]).to(dev)
        label = labels(168, 3, H, W, 12).to(dev)
        ref_p = ops.to_nhwc(hr(frames[0:1])[-1])[0]
        groups = [1, 2, 3]
        pred, hist = ev.alter_res_batch_bands(lr, [ref_p] * 3, frames[1:4], mvs[1:4], label, radii, groups=groups, n_groups=4)
        pred_p, _ = ev.alter_res_batch_pred(lr, [ref_p] * 3, frames[1:4], mvs[1:4], 0.5)
        _, hist_p = ops.label_bands(label, radii, pred=pred_p, groups=groups, n_groups=4, n_cls=12)
        assert torch.equal(pred, pred_p) and torch.equal(hist, hist_p) and tuple(hist.shape) == (4, 5, 12, 12)
        _, plain_h = ev.alter_res_batch_pred(lr, [ref_p] * 3, frames[1:4], mvs[1:4], 0.5, labels=label, groups=groups, n_groups=4)
        assert torch.equal(hist.sum(1), plain_h)
        again = ev.alter_res_batch_bands(lr, [ref_p] * 3, frames[1:4], mvs[1:4], label, radii, hist=hist, groups=groups, n_groups=4)[1]
        assert again is hist and torch.equal(hist, 2 * hist_p)
