"""GPU tests of the Boundary IoU counts (ops.boundary_iou, csrc/bands.hip) against tests/boundary_iou_oracle.py, which states the window
definition without the kernels' separable form, and of what is built on them (evaluation.alter_res_batch_boundary,
evaluation.EvalByBoundary).  Labels and predictions come from numpy, so only bands.hip runs, except where the tail or the model is the
point.  Every comparison is of integers and exact.

The kernels' sizes the shapes aim at: 64-pixel chunks and 1024-pixel segments of a row (the row launch), tiles of 64 x 64 pixels with a
halo of R <= 64 rows (the column launch)."""
import ctypes

import numpy as np
import pytest
import torch

import bands_oracle as bo
import boundary_iou_oracle as bio

pytestmark = pytest.mark.gpu

GUARD = 0xAB
TILE, SEG = 64, 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _preds(seed, label, n_cls, wrong=0.2, outside=2):
    """The labels with a share of other values, some of them outside [0, n_cls) (``outside`` = 0: none)."""
    g = np.random.Generator(np.random.PCG64(seed))
    other = g.integers(-outside, n_cls + outside, label.shape)
    return np.where(g.random(label.shape) < wrong, other, np.where(label == 255, 0, label)).astype(np.int32)


def run(dev, label, pred, radii, n_cls, groups=None, n_groups=1, ignore=255, border=1, lplane=True, pplane=True, counts0=None, pad=(0, 0)):
    """One guarded call: guard bytes behind both planes (row padding included), guard groups either side of counts, guard bytes behind a
    workspace of the exact size, the inputs compared after the call.  ``pad``: extra bytes per row and extra rows per image of the planes.
    -> (counts int64, label bands | None, prediction bands | None), numpy."""
    from arseg_amd import _lib, ops

    N, H, W = label.shape
    lab_t, pred_t = torch.from_numpy(label).to(dev), torch.from_numpy(pred).to(dev)
    grp_t = groups if groups is None or isinstance(groups, list) else torch.tensor(groups, dtype=torch.int32, device=dev)
    grp_keep = None if not torch.is_tensor(grp_t) else grp_t.clone()
    need = _lib.load().arseg_boundary_iou_workspace_bytes(N, H, W)
    assert need == (4 * N * H * W + 15) // 16 * 16
    ws_all = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=dev)
    pitch, rows = W + pad[0], H + pad[1]
    alls, views = [], []
    for want in (lplane, pplane):
        a = torch.full((N * rows * pitch + 64,), GUARD, dtype=torch.uint8, device=dev) if want else None
        alls.append(a)
        views.append(a[:N * rows * pitch].view(N, rows, pitch)[:, :H, :W] if want else None)
    nb = len(radii) + 1
    counts_all = torch.full((n_groups + 2, 3, nb, n_cls), -7, dtype=torch.int64, device=dev)
    counts_t = counts_all[1:n_groups + 1]
    counts_t.copy_(torch.zeros_like(counts_t) if counts0 is None else torch.from_numpy(counts0).to(dev))
    got_c, got_l, got_p = ops.boundary_iou(lab_t, pred_t, radii, groups=grp_t, n_groups=n_groups, n_cls=n_cls, counts=counts_t, ignore_label=ignore,
                                           border=bool(border), label_band_out=views[0], pred_band_out=views[1], workspace=ws_all[:need])
    torch.cuda.synchronize()
    assert bool((ws_all[need:] == GUARD).all()), "the workspace's guard"
    assert np.array_equal(lab_t.cpu().numpy(), label) and np.array_equal(pred_t.cpu().numpy(), pred)
    assert grp_keep is None or torch.equal(grp_keep, grp_t)
    for a, v, got in zip(alls, views, (got_l, got_p)):
        if a is None:
            assert got is None
            continue
        assert got.data_ptr() == v.data_ptr()
        seen = a.clone()
        seen[:N * rows * pitch].view(N, rows, pitch)[:, :H, :W] = GUARD
        assert bool((seen == GUARD).all()), "a band plane's guard, padding included"
    assert got_c.data_ptr() == counts_t.data_ptr()
    assert bool((counts_all[0] == -7).all()) and bool((counts_all[-1] == -7).all()), "counts' guard groups"
    return counts_t.cpu().numpy(), *(None if v is None else v.cpu().numpy() for v in views)


def _differ(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} {what} differ, the first at (n, y, x) = {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def check(dev, label, pred, radii, n_cls, groups=None, n_groups=1, ignore=255, border=1, want_planes=None, **kw):
    """``run`` against the oracle -> (counts, label bands, prediction bands)."""
    if want_planes is None:
        want_planes = bio.planes(label, pred, radii, n_cls, ignore, border, fast="minmax")
    got_c, got_l, got_p = run(dev, label, pred, radii, n_cls, groups=groups, n_groups=n_groups, ignore=ignore, border=border, **kw)
    if got_l is not None:
        _differ(got_l, want_planes[0], "label bands")
    if got_p is not None:
        _differ(got_p, want_planes[1], "prediction bands")
    ids = [0] * label.shape[0] if groups is None else [int(g) for g in groups]
    want_c = bio.counts(label, pred, want_planes[0], want_planes[1], ids, n_groups, len(radii), n_cls, ignore)
    if kw.get("counts0") is not None:
        want_c = want_c + kw["counts0"]
    assert np.array_equal(got_c, want_c)
    return got_c, got_l, got_p


def test_hand_cases(dev):
    """The hand cases of one shape and border as the frames of one call, against the literals."""
    sets = {}
    for h in bio.HAND:
        sets.setdefault((np.array(h[1]).shape, h[3]), []).append(h)
    assert len(sets[((5, 5), 0)]) == 4 and len(sets[((5, 5), 1)]) == 2
    for (shape, border), cases in sets.items():
        label = np.stack([np.array(h[1], dtype=np.int64) for h in cases])
        pred = np.stack([np.array(h[2], dtype=np.int32) for h in cases])
        want = (np.stack([bo.bands(np.array(h[4]), bio.RADII_HAND) for h in cases]), np.stack([bo.bands(np.array(h[5]), bio.RADII_HAND) for h in cases]))
        got, _, _ = check(dev, label, pred, bio.RADII_HAND, bio.HAND_N_CLS, groups=list(range(len(cases))), n_groups=len(cases), border=border,
                          want_planes=want)
        for n, h in enumerate(cases):
            assert np.array_equal(got[n], bio.sparse(h[6])), h[0]


# W = 1, 63, 64, 65, 129 and around a row segment; H = 1, 2, 33, 65, 131; one below, at and one above the tile in both; H or W below 2 R + 1
SHAPES = [(33, 1), (2, 63), (1, 64), (33, 65), (65, 129), (2, SEG - 1), (1, SEG), (131, SEG + 1), (TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1),
          (131, 5), (5, 200), (1, 1)]


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_shapes(dev, H, W):
    n_cls = 7
    label = np.stack([bo.block_plane(100 + H, H, W, n_cls), bo.noise_plane(200 + W, H, W, n_cls), bo.block_plane(300 + W, H, W, n_cls, cell=53)])
    pred = np.stack([_preds(3, label[0], n_cls), _preds(4, label[1], n_cls),
                     np.where(label[2] == 255, 2, np.roll(label[2], (1, 2), (0, 1))).astype(np.int32)])           # the labels shifted
    for radii in ((1, 2, 4, 8), (3, 33, 64)):
        for border in (0, 1):
            check(dev, label, pred, radii, n_cls, groups=[1, 0, 1], n_groups=2, border=border)


def _odd_pixel_distance(H, W, py, px):
    """D of a constant plane with one other pixel at (py, px): the Chebyshev distance to it, and 1 at the pixel itself."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.maximum(np.abs(yy - py), np.abs(xx - px))
    d[py, px] = 1
    return d


@pytest.mark.parametrize("r", [1, 32, 33, 64])
def test_pixels_at_exactly_r_and_r_plus_one(dev, r):
    """One differing pixel per frame and plane, placed on the first and last row and column, either side of a 64-lane chunk seam, a tile
    seam and a row-segment seam; frame n has it at spot n on the label plane and at another spot on the prediction plane (the first and
    the last frame on one plane only).  The pixels at Chebyshev distance exactly r of it are in band 0 and those at r + 1 are interior,
    horizontally, vertically and diagonally, whichever seam lies between -- both whole planes are compared with the closed form, and the
    probes are named."""
    H, W = 2 * TILE + 2, SEG + 70
    spots = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (TILE - 1, TILE - 1), (TILE, TILE), (TILE - 1, SEG - 1), (TILE, SEG), (2 * TILE - 1, 3 * 64),
             (1, SEG - 64)]
    N = len(spots)
    others = [spots[(n + 3) % N] for n in range(N)]
    label, pred = np.full((N, H, W), 3, np.int64), np.full((N, H, W), 3, np.int32)
    want_l, want_p = np.ones((N, H, W), np.uint8), np.ones((N, H, W), np.uint8)
    for n in range(N):
        if n != N - 1:
            label[n][spots[n]] = 255 if n % 2 else 5
            want_l[n] = _odd_pixel_distance(H, W, *spots[n]) > r
        if n != 0:
            pred[n][others[n]] = -1 if n % 2 else 4
            want_p[n] = _odd_pixel_distance(H, W, *others[n]) > r
    _, got_l, got_p = check(dev, label, pred, (r,), 6, border=0, want_planes=(want_l, want_p))
    for got, places, skip in ((got_l, spots, N - 1), (got_p, others, 0)):
        for n, (py, px) in enumerate(places):
            if n == skip:
                assert int(got[n].min()) == 1                                                # a constant plane without the border: all interior
                continue
            for sy, sx in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)):
                for dist, band in ((r, 0), (r + 1, 1)):
                    y, x = py + sy * dist, px + sx * dist
                    if 0 <= y < H and 0 <= x < W:
                        assert got[n, y, x] == band, (n, py, px, y, x)


def test_the_border_is_a_boundary(dev):
    H, W, radii, n_cls = 131, 200, (1, 8, 64), 3
    edge = bio.edge(H, W)
    # a constant plane: D is the distance to the edge
    label, pred = np.full((1, H, W), 2, np.int64), np.full((1, H, W), 2, np.int32)
    want = bo.bands(edge, radii)[None]
    got_c, got_l, got_p = check(dev, label, pred, radii, n_cls, border=1, want_planes=(want, want))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert got_l[0, y, x] == 0 and got_p[0, y, x] == 0
    assert got_l[0, 8, 100] == 2 and got_l[0, 7, 100] == 1 and got_l[0, 64, 100] == 3 and got_l[0, 63, 100] == 2 and got_l[0, 65, 100] == 3
    assert int(got_c[0, 0, 3, 2]) == (H - 128) * (W - 128) and int(got_c[0, :, :, 2].sum()) == 3 * H * W
    # without it the same plane is all interior
    none = np.full((1, H, W), 3, np.uint8)
    check(dev, label, pred, radii, n_cls, border=0, want_planes=(none, none))
    # a pixel whose nearest other byte and nearest edge tie: (10, 40) is 11 rows below the top edge's outside and 11 rows above (21, 40)
    label[0, 21, 40] = 0
    radii = (10, 11, 64)
    d = np.minimum(np.minimum(_odd_pixel_distance(H, W, 21, 40), 65), edge)
    assert d[10, 40] == 11 and edge[10, 40] == 11 and _odd_pixel_distance(H, W, 21, 40)[10, 40] == 11 and d[9, 40] == 10
    _, got_l, _ = check(dev, label, pred, radii, n_cls, border=1, want_planes=(bo.bands(d, radii)[None], bo.bands(np.minimum(edge, 65), radii)[None]))
    assert got_l[0, 10, 40] == 1 and got_l[0, 9, 40] == 0 and got_l[0, 11, 40] == 0 and got_l[0, 11, 20] == 2


@pytest.mark.parametrize("radii", [(1, 2, 4, 8), (3, 5, 32)], ids=str)
def test_without_border_the_label_plane_is_label_bands(dev, radii):
    from arseg_amd import ops

    n_cls = 7
    H, W = 70, SEG + 30
    label = np.stack([bo.block_plane(20, H, W, n_cls, cell=19), bo.noise_plane(21, H, W, n_cls)])
    pred = _preds(5, label, n_cls)
    groups = [1, 0]
    got_c, got_l, _ = check(dev, label, pred, radii, n_cls, groups=groups, n_groups=2, border=0)
    band, hist = ops.label_bands(torch.from_numpy(label).to(dev), radii, pred=torch.from_numpy(pred).to(dev), groups=groups, n_groups=2, n_cls=n_cls,
                                 band_out=True)
    assert np.array_equal(band.cpu().numpy(), got_l)
    assert np.array_equal(hist.sum(-1).cpu().numpy(), got_c[:, 0]) and int(got_c[:, 0].sum()) > 0


def test_bands_sum_to_the_grouped_tail(dev):
    """Summed over the bands, rows 0, 1 and 2 are the row sums, column sums and diagonal of ops.argmax_confusion_grouped's histogram on
    one-hot logits built from the same predictions."""
    from arseg_amd import ops

    N, n_cls, H, W = 3, 12, 33, 65
    label = np.stack([bo.block_plane(61 + n, H, W, n_cls) for n in range(N)])
    label[0, :2, :3] = 255
    pred = _preds(62, label, n_cls, wrong=0.3, outside=0)
    assert int(pred.min()) >= 0 and int(pred.max()) < n_cls
    logits = torch.nn.functional.one_hot(torch.from_numpy(pred).long(), n_cls).permute(0, 3, 1, 2).float().contiguous().to(dev)
    lab_t, pred_t = torch.from_numpy(label).to(dev), torch.from_numpy(pred).to(dev)
    groups = [4, 0, 4]
    tail_pred, hist = ops.argmax_confusion_grouped(logits, lab_t, groups, 5, H, W)
    assert torch.equal(tail_pred, pred_t) and int(hist.sum()) > 0
    for radii, border in (((1, 2, 4, 8), True), ((46,), True), ((64,), False)):
        counts, none_l, none_p = ops.boundary_iou(lab_t, pred_t, radii, groups=groups, n_groups=5, n_cls=n_cls, border=border)
        assert none_l is None and none_p is None and tuple(counts.shape) == (5, 3, len(radii) + 1, n_cls)
        total = counts.sum(2)
        assert torch.equal(total[:, 0], hist.sum(2)) and torch.equal(total[:, 1], hist.sum(1))
        assert torch.equal(total[:, 2], torch.diagonal(hist, dim1=1, dim2=2))
        want, _, _ = bio.boundary_iou(label, pred, radii, n_cls, border=border, groups=groups, n_groups=5, fast="minmax")
        assert np.array_equal(counts.cpu().numpy(), want)


def test_plane_pitch_and_image_stride(dev):
    n_cls, radii = 5, (1, 2, 4, 8)
    label = np.stack([bo.block_plane(20, 37, 70, n_cls), bo.noise_plane(21, 37, 70, n_cls)])
    pred = _preds(4, label, n_cls)
    check(dev, label, pred, radii, n_cls, pad=(7, 0))
    check(dev, label, pred, radii, n_cls, pad=(0, 3))
    check(dev, label, pred, (40,), n_cls, pad=(13, 2))


def test_unlike_frames_in_both_orders(dev):
    n_cls, radii = 5, (2, 40)
    a, b = bo.block_plane(22, 70, 130, n_cls, cell=30), bo.noise_plane(23, 70, 130, n_cls)
    pa, pb = _preds(5, a, n_cls), _preds(6, b, n_cls, wrong=0.5)
    c1, l1, p1 = check(dev, np.stack([a, b]), np.stack([pa, pb]), radii, n_cls, groups=[0, 1], n_groups=2)
    c2, l2, p2 = check(dev, np.stack([b, a]), np.stack([pb, pa]), radii, n_cls, groups=[1, 0], n_groups=2)
    assert np.array_equal(l1[0], l2[1]) and np.array_equal(l1[1], l2[0]) and np.array_equal(p1[0], p2[1]) and np.array_equal(c1, c2)
    assert not np.array_equal(c1[0], c1[1])


def _raw(dev, label, pred, radii, n_cls, lplane, pplane, counts):
    """The entry point through ctypes, any output NULL: -> the status."""
    from arseg_amd import _lib

    lib = _lib.load()
    N, H, W = label.shape
    ws = torch.zeros((lib.arseg_boundary_iou_workspace_bytes(N, H, W),), dtype=torch.uint8, device=dev)

    def ptr(t):
        return ctypes.c_void_p(0 if t is None else t.data_ptr())

    status = lib.arseg_boundary_iou_fwd(ptr(label), ptr(pred), ptr(None), (ctypes.c_int * len(radii))(*radii), len(radii), 1, ptr(lplane), W, H * W,
                                        ptr(pplane), W, H * W, ptr(counts), N, 1, n_cls, H, W, 255, ptr(ws), ws.numel(),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status


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
    counts, lband, pband = check(dev, label, pred, radii, n_cls, groups=ids, n_groups=3)
    conf = bo.confusion(label[[0, 2, 4]], pred[[0, 2, 4]], n_cls)
    assert int(counts[1].sum()) == 0 and int(counts[:, 0].sum()) == int(counts[:, 1].sum()) == int(conf.sum()) and int(counts[:, 2].sum()) == int(np.trace(conf))
    # a second call accumulates
    twice, _, _ = check(dev, label, pred, radii, n_cls, groups=[2, 1, 0, 1, 2], n_groups=3, counts0=counts)
    assert int(twice.sum()) > int(counts.sum())
    # a NULL group, one set of counts
    one, _, _ = check(dev, label, pred, radii, n_cls)
    assert np.array_equal(one[0, 0].sum(0), bo.confusion(label, pred, n_cls).sum(1))
    # each plane NULL in turn, both NULL
    for lp, pp in ((False, True), (True, False), (False, False)):
        again, l, p = check(dev, label, pred, radii, n_cls, lplane=lp, pplane=pp)
        assert np.array_equal(again, one) and (l is None) == (not lp) and (p is None) == (not pp)
    # counts NULL: the planes alone, through the entry point itself
    lab_t, pred_t = torch.from_numpy(label).to(dev), torch.from_numpy(pred).to(dev)
    l_t, p_t = torch.full((N, H, W), 9, dtype=torch.uint8, device=dev), torch.full((N, H, W), 9, dtype=torch.uint8, device=dev)
    assert _raw(dev, lab_t, pred_t, radii, n_cls, l_t, p_t, None) == 0
    assert np.array_equal(l_t.cpu().numpy(), lband) and np.array_equal(p_t.cpu().numpy(), pband)
    p_t.fill_(9)
    assert _raw(dev, lab_t, pred_t, radii, n_cls, None, p_t, None) == 0 and np.array_equal(p_t.cpu().numpy(), pband)
    # the defaults allocate: the stream's workspace, fresh counts, the planes asked for
    c0, l0, p0 = ops.boundary_iou(lab_t, pred_t, radii, n_cls=n_cls)
    assert l0 is None and p0 is None and np.array_equal(c0.cpu().numpy(), one)
    c1, l1, p1 = ops.boundary_iou(lab_t, pred_t, radii, counts=c0, label_band_out=True, pred_band_out=True)
    assert c1 is c0 and np.array_equal(c0.cpu().numpy(), 2 * one)
    assert np.array_equal(l1.cpu().numpy(), lband) and np.array_equal(p1.cpu().numpy(), pband)


def test_graph_capture_replayed_on_refilled_inputs(dev):
    from arseg_amd import _lib, ops

    n_cls, radii, N, H, W = 6, (2, 8, 46), 2, 70, 131
    sets = []
    for s in (40, 50):
        label = np.stack([bo.block_plane(s, H, W, n_cls, cell=13), bo.noise_plane(s + 1, H, W, n_cls)])
        sets.append((label, _preds(s + 2, label, n_cls), np.array([1, 0] if s == 40 else [0, 2], np.int32)))
    lab_t, pred_t = torch.from_numpy(sets[0][0]).to(dev), torch.from_numpy(sets[0][1]).to(dev)
    grp_t = torch.from_numpy(sets[0][2]).to(dev)
    l_t, p_t = torch.zeros((N, H, W), dtype=torch.uint8, device=dev), torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    counts_t = torch.zeros((3, 3, len(radii) + 1, n_cls), dtype=torch.int64, device=dev)
    ws = torch.zeros((_lib.load().arseg_boundary_iou_workspace_bytes(N, H, W),), dtype=torch.uint8, device=dev)

    def call():
        ops.boundary_iou(lab_t, pred_t, radii, groups=grp_t, n_groups=3, counts=counts_t, label_band_out=l_t, pred_band_out=p_t, workspace=ws)

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
        l_t.fill_(9)
        p_t.fill_(9)
        counts_t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want, bg, bp = bio.boundary_iou(label, pred, radii, n_cls, groups=ids.tolist(), n_groups=3, fast="minmax")
        assert np.array_equal(l_t.cpu().numpy(), bg) and np.array_equal(p_t.cpu().numpy(), bp)
        assert np.array_equal(counts_t.cpu().numpy(), want)


def test_with_the_model(dev, golden, manifest):
    """EvalByBoundary on the small PSPNet and the samples of test_gpu_eval_grouped: its iou() is EvalByDistance's on the same loader, and
    alter_res_batch_boundary is alter_res_batch_pred followed by ops.boundary_iou."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from test_gpu_eval_grouped import _g7_samples, labels
    from test_gpu_models import _psp

    hr, lr = _psp(manifest, dev, False), _psp(manifest, dev, True)
    by_d, keys = _g7_samples(golden, "psp")
    loader = [by_d[4][0] + (4,), keys[0], by_d[11][0] + (torch.tensor([11]),), by_d[1][0] + (1,)]
    with torch.no_grad():
        plain = ev.EvalByDistance(scale=0.5, gop=12)(hr, torch.nn.DataParallel(lr), loader, 12)
        table = ev.EvalByBoundary(scale=0.5, gop=12)(hr, torch.nn.DataParallel(lr), loader, 12)
        size = loader[0][1].shape[-2:]
        assert isinstance(table, ev.BoundaryTable) and table.radii == (ops.boundary_radius(*size),) and table.border is True
        assert tuple(table.counts.shape) == (12, 3, 2, 12)
        total = table.counts.sum(2)
        assert torch.equal(total[:, 0], plain.hist.sum(2)) and torch.equal(total[:, 1], plain.hist.sum(1)) and int(plain.hist.sum()) > 0
        assert torch.equal(total[:, 2], torch.diagonal(plain.hist, dim1=1, dim2=2))
        assert np.array_equal(table.iou().numpy(), plain.iou.numpy(), equal_nan=True)
        assert np.array_equal(table.as_array()[-1], plain.as_array(), equal_nan=True) and table.as_array().shape == (2, 13)
        assert int(table.counts[:, 2, 0].sum()) > 0 and int(table.counts[[2, 3, 5]].sum()) == 0
        wide = ev.EvalByBoundary(scale=0.5, gop=12, radii=(1, 2, 4, 8), border=False)(hr, torch.nn.DataParallel(lr), loader, 12)
        assert wide.radii == (1, 2, 4, 8) and wide.border is False and torch.equal(wide.counts.sum(2), total)
        H, W = 48, 64
        clip = synth.make_clip(6, H, W, gop=4)
        frames, mvs = torch.from_numpy(clip["frames"]).to(dev), torch.from_numpy(clip["mv"]).to(dev)
        label = labels(168, 3, H, W, 12).to(dev)
        ref_p = ops.to_nhwc(hr(frames[0:1])[-1])[0]
        groups, radii = [1, 2, 3], (1, 2, 4, 8)
        pred, counts = ev.alter_res_batch_boundary(lr, [ref_p] * 3, frames[1:4], mvs[1:4], label, radii, groups=groups, n_groups=4)
        pred_p, _ = ev.alter_res_batch_pred(lr, [ref_p] * 3, frames[1:4], mvs[1:4], 0.5)
        counts_p, _, _ = ops.boundary_iou(label, pred_p, radii, groups=groups, n_groups=4, n_cls=12)
        assert torch.equal(pred, pred_p) and torch.equal(counts, counts_p) and tuple(counts.shape) == (4, 3, 5, 12)
        _, plain_h = ev.alter_res_batch_pred(lr, [ref_p] * 3, frames[1:4], mvs[1:4], 0.5, labels=label, groups=groups, n_groups=4)
        assert torch.equal(counts.sum(2)[:, 0], plain_h.sum(2)) and torch.equal(counts.sum(2)[:, 2], torch.diagonal(plain_h, dim1=1, dim2=2))
        again = ev.alter_res_batch_boundary(lr, [ref_p] * 3, frames[1:4], mvs[1:4], label, radii, counts=counts, groups=groups, n_groups=4)[1]
        assert again is counts and torch.equal(counts, 2 * counts_p)
        host = ev.boundary_iou_numpy(label.cpu().numpy(), pred.cpu().numpy(), radii, 12)
        assert np.array_equal(counts_p.sum(0).cpu().numpy(), host)
