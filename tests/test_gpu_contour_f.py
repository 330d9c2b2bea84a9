"""GPU tests of the contour F-measure counts (ops.contour_f, csrc/bands.hip) against tests/contour_f_oracle.py, which states the definition
without the kernels' tiles, lists and rings, and of what is built on them (evaluation.alter_res_batch_contour, evaluation.EvalByContour).
Labels and predictions come from numpy, so only bands.hip runs, except where the tail or the model is the point.  Every comparison is of
integers and exact.

The kernels' sizes the shapes aim at: tiles of 64 x 64 pixels, with a halo of one pixel in the mark launch and of R <= 32 marks in the
match launch; a wave takes 64 contour pixels of a tile's list at a time."""
import ctypes

import numpy as np
import pytest
import torch

import bands_oracle as bo
import contour_f_oracle as co

pytestmark = pytest.mark.gpu

GUARD = 0xAB
TILE = 64


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


def _shifted(label, by, fill=1):
    return np.where(label == 255, fill, np.roll(label, by, (-2, -1))).astype(np.int32)


def run(dev, label, pred, radii, n_cls, groups=None, n_groups=1, ignore=255, lplane=True, pplane=True, counts0=None, pad=(0, 0)):
    """One guarded call: guard bytes behind both planes (row padding included), guard groups either side of counts, guard bytes behind a
    workspace of the exact size, the inputs compared after the call.  ``pad``: extra bytes per row and extra rows per image of the planes.
    -> (counts int64, label plane | None, prediction plane | None), numpy."""
    from arseg_amd import _lib, ops

    N, H, W = label.shape
    lab_t, pred_t = torch.from_numpy(label).to(dev), torch.from_numpy(pred).to(dev)
    grp_t = groups if groups is None or isinstance(groups, list) else torch.tensor(groups, dtype=torch.int32, device=dev)
    grp_keep = None if not torch.is_tensor(grp_t) else grp_t.clone()
    need = _lib.load().arseg_contour_f_workspace_bytes(N, H, W)
    assert need == (2 * N * H * W + 15) // 16 * 16
    ws_all = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=dev)
    pitch, rows = W + pad[0], H + pad[1]
    alls, views = [], []
    for want in (lplane, pplane):
        a = torch.full((N * rows * pitch + 64,), GUARD, dtype=torch.uint8, device=dev) if want else None
        alls.append(a)
        views.append(a[:N * rows * pitch].view(N, rows, pitch)[:, :H, :W] if want else None)
    nb = len(radii) + 1
    counts_all = torch.full((n_groups + 2, 2, nb, n_cls), -7, dtype=torch.int64, device=dev)
    counts_t = counts_all[1:n_groups + 1]
    counts_t.copy_(torch.zeros_like(counts_t) if counts0 is None else torch.from_numpy(counts0).to(dev))
    got_c, got_l, got_p = ops.contour_f(lab_t, pred_t, radii, groups=grp_t, n_groups=n_groups, n_cls=n_cls, counts=counts_t, ignore_label=ignore,
                                        label_match_out=views[0], pred_match_out=views[1], workspace=ws_all[:need])
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
        assert bool((seen == GUARD).all()), "a match plane's guard, padding included"
    assert got_c.data_ptr() == counts_t.data_ptr()
    assert bool((counts_all[0] == -7).all()) and bool((counts_all[-1] == -7).all()), "counts' guard groups"
    return counts_t.cpu().numpy(), *(None if v is None else v.cpu().numpy() for v in views)


def _differ(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} {what} differ, the first at (n, y, x) = {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def check(dev, label, pred, radii, n_cls, groups=None, n_groups=1, ignore=255, want_planes=None, **kw):
    """``run`` against the oracle -> (counts, label plane, prediction plane).  ``want_planes``: (label marks, prediction marks, label
    bands, prediction bands) when the test has them in closed form."""
    if want_planes is None:
        want_planes = co.planes(label, pred, radii, n_cls, ignore, fast=True)
    got_c, got_l, got_p = run(dev, label, pred, radii, n_cls, groups=groups, n_groups=n_groups, ignore=ignore, **kw)
    if got_l is not None:
        _differ(got_l, want_planes[2], "label bands")
    if got_p is not None:
        _differ(got_p, want_planes[3], "prediction bands")
    ids = [0] * label.shape[0] if groups is None else [int(g) for g in groups]
    want_c = co.counts(label, pred, *want_planes, ids, n_groups, len(radii), n_cls, ignore)
    if kw.get("counts0") is not None:
        want_c = want_c + kw["counts0"]
    assert np.array_equal(got_c, want_c)
    return got_c, got_l, got_p


def test_hand_cases(dev):
    """The hand cases of one shape and set of radii as the frames of one call, against the literals."""
    sets = {}
    for h in co.HAND:
        sets.setdefault((np.array(h[1]).shape, h[3]), []).append(h)
    assert len(sets[((5, 5), (0, 1))]) == 3
    for (shape, radii), cases in sets.items():
        label = np.stack([np.array(h[1], dtype=np.int64) for h in cases])
        pred = np.stack([np.array(h[2], dtype=np.int32) for h in cases])
        want = tuple(np.stack([np.array(h[i]) for h in cases]) for i in (4, 5, 6, 7))
        got, _, _ = check(dev, label, pred, radii, co.HAND_N_CLS, groups=list(range(len(cases))), n_groups=len(cases), want_planes=want)
        for n, h in enumerate(cases):
            assert np.array_equal(got[n], co.sparse(h[8], len(radii))), h[0]


# W = 1, 5, 63, 64, 65, 129, 200; H = 1, 2, 5, 33, 65, 131; one below, at and one above the tile in both
SHAPES = [(33, 1), (131, 5), (2, 63), (1, 64), (33, 65), (65, 129), (5, 200), (131, 200), (TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1), (1, 1)]


@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
def test_shapes(dev, H, W):
    n_cls = 7
    label = np.stack([bo.block_plane(100 + H, H, W, n_cls), bo.noise_plane(200 + W, H, W, n_cls), bo.block_plane(300 + W, H, W, n_cls, cell=53),
                      bo.block_plane(400 + W, H, W, n_cls, cell=29)])
    pred = np.stack([_preds(3, label[0], n_cls), _preds(4, label[1], n_cls), _shifted(label[2], (1, 2), 2), _shifted(label[3], (-6, 7))])
    for radii in ((1, 2, 4, 8), (3, 10, 32)):
        check(dev, label, pred, radii, n_cls, groups=[1, 0, 1, 0], n_groups=2)


def _lone_planes(H, W, lones_l, lones_p, radii):
    """Planes of class 0 with single pixels of class 2 -- ``lones_l`` on the labels, ``lones_p`` on the predictions -- and what the entry
    point gives on them, in closed form: a lone pixel is a contour pixel of class 2, its neighbours inside the image are contour pixels of
    class 0, and nothing else is one; a band is that of the least squared distance between two such short lists.
    -> (label, prediction, (label marks, prediction marks, label bands, prediction bands))."""
    def marked(lones):
        m = {}
        for y, x in lones:
            for qy in range(max(y - 1, 0), min(y + 2, H)):
                for qx in range(max(x - 1, 0), min(x + 2, W)):
                    m.setdefault((qy, qx), 0)
        for at in lones:
            m[at] = 2
        return m

    def plane(lones, dtype):
        p = np.zeros((H, W), dtype)
        for at in lones:
            p[at] = 2
        return p

    def banded(mine, theirs):
        marks, band = np.full((H, W), -1, np.int64), np.full((H, W), 255, np.uint8)
        for (y, x), c in mine.items():
            d2 = min(((y - ty) ** 2 + (x - tx) ** 2 for (ty, tx), tc in theirs.items() if tc == c), default=co.INF)
            marks[y, x], band[y, x] = c, sum(d2 > r * r for r in radii)
        return marks, band

    ml, mp = marked(lones_l), marked(lones_p)
    (a, b), (c, d) = banded(ml, mp), banded(mp, ml)
    return plane(lones_l, np.int64), plane(lones_p, np.int32), (a, c, b, d)


@pytest.mark.parametrize("r", [1, 5, 10, 32])
def test_pairs_at_exactly_r_and_just_above(dev, r):
    """One pixel of class 2 per frame and plane, the two at a squared distance of exactly r * r -- (r, 0), (0, r) and the multiples of
    (3, 4) -- or just above it -- one more in the other coordinate, (4, 4) against 5, and a lone target at Chebyshev distance r + 1, outside
    the staged halo --, placed across the tile seam in x, in y and at the tile corner, and with the label's pixel on the first and last row
    and column.  Within r is band 0, beyond it unmatched, whichever seam lies between; both whole planes are compared with the closed
    form, and the pair is named."""
    H = W = 2 * TILE + 3
    exact, above = [(r, 0), (0, r)], [(r, 1), (1, r), (r + 1, 0), (0, r + 1)]
    if r % 5 == 0:
        k = r // 5
        exact.append((3 * k, 4 * k))
        above.append((3 * k, 4 * k + 1))
    if r == 5:
        above.append((4, 4))
    assert all(dy * dy + dx * dx == r * r for dy, dx in exact) and all(dy * dy + dx * dx > r * r for dy, dx in above)
    # (the label's pixel, the sign of the offset): at (63, .) / (., 63) any offset of a pixel or more crosses the seam at 64
    anchors = [((20, TILE - 1), 1), ((TILE - 1, 20), 1), ((TILE - 1, TILE - 1), 1), ((0, 30), 1), ((30, 0), 1), ((H - 1, 90), -1), ((90, W - 1), -1),
               ((TILE, TILE), -1)]
    frames, named = [], []
    for (ay, ax), sign in anchors:
        for (dy, dx), band in [(o, 0) for o in exact] + [(o, 1) for o in above]:
            by, bx = ay + sign * dy, ax + sign * dx
            assert 0 <= by < H and 0 <= bx < W
            frames.append(_lone_planes(H, W, [(ay, ax)], [(by, bx)], (r,)))
            named.append(((ay, ax), (by, bx), band))
    label, pred = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    want = tuple(np.stack([f[2][i] for f in frames]) for i in range(4))
    got_c, got_l, got_p = check(dev, label, pred, (r,), 3, want_planes=want)
    for n, (a, b, band) in enumerate(named):
        assert got_l[n][a] == band and got_p[n][b] == band, (a, b)
    assert int(got_c[0, 0, 0, 2]) == int(got_c[0, 1, 0, 2]) == len(anchors) * len(exact)
    assert int(got_c[0, 0, 1, 2]) == int(got_c[0, 1, 1, 2]) == len(anchors) * len(above)


def test_a_nearer_target_in_a_later_ring_across_a_seam(dev):
    """Targets at (5, 5), Chebyshev ring 5, squared distance 50, and at (0, 6), ring 6, squared distance 36, either side of a tile seam of the
    label's pixel: within 6.  Then the nearer one alone, the farther one alone (within 8) and none."""
    H, W, radii = TILE + 20, 2 * TILE, (6, 7, 8)
    frames = []
    for a in ((30, 60), (60, 30), (62, 61), (0, 0)):
        both = [(a[0] + 5, a[1] + 5), (a[0], a[1] + 6)]
        for targets, band in ((both, 0), (both[1:], 0), (both[:1], 2), ([], 3)):
            frames.append((a, band) + _lone_planes(H, W, [a], targets, radii))
    label, pred = np.stack([f[2] for f in frames]), np.stack([f[3] for f in frames])
    want = tuple(np.stack([f[4][i] for f in frames]) for i in range(4))
    _, got_l, _ = check(dev, label, pred, radii, 3, want_planes=want)
    for n, f in enumerate(frames):
        assert got_l[n][f[0]] == f[1], (n, f[0])


def test_plane_pitch_and_image_stride(dev):
    n_cls, radii = 5, (1, 2, 4, 8)
    label = np.stack([bo.block_plane(20, 37, 70, n_cls), bo.noise_plane(21, 37, 70, n_cls)])
    pred = _preds(4, label, n_cls)
    check(dev, label, pred, radii, n_cls, pad=(7, 0))
    check(dev, label, pred, radii, n_cls, pad=(0, 3))
    check(dev, label, pred, (0, 20), n_cls, pad=(13, 2))


def test_unlike_frames_in_both_orders(dev):
    """Frames must not reach each other through the halo: the last rows of one frame and the first of the next are neighbours in memory."""
    n_cls, radii = 5, (2, 32)
    a, b = bo.block_plane(22, 70, 130, n_cls, cell=30), bo.noise_plane(23, 70, 130, n_cls)
    pa, pb = _shifted(a, (3, -4)), _preds(6, b, n_cls, wrong=0.5)
    c1, l1, p1 = check(dev, np.stack([a, b]), np.stack([pa, pb]), radii, n_cls, groups=[0, 1], n_groups=2)
    c2, l2, p2 = check(dev, np.stack([b, a]), np.stack([pb, pa]), radii, n_cls, groups=[1, 0], n_groups=2)
    assert np.array_equal(l1[0], l2[1]) and np.array_equal(l1[1], l2[0]) and np.array_equal(p1[0], p2[1]) and np.array_equal(c1, c2)
    assert not np.array_equal(c1[0], c1[1])


def _raw(dev, label, pred, radii, n_cls, lplane, pplane, counts):
    """The entry point through ctypes, any output NULL: -> the status."""
    from arseg_amd import _lib

    lib = _lib.load()
    N, H, W = label.shape
    ws = torch.zeros((lib.arseg_contour_f_workspace_bytes(N, H, W),), dtype=torch.uint8, device=dev)

    def ptr(t):
        return ctypes.c_void_p(0 if t is None else t.data_ptr())

    status = lib.arseg_contour_f_fwd(ptr(label), ptr(pred), ptr(None), (ctypes.c_int * len(radii))(*radii), len(radii), ptr(lplane), W, H * W,
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
    assert int(counts[1].sum()) == 0 and (n_cls == 1) == (int(counts.sum()) == 0) and (n_cls == 1) == (int(lband.min()) == 255)
    # a second call accumulates
    twice, _, _ = check(dev, label, pred, radii, n_cls, groups=[2, 1, 0, 1, 2], n_groups=3, counts0=counts)
    assert n_cls == 1 or int(twice.sum()) > int(counts.sum())
    # a NULL group, one set of counts
    one, _, _ = check(dev, label, pred, radii, n_cls)
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
    c0, l0, p0 = ops.contour_f(lab_t, pred_t, radii, n_cls=n_cls)
    assert l0 is None and p0 is None and np.array_equal(c0.cpu().numpy(), one)
    c1, l1, p1 = ops.contour_f(lab_t, pred_t, radii, counts=c0, label_match_out=True, pred_match_out=True)
    assert c1 is c0 and np.array_equal(c0.cpu().numpy(), 2 * one)
    assert np.array_equal(l1.cpu().numpy(), lband) and np.array_equal(p1.cpu().numpy(), pband)


def test_totals_at_radius_one_are_the_first_band_of_boundary_iou(dev):
    """On planes without 255 the contour pixels are the pixels at trimap distance 1: summed over the bands, rows 0 and 1 are rows 0 and 1
    of band 0 of ops.boundary_iou at radius 1 without the border term -- other code, another distance pass."""
    from arseg_amd import ops

    N, n_cls, H, W = 3, 12, 70, 131
    g = np.random.Generator(np.random.PCG64(64))
    label = np.stack([np.kron(g.integers(0, n_cls, (H // 9 + 1, W // 9 + 1)), np.ones((9, 9), np.int64))[:H, :W] for _ in range(N)])
    pred = np.where(g.random(label.shape) < 0.1, g.integers(0, n_cls, label.shape), np.roll(label, (2, 1), (1, 2))).astype(np.int32)
    assert int(label.max()) < n_cls and int(pred.min()) >= 0 and int(pred.max()) < n_cls
    lab_t, pred_t = torch.from_numpy(label).to(dev), torch.from_numpy(pred).to(dev)
    groups = [4, 0, 4]
    counts, _, _ = ops.contour_f(lab_t, pred_t, (1,), groups=groups, n_groups=5, n_cls=n_cls)
    other, _, _ = ops.boundary_iou(lab_t, pred_t, (1,), groups=groups, n_groups=5, n_cls=n_cls, border=False)
    assert tuple(counts.shape) == (5, 2, 2, n_cls) and int(counts.sum()) > 0
    assert torch.equal(counts.sum(2)[:, 0], other[:, 0, 0]) and torch.equal(counts.sum(2)[:, 1], other[:, 1, 0])
    want, _, _ = co.contour_f(label, pred, (1,), n_cls, groups=groups, n_groups=5, fast=True)
    assert np.array_equal(counts.cpu().numpy(), want)


def test_graph_capture_replayed_on_refilled_inputs(dev):
    from arseg_amd import _lib, ops

    n_cls, radii, N, H, W = 6, (2, 8, 19), 2, 70, 131
    sets = []
    for s in (40, 50):
        label = np.stack([bo.block_plane(s, H, W, n_cls, cell=13), bo.noise_plane(s + 1, H, W, n_cls)])
        sets.append((label, _preds(s + 2, label, n_cls), np.array([1, 0] if s == 40 else [0, 2], np.int32)))
    lab_t, pred_t = torch.from_numpy(sets[0][0]).to(dev), torch.from_numpy(sets[0][1]).to(dev)
    grp_t = torch.from_numpy(sets[0][2]).to(dev)
    l_t, p_t = torch.zeros((N, H, W), dtype=torch.uint8, device=dev), torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    counts_t = torch.zeros((3, 2, len(radii) + 1, n_cls), dtype=torch.int64, device=dev)
    ws = torch.zeros((_lib.load().arseg_contour_f_workspace_bytes(N, H, W),), dtype=torch.uint8, device=dev)

    def call():
        ops.contour_f(lab_t, pred_t, radii, groups=grp_t, n_groups=3, counts=counts_t, label_match_out=l_t, pred_match_out=p_t, workspace=ws)

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
        want, bl, bp = co.contour_f(label, pred, radii, n_cls, groups=ids.tolist(), n_groups=3, fast=True)
        assert np.array_equal(l_t.cpu().numpy(), bl) and np.array_equal(p_t.cpu().numpy(), bp)
        assert np.array_equal(counts_t.cpu().numpy(), want)


def test_with_the_model(dev, golden, manifest):
    """EvalByContour on the small PSPNet and the samples of test_gpu_eval_grouped is alter_res_batch_pred's tail followed by ops.contour_f
    per sample, and alter_res_batch_contour is alter_res_batch_pred followed by ops.contour_f."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops, synth
    from test_gpu_eval_grouped import _g7_samples, labels
    from test_gpu_models import _psp

    hr, lr = _psp(manifest, dev, False), _psp(manifest, dev, True)
    by_d, keys = _g7_samples(golden, "psp")
    loader = [by_d[4][0] + (4,), keys[0], by_d[11][0] + (torch.tensor([11]),), by_d[1][0] + (1,)]
    with torch.no_grad():
        table = ev.EvalByContour(scale=0.5, gop=12)(hr, torch.nn.DataParallel(lr), loader, 12)
        size = loader[0][1].shape[-2:]
        assert isinstance(table, ev.ContourTable) and table.radii == (ops.contour_radius(*size),)
        assert tuple(table.counts.shape) == (12, 2, 2, 12) and table.as_array().shape == (1, 13)
        assert int(table.counts[[0, 1, 4, 11]].sum()) > 0 and int(table.counts[[2, 3, 5]].sum()) == 0
        wide = ev.EvalByContour(scale=0.5, gop=12, radii=(1, 2, 4, 8))(hr, torch.nn.DataParallel(lr), loader, 12)
        assert wide.radii == (1, 2, 4, 8) and torch.equal(wide.counts.sum(2), table.counts.sum(2))
        # the same samples by hand: the evaluator's logits through the tail's argmax, then ops.contour_f
        again = torch.zeros_like(wide.counts)
        e = ev.EvalByDistance(scale=0.5, gop=12)
        cache = [None, None]
        for sample in loader:
            label = sample[1].to(dev)
            if len(sample) == 3:
                out, groups = hr(sample[0].to(dev))[0], [0] * label.shape[0]
            else:
                out, groups = e._logits(hr, lr, sample[0], sample[3], sample[4], cache), e._groups(sample[5], label.shape[0])
            pred, _ = ops.argmax_confusion_grouped(out, None, groups, 12, label.shape[-2], label.shape[-1])
            ops.contour_f(label, pred, (1, 2, 4, 8), groups=groups, n_groups=12, counts=again)
            host = ev.contour_f_numpy(label.cpu().numpy(), pred.cpu().numpy(), (1, 2, 4, 8), 12)
            fresh, _, _ = ops.contour_f(label, pred, (1, 2, 4, 8), n_cls=12)
            assert np.array_equal(fresh[0].cpu().numpy(), host)
        assert torch.equal(again, wide.counts)
        H, W = 48, 64
        clip = synth.make_clip(6, H, W, gop=4)
        frames, mvs = torch.from_numpy(clip["frames"]).to(dev), torch.from_numpy(clip["mv"]).to(dev)
        label = labels(168, 3, H, W, 12).to(dev)
        ref_p = ops.to_nhwc(hr(frames[0:1])[-1])[0]
        groups, radii = [1, 2, 3], (1, 2, 4, 8)
        pred, counts = ev.alter_res_batch_contour(lr, [ref_p] * 3, frames[1:4], mvs[1:4], label, radii, groups=groups, n_groups=4)
        pred_p, _ = ev.alter_res_batch_pred(lr, [ref_p] * 3, frames[1:4], mvs[1:4], 0.5)
        counts_p, _, _ = ops.contour_f(label, pred_p, radii, groups=groups, n_groups=4, n_cls=12)
        assert torch.equal(pred, pred_p) and torch.equal(counts, counts_p) and tuple(counts.shape) == (4, 2, 5, 12)
        again = ev.alter_res_batch_contour(lr, [ref_p] * 3, frames[1:4], mvs[1:4], label, radii, counts=counts, groups=groups, n_groups=4)[1]
        assert again is counts and torch.equal(counts, 2 * counts_p)
        host = ev.contour_f_numpy(label.cpu().numpy(), pred.cpu().numpy(), radii, 12)
        assert np.array_equal(counts_p.sum(0).cpu().numpy(), host)
