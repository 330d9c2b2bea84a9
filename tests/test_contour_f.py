"""CPU-side checks of the contour F-measure counts (include/arseg_hip.h, arseg_contour_f_fwd): the hand cases' literal marks, bands and
counts, the host form evaluation.contour_f_numpy (per-class dilation by the disc) against the oracle's direct definition, the contour pixels
against the trimap distance D == 1, ContourTable's arithmetic, every argument the entry point refuses before a launch, the workspace size,
and header, binding and exports in step.  All equalities are exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bands_oracle as bo
import contour_f_oracle as co
import rle_oracle
from conftest import ROOT

RADII = [(0,), (1, 2, 4, 8), (3, 10, 32), (32,)]


@pytest.mark.parametrize("name,label,pred,radii,want_ml,want_mp,want_bl,want_bp,want_counts", co.HAND, ids=co.HAND_IDS)
def test_hand_cases_have_the_written_marks_bands_and_counts(name, label, pred, radii, want_ml, want_mp, want_bl, want_bp, want_counts):
    from arseg_amd import evaluation as ev

    lab, prd = np.array(label, dtype=np.int64), np.array(pred, dtype=np.int32)
    want = co.sparse(want_counts, len(radii))
    for fast in (False, True):
        ml, mp, bl, bp = co.planes(lab[None], prd[None], radii, co.HAND_N_CLS, fast=fast)
        assert ml[0].tolist() == want_ml and mp[0].tolist() == want_mp, fast
        assert bl[0].tolist() == want_bl and bp[0].tolist() == want_bp, fast
        got, _, _ = co.contour_f(lab[None], prd[None], radii, co.HAND_N_CLS, fast=fast)
        assert np.array_equal(got[0], want), fast
    host = ev.contour_f_numpy(lab, prd, radii, co.HAND_N_CLS)
    assert host.dtype == np.int64 and np.array_equal(host, want)


def test_hand_cases_say_what_they_are_there_for():
    by = {h[0]: h for h in co.HAND}
    assert by["lone-pixels-offset-3-4"][6][1][1] == 1 and by["lone-pixels-offset-3-4"][7][4][5] == 1                 # 16 < 25 <= 25
    assert by["lone-pixels-offset-4-4"][6][1][1] == 1 and len(by["lone-pixels-offset-4-4"][3]) == 1                   # unmatched: 32 > 25
    assert by["nearer-target-in-a-later-ring"][6][1][1] == 0                                                          # 36, not 50
    assert by["void-block"][4][0][1] == -1 and by["void-block"][7][1][2] == 1 and by["void-block"][6][1][3] == 1
    one = by["class-on-one-plane-only"]
    c = co.sparse(one[8], 2)
    assert c[0, :, 3].sum() == 0 and c[1, :2, 3].sum() == 0 and c[1, 2, 3] == 4
    # and the host form says the same of them: the lone label pixel's class (its mark at (1, 1)) counts once on row 0, in that band
    from arseg_amd import evaluation as ev

    def host(name):
        h = by[name]
        return ev.contour_f_numpy(np.array(h[1], dtype=np.int64), np.array(h[2], dtype=np.int32), h[3], co.HAND_N_CLS), h[4][1][1]

    for name, band in (("lone-pixels-offset-3-4", 1), ("lone-pixels-offset-4-4", 1), ("nearer-target-in-a-later-ring", 0)):
        got, cls = host(name)
        assert cls >= 0 and got[0, :, cls].tolist() == [int(k == band) for k in range(got.shape[1])], name
    got, _ = host("class-on-one-plane-only")
    assert got[0, :, 3].sum() == 0 and got[1, :, 3].tolist() == [0, 0, 4]


def _planes():
    """(name, labels [N,H,W] int64, predictions [N,H,W] int32, n_cls): void pixels and predictions outside the classes in each."""
    g = np.random.Generator(np.random.PCG64(90))

    def preds(label, n_cls, wrong=0.2):
        return np.where(g.random(label.shape) < wrong, g.integers(-2, n_cls + 2, label.shape), np.where(label == 255, 0, label)).astype(np.int32)

    def shifted(label, by=1):
        return np.where(label == 255, 1, np.roll(label, by, axis=-1)).astype(np.int32)

    noise = bo.noise_plane(91, 23, 37, 5)[None]
    blocks = np.stack([bo.block_plane(92, 40, 70, 6), bo.block_plane(93, 40, 70, 6, cell=17)])
    blobs = rle_oracle.blob_planes(94, 2, 40, 56, n_cls=19, cell=8).astype(np.int64)
    blobs[:, :3, 10:30] = 255
    row, col = bo.block_plane(96, 1, 90, 4, cell=20), bo.block_plane(97, 90, 1, 4, cell=20)
    return [("noise", noise, preds(noise, 5), 5), ("blocks", blocks, preds(blocks, 6), 6), ("blocks-shifted", blocks, shifted(blocks), 6),
            ("blobs", blobs, shifted(blobs), 19), ("blobs-shifted-far", blobs, shifted(blobs, 5), 19), ("one-row", row[None], preds(row, 4)[None], 4),
            ("one-column", col[None], preds(col, 4)[None], 4)]


_PLANES = _planes()


@pytest.mark.parametrize("radii", RADII, ids=str)
def test_numpy_form_equals_the_definition(radii):
    from arseg_amd import evaluation as ev

    for name, label, pred, n_cls in _PLANES:
        want, bl, bp = co.contour_f(label, pred, radii, n_cls, fast=True)
        got = ev.contour_f_numpy(label, pred, radii, n_cls)
        assert got.shape == (2, len(radii) + 1, n_cls) and np.array_equal(got, want[0]), name
        assert int(bl[bl != 255].max(initial=0)) <= len(radii) and int(bp[bp != 255].max(initial=0)) <= len(radii)
    for name, label, pred, _, _, _, _, _, _ in co.HAND:
        lab, prd = np.array(label, dtype=np.int64), np.array(pred, dtype=np.int32)
        want, _, _ = co.contour_f(lab[None], prd[None], radii, co.HAND_N_CLS)
        assert np.array_equal(ev.contour_f_numpy(lab, prd, radii, co.HAND_N_CLS), want[0]), name


@pytest.mark.parametrize("radii", RADII, ids=str)
def test_fast_form_equals_the_direct_definition(radii):
    """The form over the disc's offsets that the larger planes use, held to the minimum over all contour pixels of the other plane; and the
    host form's counts held to the direct definition's planes themselves, not only to the fast form's."""
    from arseg_amd import evaluation as ev
    from arseg_amd import ops

    assert ops.contour_radii(list(radii)) == radii
    for name, label, pred, n_cls in (_PLANES[0], (_PLANES[1][0], _PLANES[1][1][:1], _PLANES[1][2][:1], 6), (_PLANES[4][0], _PLANES[4][1][:1], _PLANES[4][2][:1], 19),
                                     _PLANES[5], _PLANES[6]):
        slow, fast = co.planes(label, pred, radii, n_cls), co.planes(label, pred, radii, n_cls, fast=True)
        for a, b in zip(slow, fast):
            assert np.array_equal(a, b), name
        want = co.counts(label, pred, *slow, [0] * label.shape[0], 1, len(radii), n_cls)
        assert np.array_equal(ev.contour_f_numpy(label, pred, radii, n_cls), want[0]), name


def test_contour_pixels_are_the_trimap_distance_one_on_void_free_planes():
    """Without 255 on a plane its contour pixels are exactly D(p) == 1 of the trimap bands; so rows 0 and 1 summed over the bands are the
    per-class counts of D == 1 on the respective plane."""
    from arseg_amd import evaluation as ev

    n_cls = 7
    blobs = rle_oracle.blob_planes(98, 2, 24, 31, n_cls=n_cls, cell=6).astype(np.int64)
    g = np.random.Generator(np.random.PCG64(99))
    noise = g.integers(0, n_cls, (1, 24, 31)).astype(np.int64)
    for label in (blobs, noise):
        pred = np.roll(label, (1, 2), (-2, -1)).astype(np.int32)
        assert int(label.max()) < n_cls and int(pred.max()) < n_cls
        for radii in ((1,), (1, 2, 4, 8)):
            got, _, _ = co.contour_f(label, pred, radii, n_cls, fast=True)
            host = ev.contour_f_numpy(label, pred, radii, n_cls)
            for row, plane in ((0, label), (1, pred)):
                b = plane.astype(np.uint8)
                d1 = np.stack([bo.distance(p, 1) == 1 for p in b])
                assert np.array_equal(np.stack([co.marks(p) >= 0 for p in b]), d1)
                want = np.bincount(plane[d1].astype(np.int64), minlength=n_cls)
                assert np.array_equal(got[0, row].sum(0), want) and np.array_equal(host[row].sum(0), want) and int(want.sum()) > 0


def test_numpy_form_refuses_bad_arguments():
    from arseg_amd import evaluation as ev

    lab, prd = np.zeros((4, 4), np.int64), np.zeros((4, 4), np.int32)
    for bad in ((), (-1,), (33,), (2, 2), (4, 2), tuple(range(0, 9))):
        with pytest.raises(ValueError):
            ev.contour_f_numpy(lab, prd, bad, 3)
    with pytest.raises(ValueError):
        ev.contour_f_numpy(lab.astype(np.float32), prd, (1,), 3)
    with pytest.raises(ValueError):
        ev.contour_f_numpy(lab, prd[:3], (1,), 3)
    assert ev.contour_f_numpy(lab, prd, (0, 32), 3).shape == (2, 3, 3)


def test_contour_radius_at_the_dataset_sizes():
    from arseg_amd import ops

    assert ops.contour_radius(512, 1024) == 10 and ops.contour_radius(720, 960) == 10 and ops.contour_radius(1024, 2048) == 19
    assert ops.contour_radius(1, 1) == 1 and ops.contour_radius(720, 960, ratio=0.02) == 24
    assert ops.contour_radii([0, 3, 32]) == (0, 3, 32) and ops.contour_radii((32,)) == (32,) and ops.contour_radii((0,)) == (0,)
    for bad in ((), (-1,), (33,), (2, 2), (4, 2), tuple(range(0, 9))):
        with pytest.raises(ValueError):
            ops.contour_radii(bad)
    with pytest.raises(ValueError):
        ops.boundary_radii((0,))                                                    # Boundary IoU keeps its range
    assert ops.boundary_radii((64,)) == (64,)


def test_contour_table_arithmetic(tmp_path):
    from arseg_amd import evaluation as ev

    # hand numbers: one group, two radii, four classes.  (row, band, class); row 0 the ground truth's contour pixels, row 1 the prediction's
    c = np.zeros((1, 2, 3, 4), np.int64)
    c[0, 0, :, 0], c[0, 1, :, 0] = (2, 4, 2), (1, 2, 1)                            # class 0: R = 2/8, 6/8; P = 1/4, 3/4
    c[0, 0, :, 1], c[0, 1, :, 1] = (0, 0, 0), (0, 3, 1)                            # class 1: no true contour: R = NaN, so F = NaN
    c[0, 0, :, 2], c[0, 1, :, 2] = (0, 0, 5), (0, 0, 7)                            # class 2: nothing matched: P = R = 0, F = 0
    c[0, 0, :, 3], c[0, 1, :, 3] = (0, 0, 0), (0, 0, 0)                            # class 3: absent: all NaN
    table = ev.ContourTable(torch.from_numpy(c), (2, 5))
    assert table.radii == (2, 5)
    p0, r0, f0, f1 = table.precision(0), table.recall(0), table.f(0), table.f(1)
    assert p0.dtype == r0.dtype == f0.dtype == torch.float32 and tuple(f0.shape) == (1, 4)
    q, h = np.float32(0.25), np.float32(0.75)
    assert p0[0, 0].item() == q and r0[0, 0].item() == q and f0[0, 0].item() == np.float32(2) * q * q / (q + q)
    assert table.precision(1)[0, 0].item() == h and table.recall(1)[0, 0].item() == h and f1[0, 0].item() == np.float32(2) * h * h / (h + h)
    assert np.isnan(r0[0, 1].item()) and p0[0, 1].item() == 0.0 and np.isnan(f0[0, 1].item()) and table.precision(1)[0, 1].item() == h
    assert np.isnan(f1[0, 1].item())
    assert p0[0, 2].item() == 0.0 and r0[0, 2].item() == 0.0 and f0[0, 2].item() == 0.0 and f1[0, 2].item() == 0.0
    assert np.isnan(p0[0, 3].item()) and np.isnan(r0[0, 3].item()) and np.isnan(f0[0, 3].item())
    assert np.isnan(table.mean_f(0)[0]) and np.isnan(table.mean(1))
    two = ev.ContourTable(torch.from_numpy(c[..., [0, 2]]), (2, 5))                 # without the NaN classes
    assert two.mean_f(1) == [two.f(1)[0].mean().item()] == [(np.float32(0.75) + np.float32(0)) / np.float32(2)]
    assert two.mean(1) == np.array(two.mean_f(1)).mean()

    # shape and file round trip on counts from planes
    G, radii, n_cls = 3, (1, 2, 4, 8), 5
    label = rle_oracle.blob_planes(100, G, 30, 40, n_cls=n_cls, cell=6).astype(np.int64)        # every class has a contour in every frame
    label[:, :2, 5:9] = 255
    pred = np.where(label == 255, 1, np.roll(label, 2, axis=-1)).astype(np.int32)
    label[2], pred[2] = 255, 0                                                      # a distance without samples: NaN
    counts, _, _ = co.contour_f(label, pred, radii, n_cls, groups=range(G), n_groups=G, fast=True)
    table = ev.ContourTable(torch.from_numpy(counts), radii)
    assert table.counts.shape == (G, 2, 5, n_cls)
    arr = table.as_array()
    assert arr.shape == (len(radii), G + 1)
    for k in range(len(radii)):
        assert np.array_equal(arr[k, :G], np.array(table.mean_f(k)), equal_nan=True) and tuple(table.f(k).shape) == (G, n_cls)
        assert np.array_equal(arr[k, G], table.mean(k), equal_nan=True)
        both = torch.stack([table.recall(k)[:2], table.precision(k)[:2]])
        both = both[~both.isnan()]                                                  # (a class without a contour on a plane)
        assert both.numel() > 0 and bool((both >= 0).all()) and bool((both <= 1).all())
    wide, narrow = table.recall(3)[:2], table.recall(0)[:2]
    seen = ~narrow.isnan()
    assert bool((wide[seen] >= narrow[seen]).all()) and float(wide[seen].min()) > 0.5                                # a shift of 2 is within 8
    assert np.isnan(arr[:, 2]).all() and not np.isnan(arr[:, :2]).any()
    path = tmp_path / "contour.txt"
    table.save(path)
    assert open(path).readline().split() == ["#", "contour", "radii", "1", "2", "4", "8"]
    back = ev.ContourTable.load(path)
    assert back.radii == radii and back.counts is None
    assert np.array_equal(back.as_array(), arr, equal_nan=True)
    with pytest.raises(ValueError):
        back.f(0)
    with pytest.raises(ValueError):
        ev.ContourTable(torch.from_numpy(counts[:, :, :3]), radii)
    with pytest.raises(ValueError):
        ev.ContourTable(torch.from_numpy(counts[:, :1]), radii)
    with pytest.raises(IndexError):
        table.f(len(radii))
    other = tmp_path / "boundary.txt"
    ev.BoundaryTable(torch.zeros((2, 3, 5, 3), dtype=torch.int64), radii).save(other)
    with pytest.raises(ValueError):
        ev.ContourTable.load(other)                                                 # another table's file


def test_eval_by_contour_keeps_the_distance_evaluator():
    from arseg_amd import evaluation as ev

    e = ev.EvalByContour(scale=0.5, gop=12)
    assert isinstance(e, ev.EvalByDistance) and e.radii is None and e.gop == 12
    assert ev.EvalByContour(radii=[0, 3, 32]).radii == (0, 3, 32)
    with pytest.raises(ValueError):
        ev.EvalByContour(radii=(33,))


def _call(lib, label, pred, group, radii, lplane, lpitch, lns, pplane, ppitch, pns, counts, N, n_groups, n_cls, H, W, ws, ws_bytes):
    arr = None if radii is None else (ctypes.c_int * max(len(radii), 1))(*radii)
    return lib.arseg_contour_f_fwd(label, pred, group, arr, 0 if radii is None else len(radii), lplane, lpitch, lns, pplane, ppitch, pns, counts, N,
                                   n_groups, n_cls, H, W, 255, ws, ws_bytes, ctypes.c_void_p(0))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Never-dereferenced pointers: every refusal comes before a launch, so none of these touches a GPU."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    N, H, W = 2, 8, 10
    need = lib.arseg_contour_f_workspace_bytes(N, H, W)
    assert need == 2 * N * H * W
    good = dict(label=one, pred=one, group=one, radii=(0, 1, 10, 32), lplane=one, lpitch=W, lns=H * W, pplane=one, ppitch=W, pns=H * W, counts=one,
                N=N, n_groups=3, n_cls=19, H=H, W=W, ws=one, ws_bytes=need)
    bad = [dict(label=null), dict(pred=null), dict(ws=null), dict(radii=None), dict(radii=()), dict(radii=tuple(range(0, 9))), dict(radii=(-1, 1)),
           dict(radii=(1, 33)), dict(radii=(2, 2)), dict(radii=(4, 2)), dict(radii=(0, 0)), dict(n_cls=0), dict(n_cls=33), dict(n_cls=-1),
           dict(n_groups=0), dict(n_groups=-2), dict(group=null), dict(lpitch=W - 1), dict(lns=-1), dict(ppitch=W - 1), dict(pns=-1), dict(N=0),
           dict(H=0), dict(W=-1), dict(H=16385), dict(W=16385), dict(lplane=null, pplane=null, counts=null),
           dict(label=ctypes.c_void_p(68)), dict(counts=ctypes.c_void_p(68)), dict(pred=ctypes.c_void_p(66)), dict(group=ctypes.c_void_p(66)),
           dict(ws=ctypes.c_void_p(65))]
    for change in bad:
        assert _call(lib, **{**good, **change}) == _lib.ARSEG_EINVAL, change
    for short in (0, need - 1):
        assert _call(lib, **{**good, "ws_bytes": short}) == _lib.ARSEG_EWORKSPACE, short
    # the argument errors come first: a short workspace does not hide them
    assert _call(lib, **{**good, "ws_bytes": 0, "n_cls": 33}) == _lib.ARSEG_EINVAL
    assert _call(lib, **{**good, "ws_bytes": 0, "radii": (33,)}) == _lib.ARSEG_EINVAL
    # a null group is refused only with more than one group; a pitch is looked at only with its plane; any one output will do; radius 0 alone
    assert _call(lib, **{**good, "group": null, "n_groups": 1, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "lplane": null, "lpitch": 0, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "pplane": null, "ppitch": 0, "pns": -1, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    for keep in ("lplane", "pplane", "counts"):
        assert _call(lib, **{**good, **{k: null for k in ("lplane", "pplane", "counts") if k != keep}, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "radii": (0,), "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    # the siblings keep their radius ranges and workspaces
    arr = (ctypes.c_int * 2)(0, 1)
    assert lib.arseg_label_bands_fwd(one, one, one, arr, 2, one, W, H * W, one, N, 3, 19, H, W, 255, one, 1 << 20, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_boundary_iou_fwd(one, one, one, arr, 2, 1, one, W, H * W, one, W, H * W, one, N, 3, 19, H, W, 255, one, 1 << 20, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_label_bands_workspace_bytes(N, H, W) == 2 * N * H * W and lib.arseg_boundary_iou_workspace_bytes(N, H, W) == 4 * N * H * W


def test_workspace_size_saturates():
    from arseg_amd import _lib

    lib = _lib.load()
    size = lib.arseg_contour_f_workspace_bytes
    assert size(1, 1, 1) == 16 and size(1, 3, 3) == 32 and size(1, 3, 5) == 32 and size(1, 3, 6) == 48 and size(11, 1024, 2048) == 2 * 11 * 1024 * 2048
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, 16385, 4), (1, 4, 16385)):
        assert size(*bad) == 0
    # the largest arguments an int holds: 2^60 bytes, below SIZE_MAX on a 64-bit size_t -- exact, and more than any workspace has
    big = size(2 ** 31 - 1, 16384, 16384)
    limit = 2 ** (8 * ctypes.sizeof(ctypes.c_size_t)) - 1
    want = 2 * (2 ** 31 - 1) * 16384 * 16384
    assert big == (want if want + 15 <= limit else limit)
    one = ctypes.c_void_p(64)
    assert _call(lib, one, one, one, (1,), one, 16384, 0, one, 16384, 0, one, 2 ** 31 - 1, 1, 2, 16384, 16384, one, 1 << 40) == _lib.ARSEG_EWORKSPACE


def test_header_binding_and_exports_in_step():
    from arseg_amd import _lib, evaluation, ops

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("arseg_contour_f_workspace_bytes", 3), ("arseg_contour_f_fwd", 21)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in arseg_hip.h"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert sorted(n for n in _lib.PROTOTYPES if "contour_f" in n) == ["arseg_contour_f_fwd", "arseg_contour_f_workspace_bytes"]
    assert sorted(n for n in _lib.PROTOTYPES if "boundary_iou" in n) == ["arseg_boundary_iou_fwd", "arseg_boundary_iou_workspace_bytes"]
    assert sorted(n for n in _lib.PROTOTYPES if "label_bands" in n) == ["arseg_label_bands_fwd", "arseg_label_bands_workspace_bytes"]
    assert sorted(set(re.findall(r"\b(arseg_\w+)\s*\(", code))) == sorted(_lib.PROTOTYPES)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5 and "#define ARSEG_ABI_VERSION 5" in text
    assert "label_match_n_stride" in text and "pred_match_n_stride" in text and "m2(p) <= radii[k]^2" in text
    for mod, names in ((ops, ("contour_f", "contour_radii", "contour_radius", "boundary_iou", "label_bands")),
                       (evaluation, ("contour_f_numpy", "alter_res_batch_contour", "EvalByContour", "ContourTable"))):
        for n in names:
            assert callable(getattr(mod, n)), n


def test_the_kernels_sit_beside_their_siblings():
    """Both launches are in bands.hip and use its byte mapping and wave tally instead of restating them."""
    src = open(os.path.join(ROOT, "ar-seg_amd", "csrc", "bands.hip")).read()
    for name in ("bd_byte", "bd_tally"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ " + name + r"\(", src)) == 1, name
    marks = src[src.index("void contour_marks_kernel"):]
    assert marks[:marks.index("\n}\n")].count("bd_byte(") == 2
    match = src[src.index("void contour_match_kernel"):]
    assert "bd_tally(" in match[:match.index("\n}\n")] and "cf_search(" in match[:match.index("\n}\n")]
    assert src.count("hipLaunchKernelGGL(contour_") == 2


def test_documents_describe_the_contour_measure():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.18" in design and design.index("### 6.18") > design.index("### 6.17")
    section = design[design.index("### 6.18"):]
    for heading in ("Why", "Contract", "Passes", "Host layers", "Tests", "Measured", "Not covered"):
        assert f"**{heading}" in section, heading
    for word in ("seg2bmap", "bipartite", "per-frame F", "radii above 32", "Chebyshev"):
        assert word in section, word
    assert "6.18" in design[design.index("### 6.16"):design.index("### 6.17")]
    assert "6.18" in design[design.index("### 6.17"):design.index("### 6.18")]
    assert "EvalByContour" in open(os.path.join(ROOT, "README.md")).read()
    assert "EvalByContour" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_no_cpu_fallback():
    from arseg_amd import _lib, ops

    label = torch.zeros((1, 4, 4), dtype=torch.int64)
    pred = torch.zeros((1, 4, 4), dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):
        ops.contour_f(label, pred, (1, 2), n_cls=3)
    with pytest.raises(_lib.ArsegError):
        ops.contour_f(label, pred, (32,), n_cls=3, label_match_out=True)
    with pytest.raises(ValueError):
        ops.contour_f(label, pred, (2, 1), n_cls=3)
    with pytest.raises(ValueError):
        ops.contour_f(label, pred, (33,), n_cls=3)
    with pytest.raises(ValueError):
        ops.contour_f(label, pred, (1,), n_cls=3, n_groups=2)                       # no groups for two sets of counts
    with pytest.raises(ValueError):
        ops.contour_f(label, pred, (1,), n_cls=3, groups=[5], n_groups=2)           # a group id outside the range
