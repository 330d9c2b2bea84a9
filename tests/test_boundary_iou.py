"""CPU-side checks of the Boundary IoU counts (include/arseg_hip.h, arseg_boundary_iou_fwd): the hand cases' literal distances and counts,
the host form evaluation.boundary_iou_numpy (per-class erosion) against the oracle's window definition, the sum over the bands against the
plain confusion matrix, row 0 against the trimap bands, BoundaryTable's arithmetic, every argument the entry point refuses before a launch,
the workspace size, and header, binding and exports in step.  All equalities are exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bands_oracle as bo
import boundary_iou_oracle as bio
import rle_oracle
from conftest import ROOT

RADII = [(1,), (1, 2, 4, 8), (3, 33, 64), (64,)]


@pytest.mark.parametrize("name,label,pred,border,want_dl,want_dp,want_counts", bio.HAND, ids=bio.HAND_IDS)
def test_hand_cases_have_the_written_distances_and_counts(name, label, pred, border, want_dl, want_dp, want_counts):
    from arseg_amd import evaluation as ev

    lab, prd = np.array(label, dtype=np.int64), np.array(pred, dtype=np.int32)
    lb, pb = bo.void_bytes(lab, bio.HAND_N_CLS), bio.pred_bytes(prd, bio.HAND_N_CLS)
    assert bio.distance(lb, bio.R_HAND, border).tolist() == want_dl
    assert bio.distance(pb, bio.R_HAND, border).tolist() == want_dp
    assert np.array_equal(bio.distance(lb, bio.R_HAND, border, fast=True), np.array(want_dl))
    assert np.array_equal(bio.distance(pb, bio.R_HAND, border, fast=True), np.array(want_dp))
    want = bio.sparse(want_counts)
    got, bg, bp = bio.boundary_iou(lab[None], prd[None], bio.RADII_HAND, bio.HAND_N_CLS, border=border)
    assert np.array_equal(got[0], want)
    assert np.array_equal(bg[0], bo.bands(np.array(want_dl), bio.RADII_HAND)) and np.array_equal(bp[0], bo.bands(np.array(want_dp), bio.RADII_HAND))
    host = ev.boundary_iou_numpy(lab, prd, bio.RADII_HAND, bio.HAND_N_CLS, border=bool(border))
    assert host.dtype == np.int64 and np.array_equal(host, want)


def _planes():
    """(name, labels [N,H,W] int64, predictions [N,H,W] int32, n_cls): void pixels and predictions outside the classes in each."""
    g = np.random.Generator(np.random.PCG64(70))

    def preds(label, n_cls, wrong=0.2):
        return np.where(g.random(label.shape) < wrong, g.integers(-2, n_cls + 2, label.shape), np.where(label == 255, 0, label)).astype(np.int32)

    def shifted(label):
        return np.where(label == 255, 1, np.roll(label, 1, axis=-1)).astype(np.int32)

    noise = bo.noise_plane(71, 23, 37, 5)[None]
    blocks = np.stack([bo.block_plane(72, 40, 70, 6), bo.block_plane(73, 40, 70, 6, cell=17)])
    blobs = rle_oracle.blob_planes(74, 2, 40, 56, n_cls=19, cell=8).astype(np.int64)
    blobs[:, :3, 10:30] = 255
    wide = bo.block_plane(75, 70, 150, 3, cell=70)[None]                                  # regions wider than 64: the interior is populated at R = 64
    row, col = bo.block_plane(76, 1, 90, 4, cell=20), bo.block_plane(77, 90, 1, 4, cell=20)
    return [("noise", noise, preds(noise, 5), 5), ("blocks", blocks, preds(blocks, 6), 6), ("blocks-shifted", blocks, shifted(blocks), 6),
            ("blobs", blobs, shifted(blobs), 19), ("wide", wide, shifted(wide), 3), ("one-row", row[None], preds(row, 4)[None], 4),
            ("one-column", col[None], preds(col, 4)[None], 4)]


_PLANES = _planes()


@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("radii", RADII, ids=str)
def test_numpy_form_equals_the_window_definition(radii, border):
    from arseg_amd import evaluation as ev

    for name, label, pred, n_cls in _PLANES:
        want, bg, bp = bio.boundary_iou(label, pred, radii, n_cls, border=border, fast=True)
        got = ev.boundary_iou_numpy(label, pred, radii, n_cls, border=bool(border))
        assert got.shape == (3, len(radii) + 1, n_cls) and np.array_equal(got, want[0]), name
        assert int(bg.max()) <= len(radii) and int(bp.max()) <= len(radii)
    for name, label, pred, _, _, _, _ in bio.HAND:
        lab, prd = np.array(label, dtype=np.int64), np.array(pred, dtype=np.int32)
        want, _, _ = bio.boundary_iou(lab[None], prd[None], radii, bio.HAND_N_CLS, border=border)
        assert np.array_equal(ev.boundary_iou_numpy(lab, prd, radii, bio.HAND_N_CLS, border=bool(border)), want[0]), name


def test_fast_distance_equals_the_window_at_large_radii():
    """The vectorised distances the larger planes use, held to the pixel-by-pixel window where the radius passes 32, and to each other."""
    from arseg_amd import ops

    radii = ops.boundary_radii((1, 8, 33, 64))                                    # the largest is the entry point's limit
    for name, label, pred, n_cls in (_PLANES[3], (_PLANES[4][0], _PLANES[4][1][:, :12], _PLANES[4][2][:, :12], 3), _PLANES[5], _PLANES[6]):
        for b in (bo.void_bytes(label[0], n_cls), bio.pred_bytes(pred[0], n_cls)):
            for border in (0, 1):
                assert np.array_equal(bio.distance(b, radii[-1], border, fast=True), bio.distance(b, radii[-1], border)), name
                assert np.array_equal(bio.distance(b, radii[-1], border, fast="minmax"), bio.distance(b, radii[-1], border)), name
    for name, label, pred, n_cls in _PLANES:
        for b in (bo.void_bytes(label[0], n_cls), bio.pred_bytes(pred[0], n_cls)):
            for R in radii:
                assert np.array_equal(bio.distance(b, R, 0, fast="minmax"), bio.distance(b, R, 0, fast=True)), (name, R)


def test_numpy_form_refuses_bad_arguments():
    from arseg_amd import evaluation as ev

    lab, prd = np.zeros((4, 4), np.int64), np.zeros((4, 4), np.int32)
    for bad in ((), (0,), (65,), (2, 2), (4, 2), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            ev.boundary_iou_numpy(lab, prd, bad, 3)
    with pytest.raises(ValueError):
        ev.boundary_iou_numpy(lab.astype(np.float32), prd, (1,), 3)
    with pytest.raises(ValueError):
        ev.boundary_iou_numpy(lab, prd[:3], (1,), 3)
    assert ev.boundary_iou_numpy(lab, prd, (33, 64), 3).shape == (3, 3, 3)


@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("radii", RADII, ids=str)
def test_bands_sum_to_the_plain_confusion_matrix(radii, border):
    n_cls, N = 6, 3
    label = np.stack([bo.block_plane(80 + n, 40, 70, n_cls) for n in range(N)])
    g = np.random.Generator(np.random.PCG64(81))
    pred = np.where(g.random(label.shape) < 0.2, g.integers(-1, n_cls + 1, label.shape), np.where(label == 255, 0, label)).astype(np.int32)
    groups = [2, 0, 2]
    counts, _, _ = bio.boundary_iou(label, pred, radii, n_cls, border=border, groups=groups, n_groups=3, fast=True)
    assert counts.shape == (3, 3, len(radii) + 1, n_cls)
    for grp in range(3):
        sel = [n for n in range(N) if groups[n] == grp]
        conf = bo.confusion(label[sel], pred[sel], n_cls)
        total = counts[grp].sum(1)
        assert np.array_equal(total[0], conf.sum(1)) and np.array_equal(total[1], conf.sum(0)) and np.array_equal(total[2], conf.diagonal())
    assert int(counts[1].sum()) == 0 and int(counts[:, 2, 0].sum()) > 0
    from arseg_amd import evaluation as ev

    host = ev.boundary_iou_numpy(label[[0, 2]], pred[[0, 2]], radii, n_cls, border=bool(border))
    assert np.array_equal(host, counts[2]) and np.array_equal(host.sum(1)[2], bo.confusion(label[[0, 2]], pred[[0, 2]], n_cls).diagonal())
    out, _, _ = bio.boundary_iou(label, pred, radii, n_cls, border=border, groups=[3, -1, 7], n_groups=3, fast=True)
    assert int(out.sum()) == 0


@pytest.mark.parametrize("radii", [(1,), (1, 2, 4, 8), (3, 5, 32)], ids=str)
def test_row_0_without_border_is_the_trimap_histogram_summed_over_predictions(radii):
    from arseg_amd import evaluation as ev

    for name, label, pred, n_cls in _PLANES:
        N = label.shape[0]
        band = bo.label_bands(label, radii, n_cls, fast=True)
        hist = bo.banded_hist(label, pred, band, [0] * N, 1, len(radii), n_cls)
        counts, bg, _ = bio.boundary_iou(label, pred, radii, n_cls, border=0, fast=True)
        assert np.array_equal(bg, band) and np.array_equal(counts[0, 0], hist[0].sum(-1)), name
        assert np.array_equal(ev.boundary_iou_numpy(label, pred, radii, n_cls, border=False)[0], hist[0].sum(-1)), name


def test_boundary_radius_at_the_dataset_sizes():
    from arseg_amd import ops

    assert ops.boundary_radius(720, 960) == 24 and ops.boundary_radius(512, 1024) == 23 and ops.boundary_radius(1024, 2048) == 46
    assert ops.boundary_radius(1, 1) == 1 and ops.boundary_radius(720, 960, ratio=0.01) == 12
    assert ops.boundary_radii([3, 33, 64]) == (3, 33, 64) and ops.boundary_radii((64,)) == (64,)
    for bad in ((), (0,), (65,), (2, 2), (4, 2), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            ops.boundary_radii(bad)
    with pytest.raises(ValueError):
        ops.band_radii((33,))                                                      # the trimap bands keep their limit


def test_boundary_table_arithmetic(tmp_path):
    from arseg_amd import evaluation as ev

    # hand numbers: one group, two radii, two classes.  (row, band, class)
    c = np.zeros((1, 3, 3, 2), np.int64)
    c[0, 0, :, 0], c[0, 1, :, 0], c[0, 2, :, 0] = (4, 2, 10), (3, 3, 12), (1, 2, 9)      # G, P, I of class 0 per band
    c[0, 0, :, 1], c[0, 1, :, 1], c[0, 2, :, 1] = (0, 5, 5), (0, 1, 7), (0, 1, 4)
    table = ev.BoundaryTable(torch.from_numpy(c), (2, 5), border=False)
    assert table.radii == (2, 5) and table.border is False
    b0, b1, full = table.boundary_iou(0), table.boundary_iou(1), table.iou()
    assert b0.dtype == torch.float32 and tuple(b0.shape) == (1, 2)
    assert b0[0, 0].item() == np.float32(1) / np.float32(6) and np.isnan(b0[0, 1].item())           # 1 / (4 + 3 - 1); 0 / 0
    assert b1[0, 0].item() == np.float32(3) / np.float32(9) and b1[0, 1].item() == np.float32(1) / np.float32(5)
    assert full[0, 0].item() == np.float32(12) / np.float32(22) and full[0, 1].item() == np.float32(5) / np.float32(13)
    assert np.isnan(table.miou(0)[0]) and table.miou(1) == [b1[0].mean().item()] and table.miou() == [full[0].mean().item()]
    assert table.mean(1) == np.array(table.miou(1)).mean()

    # against EvalTable on the matching confusion matrices
    g = np.random.Generator(np.random.PCG64(82))
    G, radii, n_cls = 4, (1, 2, 4, 8), 5
    label = g.integers(0, n_cls, (G, 30, 40)).astype(np.int64)
    pred = np.where(g.random(label.shape) < 0.3, g.integers(0, n_cls, label.shape), label).astype(np.int32)
    label[3], pred[3] = 255, 0                                                    # a distance without samples: NaN, as EvalTable gives
    counts, _, _ = bio.boundary_iou(label, pred, radii, n_cls, groups=range(G), n_groups=G, fast=True)
    conf = torch.from_numpy(np.stack([bo.confusion(label[n], pred[n], n_cls) for n in range(G)]))
    table, plain = ev.BoundaryTable(torch.from_numpy(counts), radii), ev.EvalTable(conf)
    assert table.counts.shape == (G, 3, 5, n_cls) and table.border is True
    assert torch.equal(table.iou()[:3], plain.iou[:3]) and bool(torch.isnan(table.iou()[3]).all()) and bool(torch.isnan(plain.iou[3]).all())
    assert np.array_equal(np.array(table.miou()), np.array(plain.miou), equal_nan=True)
    arr = table.as_array()
    assert arr.shape == (len(radii) + 1, G + 1)
    assert np.array_equal(arr[-1], plain.as_array(), equal_nan=True)
    for k in range(len(radii)):
        assert np.array_equal(arr[k, :G], np.array(table.miou(k)), equal_nan=True)
        assert tuple(table.boundary_iou(k).shape) == (G, n_cls)
    assert np.isnan(arr[:, 3]).all() and not np.isnan(arr[:, :3]).any()
    path = tmp_path / "boundary.txt"
    table.save(path)
    assert open(path).readline().split() == ["#", "radii", "1", "2", "4", "8", "border", "1"]
    back = ev.BoundaryTable.load(path)
    assert back.radii == radii and back.border is True and back.counts is None
    assert np.array_equal(back.as_array(), arr, equal_nan=True)
    with pytest.raises(ValueError):
        back.iou()
    with pytest.raises(ValueError):
        ev.BoundaryTable(torch.from_numpy(counts[:, :, :3]), radii)
    with pytest.raises(ValueError):
        ev.BoundaryTable(torch.from_numpy(counts[:, :2]), radii)
    with pytest.raises(IndexError):
        table.boundary_iou(len(radii))
    other = tmp_path / "bands.txt"
    ev.BandTable(torch.zeros((2, 5, 3, 3), dtype=torch.int64), radii).save(other)
    with pytest.raises(ValueError):
        ev.BoundaryTable.load(other)                                              # a BandTable file has no border flag


def test_eval_by_boundary_keeps_the_distance_evaluator():
    from arseg_amd import evaluation as ev

    e = ev.EvalByBoundary(scale=0.5, gop=12)
    assert isinstance(e, ev.EvalByDistance) and e.radii is None and e.border is True and e.gop == 12
    assert ev.EvalByBoundary(radii=[3, 33, 64], border=False).radii == (3, 33, 64)
    with pytest.raises(ValueError):
        ev.EvalByBoundary(radii=(65,))


def _call(lib, label, pred, group, radii, border, lband, lpitch, lns, pband, ppitch, pns, counts, N, n_groups, n_cls, H, W, ws, ws_bytes):
    arr = None if radii is None else (ctypes.c_int * max(len(radii), 1))(*radii)
    return lib.arseg_boundary_iou_fwd(label, pred, group, arr, 0 if radii is None else len(radii), border, lband, lpitch, lns, pband, ppitch, pns,
                                      counts, N, n_groups, n_cls, H, W, 255, ws, ws_bytes, ctypes.c_void_p(0))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Never-dereferenced pointers: every refusal comes before a launch, so none of these touches a GPU."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    N, H, W = 2, 8, 10
    need = lib.arseg_boundary_iou_workspace_bytes(N, H, W)
    assert need == 4 * N * H * W
    good = dict(label=one, pred=one, group=one, radii=(1, 2, 33, 64), border=1, lband=one, lpitch=W, lns=H * W, pband=one, ppitch=W, pns=H * W,
                counts=one, N=N, n_groups=3, n_cls=19, H=H, W=W, ws=one, ws_bytes=need)
    bad = [dict(label=null), dict(pred=null), dict(ws=null), dict(radii=None), dict(radii=()), dict(radii=tuple(range(1, 10))), dict(radii=(0, 1)),
           dict(radii=(1, 65)), dict(radii=(2, 2)), dict(radii=(4, 2)), dict(radii=(-1,)), dict(n_cls=0), dict(n_cls=33), dict(n_cls=-1),
           dict(n_groups=0), dict(n_groups=-2), dict(group=null), dict(lpitch=W - 1), dict(lns=-1), dict(ppitch=W - 1), dict(pns=-1), dict(N=0),
           dict(H=0), dict(W=-1), dict(H=16385), dict(W=16385), dict(border=2), dict(border=-1), dict(lband=null, pband=null, counts=null),
           dict(label=ctypes.c_void_p(68)), dict(counts=ctypes.c_void_p(68)), dict(pred=ctypes.c_void_p(66)), dict(group=ctypes.c_void_p(66)),
           dict(ws=ctypes.c_void_p(65))]
    for change in bad:
        assert _call(lib, **{**good, **change}) == _lib.ARSEG_EINVAL, change
    for short in (0, need - 1):
        assert _call(lib, **{**good, "ws_bytes": short}) == _lib.ARSEG_EWORKSPACE, short
    # the argument errors come first: a short workspace does not hide them
    assert _call(lib, **{**good, "ws_bytes": 0, "n_cls": 33}) == _lib.ARSEG_EINVAL
    assert _call(lib, **{**good, "ws_bytes": 0, "border": 2}) == _lib.ARSEG_EINVAL
    # a null group is refused only with more than one group; a pitch is looked at only with its plane; any one output will do
    assert _call(lib, **{**good, "group": null, "n_groups": 1, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "lband": null, "lpitch": 0, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "pband": null, "ppitch": 0, "pns": -1, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    for keep in ("lband", "pband", "counts"):
        assert _call(lib, **{**good, **{k: null for k in ("lband", "pband", "counts") if k != keep}, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "border": 0, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    # the trimap bands keep their limit of 32 and their workspace
    arr = (ctypes.c_int * 2)(1, 33)
    assert lib.arseg_label_bands_fwd(one, one, one, arr, 2, one, W, H * W, one, N, 3, 19, H, W, 255, one, need, null) == _lib.ARSEG_EINVAL
    assert lib.arseg_label_bands_workspace_bytes(N, H, W) == 2 * N * H * W


def test_workspace_size_saturates():
    from arseg_amd import _lib

    lib = _lib.load()
    size = lib.arseg_boundary_iou_workspace_bytes
    assert size(1, 1, 1) == 16 and size(1, 3, 3) == 48 and size(1, 3, 5) == 64 and size(11, 1024, 2048) == 4 * 11 * 1024 * 2048
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, 16385, 4), (1, 4, 16385)):
        assert size(*bad) == 0
    # the largest arguments an int holds: 2^61 bytes, below SIZE_MAX on a 64-bit size_t -- exact, and more than any workspace has
    big = size(2 ** 31 - 1, 16384, 16384)
    limit = 2 ** (8 * ctypes.sizeof(ctypes.c_size_t)) - 1
    want = 4 * (2 ** 31 - 1) * 16384 * 16384
    assert big == (want if want + 15 <= limit else limit)
    one = ctypes.c_void_p(64)
    assert _call(lib, one, one, one, (1,), 1, one, 16384, 0, one, 16384, 0, one, 2 ** 31 - 1, 1, 2, 16384, 16384, one, 1 << 40) == _lib.ARSEG_EWORKSPACE


def test_header_binding_and_exports_in_step():
    from arseg_amd import _lib, evaluation, ops

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("arseg_boundary_iou_workspace_bytes", 3), ("arseg_boundary_iou_fwd", 22)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in arseg_hip.h"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert sorted(n for n in _lib.PROTOTYPES if "boundary_iou" in n) == ["arseg_boundary_iou_fwd", "arseg_boundary_iou_workspace_bytes"]
    assert sorted(n for n in _lib.PROTOTYPES if "label_bands" in n) == ["arseg_label_bands_fwd", "arseg_label_bands_workspace_bytes"]
    assert sorted(set(re.findall(r"\b(arseg_\w+)\s*\(", code))) == sorted(_lib.PROTOTYPES)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5 and "#define ARSEG_ABI_VERSION 5" in text
    assert "label_band_n_stride" in text and "pred_band_n_stride" in text and "max(bg, bp)" in text
    for mod, names in ((ops, ("boundary_iou", "boundary_radii", "boundary_radius", "label_bands", "band_radii")),
                       (evaluation, ("boundary_iou_numpy", "alter_res_batch_boundary", "EvalByBoundary", "BoundaryTable"))):
        for n in names:
            assert callable(getattr(mod, n)), n
    assert "bands.hip" in open(os.path.join(ROOT, "ar-seg_amd", "csrc", "Makefile")).read()


def test_one_definition_of_the_shared_passes():
    """The byte mapping, the row pass and the wave tally are defined once in bands.hip and used by both entry points' kernels; the dy walk
    stays label_bands', the ballots over a column's rows are boundary_iou's."""
    src = open(os.path.join(ROOT, "ar-seg_amd", "csrc", "bands.hip")).read()
    for name, uses in (("bd_byte", 1), ("bd_rows", 2), ("bd_tally", 2), ("bd_walk", 1), ("bd_band", 1), ("bi_column", 2)):
        assert len(re.findall(r"__device__ __forceinline__ \w+ " + name + r"\(", src)) == 1, name
        assert len(re.findall(r"\b" + name + r"\(", src)) >= 1 + uses, name
    for kernel in ("bands_rows_kernel", "boundary_rows_kernel"):
        body = src[src.index("void " + kernel):]
        assert "bd_rows(" in body[:body.index("\n}\n")], kernel
    for kernel in ("bands_cols_kernel", "boundary_cols_kernel"):
        body = src[src.index("void " + kernel):]
        assert "bd_tally(" in body[:body.index("\n}\n")], kernel
    code = re.sub(r"//.*", "", src)
    assert "float" not in code and "double" not in code


def test_documents_describe_boundary_iou():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.17" in design and design.index("### 6.17") > design.index("### 6.16")
    section = design[design.index("### 6.17"):]
    for heading in ("Why", "Contract", "Passes", "Host layers", "Tests", "Measured", "Not covered"):
        assert f"**{heading}" in section, heading
    for word in ("Euclidean", "radii above 64", "Boundary AP", "min(IoU", "argmax launch"):
        assert word in section, word
    between = design[design.index("### 6.16"):design.index("### 6.17")]
    assert "6.17" in between
    assert "EvalByBoundary" in open(os.path.join(ROOT, "README.md")).read()
    assert "EvalByBoundary" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_no_cpu_fallback():
    from arseg_amd import _lib, ops

    label = torch.zeros((1, 4, 4), dtype=torch.int64)
    pred = torch.zeros((1, 4, 4), dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):
        ops.boundary_iou(label, pred, (1, 2), n_cls=3)
    with pytest.raises(_lib.ArsegError):
        ops.boundary_iou(label, pred, (64,), n_cls=3, border=False, label_band_out=True)
    with pytest.raises(ValueError):
        ops.boundary_iou(label, pred, (2, 1), n_cls=3)
    with pytest.raises(ValueError):
        ops.boundary_iou(label, pred, (65,), n_cls=3)
    with pytest.raises(ValueError):
        ops.boundary_iou(label, pred, (1,), n_cls=3, n_groups=2)                      # no groups for two sets of counts
    with pytest.raises(ValueError):
        ops.boundary_iou(label, pred, (1,), n_cls=3, groups=[5], n_groups=2)          # a group id outside the range
