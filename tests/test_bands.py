"""CPU-side checks of the boundary bands (include/arseg_hip.h, arseg_label_bands_fwd): the hand cases' literal distances, the host form
evaluation.label_bands_numpy against the oracle's window definition, the sum over the bands against the plain confusion matrix, BandTable's
arithmetic, every argument the entry point refuses before a launch, the workspace size, and header, binding and exports in step.  All
equalities are exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bands_oracle as bo
import rle_oracle
from conftest import ROOT

RADII = [(1,), (1, 2, 4, 8), (3, 5, 32), (32,)]


@pytest.mark.parametrize("name,plane,ignore,want", bo.HAND, ids=bo.HAND_IDS)
def test_hand_cases_have_the_written_distances(name, plane, ignore, want):
    from arseg_amd import evaluation as ev

    b = bo.void_bytes(np.array(plane, dtype=np.int64), bo.HAND_N_CLS, ignore)
    d = bo.distance(b, bo.R_HAND)
    assert d.tolist() == want
    assert np.array_equal(bo.distance_fast(b, bo.R_HAND), d)
    for radii in ((1, 2, 3), (1, 3), (2,), (3,)):
        got = ev.label_bands_numpy(np.array(plane, dtype=np.int64), radii, bo.HAND_N_CLS, ignore)
        assert got.dtype == np.uint8 and np.array_equal(got, bo.bands(np.array(want), radii)), radii
    # a distance beyond the last radius is interior whatever the radius: the literals at R = 3 fix the bands of every smaller R
    for R in (1, 2):
        assert np.array_equal(bo.distance(b, R), np.minimum(np.array(want), R + 1))


def _planes():
    out = [("noise", bo.noise_plane(1, 23, 37, 5)[None], 5), ("noise-1-class", bo.noise_plane(2, 9, 70, 1, void=0.02)[None], 1),
           ("blocks", np.stack([bo.block_plane(3, 40, 70, 6), bo.block_plane(4, 40, 70, 6, cell=17)]), 6),
           ("blobs", rle_oracle.blob_planes(5, 2, 40, 56, n_cls=19, cell=8).astype(np.int64), 19),
           ("one-row", bo.block_plane(6, 1, 90, 4, cell=20), 4), ("one-column", bo.block_plane(7, 90, 1, 4, cell=20), 4)]
    return out


@pytest.mark.parametrize("radii", RADII, ids=str)
def test_numpy_form_equals_the_window_definition(radii):
    from arseg_amd import evaluation as ev

    for name, planes, n_cls in _planes():
        want = bo.label_bands(planes, radii, n_cls)
        got = ev.label_bands_numpy(planes, radii, n_cls)
        assert got.shape == planes.shape and np.array_equal(got, want), name
        assert np.array_equal(bo.label_bands(planes, radii, n_cls, fast=True), want), name
        assert int(want.max()) <= len(radii)
    for name, plane, ignore, _ in bo.HAND:
        lab = np.array(plane, dtype=np.int64)
        assert np.array_equal(ev.label_bands_numpy(lab, radii, bo.HAND_N_CLS, ignore), bo.label_bands(lab, radii, bo.HAND_N_CLS, ignore)), name


def test_numpy_form_refuses_bad_radii():
    from arseg_amd import evaluation as ev

    lab = np.zeros((4, 4), np.int64)
    for bad in ((), (0,), (33,), (2, 2), (4, 2), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            ev.label_bands_numpy(lab, bad, 3)
    with pytest.raises(ValueError):
        ev.label_bands_numpy(np.zeros((4, 4), np.float32), (1,), 3)


@pytest.mark.parametrize("radii", RADII, ids=str)
def test_bands_sum_to_the_plain_confusion_matrix(radii):
    n_cls, N = 6, 3
    label = np.stack([bo.block_plane(10 + n, 40, 70, n_cls) for n in range(N)])
    g = np.random.Generator(np.random.PCG64(11))
    pred = np.where(g.random(label.shape) < 0.2, g.integers(-1, n_cls + 1, label.shape), np.where(label == 255, 0, label)).astype(np.int32)
    band = bo.label_bands(label, radii, n_cls, fast=True)
    groups = [2, 0, 2]
    hist = bo.banded_hist(label, pred, band, groups, 3, len(radii), n_cls)
    assert hist.shape == (3, len(radii) + 1, n_cls, n_cls)
    for grp in range(3):
        sel = [n for n in range(N) if groups[n] == grp]
        assert np.array_equal(hist[grp].sum(0), bo.confusion(label[sel], pred[sel], n_cls))
    assert int(hist[1].sum()) == 0 and int(hist.sum()) == int(bo.confusion(label, pred, n_cls).sum())
    assert int(hist[:, 0].sum()) > 0
    out = bo.banded_hist(label, pred, band, [3, -1, 7], 3, len(radii), n_cls)
    assert int(out.sum()) == 0


def test_band_table_arithmetic(tmp_path):
    from arseg_amd import evaluation as ev

    g = np.random.Generator(np.random.PCG64(12))
    G, radii, n_cls = 4, (1, 2, 4, 8), 5
    hist = torch.from_numpy(g.integers(0, 1000, (G, len(radii) + 1, n_cls, n_cls)).astype(np.int64))
    hist[2] = 0                                                                   # a distance without samples: NaN, as EvalTable gives
    table = ev.BandTable(hist, radii)
    assert table.radii == radii and table.hist is hist
    total = table.total()
    assert isinstance(total, ev.EvalTable) and torch.equal(total.hist, hist.sum(1))
    assert torch.equal(table.trimap(len(radii) - 1).hist + table.interior().hist, total.hist)
    assert torch.equal(table.trimap(0).hist, table.band(0).hist) and torch.equal(table.interior().hist, hist[:, -1])
    for k in range(len(radii)):
        assert torch.equal(table.band(k).hist, hist[:, k])
        assert torch.equal(table.trimap(k).hist, sum(table.band(j).hist for j in range(k + 1)))
    arr = table.as_array()
    assert arr.shape == (len(radii) + 2, G + 1)
    assert np.array_equal(arr[-1], total.as_array(), equal_nan=True) and np.array_equal(arr[-2], table.interior().as_array(), equal_nan=True)
    assert np.array_equal(arr[1], table.trimap(1).as_array(), equal_nan=True)
    assert np.isnan(arr[:, 2]).all() and not np.isnan(arr[:, [0, 1, 3]]).any()
    path = tmp_path / "bands.txt"
    table.save(path)
    back = ev.BandTable.load(path)
    assert back.radii == radii and back.hist is None
    assert np.array_equal(back.as_array(), arr, equal_nan=True)
    with pytest.raises(ValueError):
        back.total()
    with pytest.raises(ValueError):
        ev.BandTable(hist[:, :3], radii)
    with pytest.raises(IndexError):
        table.trimap(len(radii))
    other = tmp_path / "plain.txt"
    total.save(other)
    with pytest.raises(ValueError):
        ev.BandTable.load(other)                                                  # an EvalTable file has no radii line


def test_eval_by_band_keeps_the_distance_evaluator():
    from arseg_amd import evaluation as ev

    e = ev.EvalByBand(scale=0.5, gop=12)
    assert isinstance(e, ev.EvalByDistance) and e.radii == (1, 2, 4, 8) and e.gop == 12
    assert ev.EvalByBand(radii=[3, 5, 32]).radii == (3, 5, 32)
    with pytest.raises(ValueError):
        ev.EvalByBand(radii=(2, 1))


def _call(lib, label, pred, group, radii, band_out, pitch, ns, hist, N, n_groups, n_cls, H, W, ws, ws_bytes):
    arr = None if radii is None else (ctypes.c_int * max(len(radii), 1))(*radii)
    return lib.arseg_label_bands_fwd(label, pred, group, arr, 0 if radii is None else len(radii), band_out, pitch, ns, hist, N, n_groups, n_cls,
                                     H, W, 255, ws, ws_bytes, ctypes.c_void_p(0))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Never-dereferenced pointers: every refusal comes before a launch, so none of these touches a GPU."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    N, H, W = 2, 8, 10
    need = lib.arseg_label_bands_workspace_bytes(N, H, W)
    assert need == 2 * N * H * W
    good = dict(label=one, pred=one, group=one, radii=(1, 2, 4, 8), band_out=one, pitch=W, ns=H * W, hist=one, N=N, n_groups=3, n_cls=19, H=H,
                W=W, ws=one, ws_bytes=need)
    bad = [dict(label=null), dict(ws=null), dict(radii=None), dict(radii=()), dict(radii=tuple(range(1, 10))), dict(radii=(0, 1)), dict(radii=(1, 33)),
           dict(radii=(2, 2)), dict(radii=(4, 2)), dict(radii=(-1,)), dict(n_cls=0), dict(n_cls=33), dict(n_cls=-1), dict(n_groups=0),
           dict(n_groups=-2), dict(group=null), dict(pred=null), dict(pitch=W - 1), dict(ns=-1), dict(N=0), dict(H=0), dict(W=-1),
           dict(H=16385), dict(W=16385), dict(label=ctypes.c_void_p(68)), dict(hist=ctypes.c_void_p(68)), dict(pred=ctypes.c_void_p(66)),
           dict(group=ctypes.c_void_p(66)), dict(ws=ctypes.c_void_p(65))]
    for change in bad:
        assert _call(lib, **{**good, **change}) == _lib.ARSEG_EINVAL, change
    for short in (0, need - 1):
        assert _call(lib, **{**good, "ws_bytes": short}) == _lib.ARSEG_EWORKSPACE, short
    # the argument errors come first: a short workspace does not hide them
    assert _call(lib, **{**good, "ws_bytes": 0, "n_cls": 33}) == _lib.ARSEG_EINVAL
    # a null group is refused only with more than one group; a pitch is looked at only with a plane
    assert _call(lib, **{**good, "group": null, "n_groups": 1, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "band_out": null, "pitch": 0, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE
    assert _call(lib, **{**good, "pred": null, "hist": null, "ws_bytes": 0}) == _lib.ARSEG_EWORKSPACE


def test_workspace_size_saturates():
    from arseg_amd import _lib

    lib = _lib.load()
    size = lib.arseg_label_bands_workspace_bytes
    assert size(1, 1, 1) == 16 and size(1, 3, 3) == 32 and size(11, 1024, 2048) == 2 * 11 * 1024 * 2048           # rounded up to 16 bytes
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, 16385, 4), (1, 4, 16385)):
        assert size(*bad) == 0
    # the largest arguments an int holds: 2^60 bytes, below SIZE_MAX on a 64-bit size_t -- exact, and more than any workspace has
    big = size(2 ** 31 - 1, 16384, 16384)
    limit = 2 ** (8 * ctypes.sizeof(ctypes.c_size_t)) - 1
    want = 2 * (2 ** 31 - 1) * 16384 * 16384
    assert big == (want if want + 15 <= limit else limit)
    one = ctypes.c_void_p(64)
    assert _call(lib, one, one, one, (1,), one, 16384, 0, one, 2 ** 31 - 1, 1, 2, 16384, 16384, one, 1 << 40) == _lib.ARSEG_EWORKSPACE


def _header():
    text = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_binding_and_exports_in_step():
    from arseg_amd import _lib, evaluation, ops

    lib = _lib.load()
    text, code = _header()
    for name in ("arseg_label_bands_workspace_bytes", "arseg_label_bands_fwd"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in arseg_hip.h"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert sorted(n for n in _lib.PROTOTYPES if "label_bands" in n) == ["arseg_label_bands_fwd", "arseg_label_bands_workspace_bytes"]
    assert sorted(set(re.findall(r"\b(arseg_\w+)\s*\(", code))) == sorted(_lib.PROTOTYPES)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5 and "#define ARSEG_ABI_VERSION 5" in text
    assert "Chebyshev" in text and "band_n_stride" in text
    for mod, names in ((ops, ("label_bands", "band_radii")), (evaluation, ("label_bands_numpy", "alter_res_batch_bands", "EvalByBand", "BandTable"))):
        for n in names:
            assert callable(getattr(mod, n)), n
    assert "bands.hip" in open(os.path.join(ROOT, "ar-seg_amd", "csrc", "Makefile")).read()


def test_documents_describe_the_bands():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.16" in design
    section = design[design.index("### 6.16"):]
    for heading in ("Why", "Contract", "Passes", "Host layers", "Tests", "Measured", "Not covered"):
        assert f"**{heading}" in section, heading
    assert "EvalByBand" in open(os.path.join(ROOT, "README.md")).read()


def test_no_cpu_fallback():
    from arseg_amd import _lib, ops

    label = torch.zeros((1, 4, 4), dtype=torch.int64)
    pred = torch.zeros((1, 4, 4), dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):
        ops.label_bands(label, (1, 2), pred=pred, n_cls=3)
    with pytest.raises(_lib.ArsegError):
        ops.label_bands(label, (1, 2), n_cls=3)
    with pytest.raises(ValueError):
        ops.label_bands(label, (2, 1), pred=pred, n_cls=3)
    with pytest.raises(ValueError):
        ops.label_bands(label, (1,), pred=pred, n_cls=3, n_groups=2)                   # no groups for two histograms
    with pytest.raises(ValueError):
        ops.label_bands(label, (1,), hist=torch.zeros((1, 2, 3, 3), dtype=torch.int64))   # hist without pred
