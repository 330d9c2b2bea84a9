"""CPU checks of the polygon fill (include/arseg_hip.h, arseg_contours_fill_fwd; arseg_amd.egress.fill / fill_numpy): the oracle written
on the pixel centres (tests/fill_oracle.py) against planes written out by hand; the pure-numpy host form against the oracle on every
plane of the contour and shared-border checks and a blob plane, for the exact outlines, simplify_numpy's and simplify_shared_numpy's at
five tolerances and both connectivities; the round trip (exact outlines and tolerance 0 give the source plane back); the partition
property of the shared borders (no gap, no overlap) and that plain simplification does not have it; E <= 2 runs; the wrappers'
refusals and every ARSEG_EINVAL / ARSEG_EWORKSPACE case through ctypes (the library loads without a GPU).  Everything is an integer:
every comparison is exact."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import contours_oracle
import fill_oracle as oracle
import rle_oracle
import simplify_shared_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCES = (0, 0.5, 1, 2, 4)
BLOB = ("blob-64x96", rle_oracle.blob_planes(3, 1, 64, 96, cell=8)[0])
BIG_BLOB = ("blob-128x256", rle_oracle.blob_planes(5, 1, 128, 256, cell=16)[0])
SHARED_PLANES = simplify_shared_oracle.cpu_planes()


def _planes():
    seen, out = set(), []
    for name, plane in SHARED_PLANES + contours_oracle.cpu_planes() + [BLOB]:
        key = (plane.shape, plane.tobytes())
        if key not in seen:
            seen.add(key)
            out.append((name, np.ascontiguousarray(plane, dtype=np.uint8)))
    return out


PLANES = _planes()
_TRACED = {}


def _traced(plane, connectivity):
    """(the source arrays, the run code, the regions' values) of a plane, computed once."""
    key = (plane.shape, plane.tobytes(), connectivity)
    if key not in _TRACED:
        loops = contours_oracle.trace_plane(plane, connectivity)
        row_start, runs = rle_oracle.encode(plane[None])
        _TRACED[key] = (contours_oracle.arrays(loops), (row_start[0], runs[0]), oracle.values_of(plane, loops))
    return _TRACED[key]


def _outlines(plane, connectivity, tolerances=TOLERANCES):
    """(kind, tolerance, (counts, loops, verts)) for the exact outlines, simplify_numpy's and simplify_shared_numpy's."""
    from arseg_amd import egress

    arrays, (row_start, runs), _ = _traced(plane, connectivity)
    H, W = plane.shape
    yield "exact", None, arrays
    for tolerance in tolerances:
        yield "plain", tolerance, egress.simplify_numpy(*arrays, tolerance)
        yield "shared", tolerance, egress.simplify_shared_numpy(row_start, runs, H, W, *arrays, tolerance)


@pytest.mark.parametrize("case", oracle.HAND, ids=oracle.HAND_IDS)
def test_oracle_and_fill_numpy_against_the_literals(case):
    from arseg_amd import egress

    _, H, W, loops, _, gaps, excess, E = case
    for background in (255, 7):
        plane, g, x, k = oracle.fill(loops, oracle.HAND_VALUES, H, W, background)
        assert np.array_equal(plane, oracle.hand_plane(case, background)) and (g, x) == (gaps, excess) and oracle.crossings(loops) == E
        host = egress.fill_numpy(*contours_oracle.arrays(loops), oracle.HAND_VALUES, H, W, background)
        assert host[0].dtype == np.uint8 and np.array_equal(host[0], plane) and host[1:] == (gaps, excess)
        assert oracle.stats(plane, k)[:3].tolist() == [gaps, excess, 0]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", PLANES, ids=[p[0] for p in PLANES])
def test_fill_numpy_equals_the_oracle_and_round_trip(case, connectivity):
    """On every plane, for the exact outlines and both simplifications at every tolerance: fill_numpy gives the oracle's plane, gaps and
    excess; E <= 2 runs (== for the exact outlines); the exact outlines and tolerance 0 give the source plane back."""
    from arseg_amd import egress

    _, plane = case
    H, W = plane.shape
    _, (_, runs), values = _traced(plane, connectivity)
    for kind, tolerance, arrays in _outlines(plane, connectivity):
        loops = contours_oracle.polygons(arrays)
        want, gaps, excess, k = oracle.fill(loops, values, H, W)
        got = egress.fill_numpy(*arrays, values, H, W)
        assert np.array_equal(got[0], want) and got[1:] == (gaps, excess), (kind, tolerance)
        E = oracle.crossings(loops)
        assert E == 2 * len(runs) if kind == "exact" else E <= 2 * len(runs), (kind, tolerance, E)
        if kind == "exact" or tolerance == 0:
            assert np.array_equal(want, plane) and gaps == excess == 0 and oracle.stats(want, k, plane)[2] == 0, (kind, tolerance)


def _partition(plane, connectivity):
    from arseg_amd import egress

    H, W = plane.shape
    arrays, (row_start, runs), values = _traced(plane, connectivity)
    for tolerance in TOLERANCES:
        shared = egress.simplify_shared_numpy(row_start, runs, H, W, *arrays, tolerance)
        _, gaps, excess = egress.fill_numpy(*shared, values, H, W)
        assert gaps == excess == 0, (tolerance, gaps, excess)


VERIFIED = [BLOB, BIG_BLOB] + SHARED_PLANES[:40]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", VERIFIED, ids=[p[0] for p in VERIFIED])
def test_shared_borders_partition_the_frame(case, connectivity):
    """simplify_shared_numpy's polygons leave no pixel uncovered and none covered twice, at every tolerance."""
    _partition(np.ascontiguousarray(case[1], dtype=np.uint8), connectivity)


BEYOND = [p for p in PLANES if all(p[1].shape != q[1].shape or p[1].tobytes() != np.ascontiguousarray(q[1], dtype=np.uint8).tobytes() for q in VERIFIED)]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", BEYOND, ids=[p[0] for p in BEYOND])
def test_shared_borders_partition_the_other_planes(case, connectivity):
    """The same assertion on the planes beyond the set above."""
    _partition(case[1], connectivity)


def test_plain_simplification_does_not_partition():
    """The check discriminates: each loop simplified on its own leaves 9 uncovered pixels on striped-stairs-9 at 1 px, and both gaps and
    doubly covered pixels on the blob plane."""
    from arseg_amd import egress

    stairs = dict(SHARED_PLANES)["striped-stairs-9"]
    arrays, _, values = _traced(stairs, 8)
    assert egress.fill_numpy(*egress.simplify_numpy(*arrays, 1), values, *stairs.shape)[1] == 9
    arrays, _, values = _traced(BLOB[1], 8)
    _, gaps, excess = egress.fill_numpy(*egress.simplify_numpy(*arrays, 1), values, *BLOB[1].shape)
    assert gaps > 0 and excess > 0


def test_fill_numpy_refusals():
    from arseg_amd import egress

    plane = BLOB[1][:8, :8]
    (counts, loops, verts), _, values = _traced(np.ascontiguousarray(plane), 8)
    H, W = plane.shape
    egress.fill_numpy(counts, loops, verts, values, H, W)
    for bad in (dict(H=0), dict(W=0), dict(H=16385), dict(background=256), dict(background=-1), dict(W=W - 1), dict(H=H - 1)):
        with pytest.raises(ValueError):
            egress.fill_numpy(counts, loops, verts, values, **dict(dict(H=H, W=W), **bad))
    with pytest.raises(ValueError):
        egress.fill_numpy(np.array([-1, -1], dtype=np.int32), loops, verts, values, H, W)
    with pytest.raises(ValueError):
        egress.fill_numpy(np.array([counts[0], len(verts) + 1], dtype=np.int32), loops, verts, values, H, W)
    broken = loops.copy()
    broken[0, 2] = 10000
    with pytest.raises(ValueError):
        egress.fill_numpy(counts, broken, verts, values, H, W)
    with pytest.raises(ValueError):
        egress.fill_numpy(counts, loops, verts, values[:-1], H, W)                              # a loop names a region without a value
    open_loop = (np.array([1, 2], dtype=np.int32), np.array([[0, 0, 2, 0]], dtype=np.int32), np.array([0, (2 << 16) | 1], dtype=np.uint32))
    assert egress.fill_numpy(*open_loop, [5], 2, 2)[1:] == (4, 0)                               # two vertices: it cancels itself


def _held(dev="cpu"):
    from arseg_amd import egress

    frames = egress.RleFrames(torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32), 3, 8)
    found = egress.RegionFrames(torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32),
                                torch.zeros((1, 4, 8), dtype=torch.int64), frames)
    counts, loops, verts = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 8, 4), dtype=torch.int32), torch.zeros((1, 32), dtype=torch.int32)
    return found, egress.ContourFrames(counts, loops, verts, found)


def test_wrappers_refuse_without_a_gpu():
    from arseg_amd import _lib, egress, ops

    found, held = _held()
    with pytest.raises(ValueError):
        egress.fill(found)
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            egress.fill(held, background=bad)
    with pytest.raises(ValueError):
        egress.fill(held, event_capacity=-1)
    with pytest.raises(_lib.ArsegError, match="fill_numpy is the host form"):
        egress.fill(held)
    with pytest.raises(ValueError):
        egress.fill(held, out=held)
    labels, counts, stats = torch.zeros((1, 3, 8), dtype=torch.uint8), torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 771), dtype=torch.int64)
    with pytest.raises(ValueError):
        egress.FilledFrames(labels, counts, stats, found, 16)
    with pytest.raises(ValueError):
        egress.FilledFrames(labels, counts, torch.zeros((1, 99), dtype=torch.int64), held, 16)
    done = egress.FilledFrames(labels, counts, stats, held, 16)
    assert done.needed() is done.counts and done.N == 1 and done.contours is held and done.event_capacity == 16 and _lib.FILL_NSTATS == 771
    with pytest.raises(ValueError):
        egress.fill(held, out=egress.FilledFrames(torch.zeros((1, 4, 8), dtype=torch.uint8), counts, stats, held, 16))      # another H
    # fidelity: from the counters alone
    stats[0, :3] = torch.tensor([2, 1, 5])
    stats[0, 3 + 4], stats[0, 3 + 256 + 4], stats[0, 3 + 512 + 4] = 10, 12, 8
    stats[0, 3 + 9] = 14
    counts[0] = 6
    (row,) = done.fidelity()
    assert (row["gaps"], row["excess"], row["changed"]) == (2, 1, 5) and row["iou"] == {4: 8 / 14, 9: 0.0} and row["miou"] == (8 / 14) / 2
    counts[0] = 17
    with pytest.raises(_lib.ArsegError, match="frame 0 needs 17 crossings, the capacity is 16"):
        done.fidelity()
    counts[0] = -1
    with pytest.raises(_lib.ArsegError, match="frame 0 could not be processed"):
        done.fidelity()
    args = (held.counts, held.loops, held.verts, found.n_regions, found.records)
    with pytest.raises(ValueError):
        ops.contours_fill(*args, 16385, 8, labels, counts)
    with pytest.raises(ValueError):
        ops.contours_fill(*args, 3, 0, labels, counts)
    with pytest.raises(ValueError):
        ops.contours_fill(*args, 3, 8, labels, counts, background=300)
    with pytest.raises(ValueError):
        ops.contours_fill(*args, 3, 8, labels, counts, event_capacity=-2)
    with pytest.raises(ValueError):
        ops.contours_fill(*args, 3, 8, None, counts, event_capacity=4)
    with pytest.raises(_lib.ArsegError):
        ops.contours_fill(*args, 3, 8, labels, counts)                                          # CPU tensors


def test_polygon_fidelity_goes_through_polygons_and_fill():
    """alter_res_batch_polygons keeps its signature; alter_res_batch_polygon_fidelity calls it, then egress.fill against the labels."""
    from arseg_amd import egress, evaluation

    sig = inspect.signature(evaluation.alter_res_batch_polygons)
    assert list(sig.parameters)[-1] == "shared_borders" and sig.parameters["shared_borders"].default is False and len(sig.parameters) == 17
    mine = inspect.signature(evaluation.alter_res_batch_polygon_fidelity)
    assert list(mine.parameters)[:7] == ["lr_net", "ref_ps", "imgs", "mv_qs", "capacity", "region_capacity", "tolerance"]
    assert mine.parameters["shared_borders"].default is False and mine.parameters["background"].default == 255
    seen = []
    real = evaluation.alter_res_batch_polygons, egress.fill
    try:
        evaluation.alter_res_batch_polygons = lambda *a, **k: seen.append(("polygons", a[6], k["shared_borders"])) or ("polys", "labels")
        egress.fill = lambda polygons, background=255, ref=None: seen.append(("fill", polygons, background, ref)) or "filled"
        assert evaluation.alter_res_batch_polygon_fidelity(None, [], None, None, 8, 8, 1.5, shared_borders=True, background=9) == ("polys", "filled", "labels")
    finally:
        evaluation.alter_res_batch_polygons, egress.fill = real
    assert seen == [("polygons", 1.5, True), ("fill", "polys", 9, "labels")]


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, egress, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arseg_hip.h")).read(), flags=re.S)
    for name in ("arseg_contours_fill_fwd", "arseg_contours_fill_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
        declared = re.search(r"%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["arseg_contours_fill_fwd"][1]) == 24 and len(_lib.PROTOTYPES["arseg_contours_fill_workspace_bytes"][1]) == 6
    assert re.search(r"#define\s+ARSEG_FILL_NSTATS\s+\(3 \+ 3 \* 256\)", text) and _lib.FILL_NSTATS == oracle.NSTATS == 771
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.contours_fill) and callable(egress.fill) and callable(egress.fill_numpy) and callable(egress.FilledFrames.rle)


def test_workspace_bytes():
    """Per frame 8 bytes per crossing slot and 8 per row and one more; beyond 8192 columns an owner line of 4 W bytes per workgroup of the
    row launch; in all rounded up to 16; nothing for sizes the entry point refuses; SIZE_MAX for sizes beyond size_t."""
    from arseg_amd import _lib

    f = _lib.load().arseg_contours_fill_workspace_bytes
    up = lambda b: (b + 15) // 16 * 16
    for N, H, W, ecap in ((1, 1, 1, 0), (1, 4, 4, 16), (3, 100, 65, 401), (4, 1024, 2048, 100000), (2, 16384, 8192, 1 << 31)):
        assert f(N, H, W, 7, 9, ecap) == up(N * (8 * ecap + 8 * (H + 1))), (N, H, W, ecap)
    for N, H, groups in ((1, 3, 3), (2, 100, 200), (1, 16384, 256), (4, 16384, 256)):
        assert f(N, H, 8193, 0, 0, 10) == up(N * (80 + 8 * (H + 1)) + groups * 4 * 8193), (N, H)
    for bad in ((0, 4, 4, 1, 1, 1), (-1, 4, 4, 1, 1, 1), (1, 0, 4, 1, 1, 1), (1, 4, 0, 1, 1, 1), (1, 16385, 4, 1, 1, 1), (1, 4, 16385, 1, 1, 1),
                (1, 4, 4, -1, 1, 1), (1, 4, 4, 1, -1, 1), (1, 4, 4, 1, 1, -1)):
        assert f(*bad) == 0
    for huge in ((1, 4, 4, 0, 0, (1 << 63) - 1), (2, 4, 4, 0, 0, 1 << 60), ((1 << 31) - 1, 4, 4, 0, 0, 1 << 40)):
        assert f(*huge) == (1 << 64) - 1                                                        # does not fit size_t: no workspace is that large


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(0)
    at = lambda k: ctypes.c_void_p(64 * k)
    EINVAL, EWORKSPACE = _lib.ARSEG_EINVAL, _lib.ARSEG_EWORKSPACE
    N, H, W, lcap, vcap, rcap, ecap = 2, 8, 24, 50, 200, 30, 120
    enough = lib.arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, ecap)
    assert enough == N * (8 * ecap + 8 * (H + 1))
    names = ("counts", "loops", "lcap", "verts", "vcap", "n_regions", "records", "rcap", "N", "H", "W", "background", "ref_labels", "ref_pitch",
             "ref_image_stride", "labels_out", "pitch", "image_stride", "counts_out", "stats", "ecap", "workspace", "workspace_bytes")
    good = dict(zip(names, (at(1), at(2), lcap, at(3), vcap, at(4), at(5), rcap, N, H, W, 255, at(6), W, H * W, at(7), W + 8, H * (W + 8) + 5, at(8),
                            at(9), ecap, at(10), enough)))

    def call(**changed):
        return lib.arseg_contours_fill_fwd(*[dict(good, **changed)[k] for k in names], null)

    for name in ("counts", "loops", "verts", "n_regions", "records", "labels_out", "counts_out"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer (with a positive capacity)
    for name in ("counts", "loops", "verts", "n_regions", "counts_out", "records", "stats", "workspace"):
        for address in (1025, 1026, 1027):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte aligned
    for name in ("records", "stats", "workspace"):
        assert call(**{name: ctypes.c_void_p(1028)}) == EINVAL                                  # not 8-byte aligned
    for name in ("N", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(H=16385) == EINVAL and call(W=16385, pitch=1 << 20, ref_pitch=1 << 20) == EINVAL
    for name in ("lcap", "vcap", "rcap", "ecap"):
        assert call(**{name: -1}) == EINVAL
    assert call(background=-1) == EINVAL and call(background=256) == EINVAL
    assert call(pitch=W - 1) == EINVAL and call(ref_pitch=W - 1) == EINVAL and call(image_stride=-1) == EINVAL and call(ref_image_stride=-1) == EINVAL
    for out in ("labels_out", "counts_out", "stats"):                                           # an output that is any of the inputs
        for src in ("counts", "loops", "verts", "n_regions", "records", "ref_labels"):
            assert call(**{out: good[src]}) == EINVAL
    assert call(stats=good["labels_out"]) == EINVAL and call(counts_out=good["labels_out"]) == EINVAL and call(stats=good["counts_out"]) == EINVAL
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == EWORKSPACE and call(workspace_bytes=0) == EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == EWORKSPACE
    assert call(labels_out=null, ecap=0, workspace_bytes=0) == EWORKSPACE                       # the sizing form passes the checks
    assert call(stats=null, workspace_bytes=0) == EWORKSPACE and call(ref_labels=null, ref_pitch=0, workspace_bytes=0) == EWORKSPACE
    assert call(H=16384, W=16384, pitch=16384, ref_pitch=16384, workspace_bytes=0) == EWORKSPACE
    assert call(loops=null, lcap=0, verts=null, vcap=0, records=null, rcap=0, workspace_bytes=0) == EWORKSPACE
    assert call(workspace_bytes=0, background=256) == EINVAL and call(workspace_bytes=0, N=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    for huge in (dict(ecap=(1 << 63) - 1), dict(ecap=1 << 60), dict(N=(1 << 31) - 1, ecap=1 << 40)):
        assert call(workspace_bytes=0, **huge) == EWORKSPACE and call(workspace_bytes=(1 << 64) - 1, **huge) == EWORKSPACE      # a size beyond size_t


def test_documented():
    """The header, DESIGN.md, README.md and INTEGRATION.md describe the pass, and what is left out is said."""
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    assert "xs = ceil((2 xa dy + t (xb - xa) - dy) / (2 dy))" in header and "never spans more rows than the chain it replaces" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.15" in design and "fill.hip" in design
    assert "egress.fill" in open(os.path.join(ROOT, "README.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "egress.fill" in integration and "anti-aliased" in integration and "winding" in integration
