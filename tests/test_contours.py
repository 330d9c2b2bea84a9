"""CPU checks of the region outlines (include/arseg_hip.h, arseg_rle_contours_fwd; arseg_amd.egress.contours): the oracle against loops
written out by hand, its invariants (axes alternate, shoelace areas add up to the regions' areas, an even-odd fill gives the regions back,
the bounds behind the default capacities), the pure-numpy host form against the oracle, the wrappers' refusals and every ARSEG_EINVAL /
ARSEG_EWORKSPACE case through ctypes (the library loads without a GPU).  Everything is an integer: every comparison is np.array_equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import contours_oracle as oracle
import links_oracle
import regions_oracle
import rle_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = oracle.cpu_planes()
PLANE_IDS = [p[0] for p in PLANES]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_oracle_against_the_literals(name, connectivity):
    got = oracle.trace_plane(oracle.hand_plane(name), connectivity)
    assert got == [(r, hole, list(pts)) for r, hole, pts in oracle.HAND[name][1][connectivity]]


def test_the_literals_say_what_they_should():
    by = oracle.HAND
    assert by["one-pixel"][1][8] == [(0, 0, [(0, 0), (1, 0), (1, 1), (0, 1)])]
    centre = by["centre"][1][4]
    assert [l[:2] for l in centre] == [(0, 0), (0, 1), (1, 0)] and centre[1][2] == [(1, 1), (1, 2), (2, 2), (2, 1)]
    assert [len(l[2]) for l in by["diagonal"][1][8]] == [8, 8] and [l[2][0] for l in by["diagonal"][1][4]] == [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert by["diagonal"][1][8][0][2].count((1, 1)) == 2                                        # through the saddle twice
    assert len(by["l-shape"][1][8][0][2]) == 6                                                  # no vertex at (0, 1) or (0, 2)
    assert [l[1] for l in by["two-holes"][1][8]] == [0, 1, 0, 1, 0] and len(by["cup-hole"][1][8][1][2]) == 8
    assert by["one-row"][0] == [[4, 4, 9, 4, 4, 4]] and by["one-column"][0] == [[1], [1], [2], [1]]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", PLANES, ids=PLANE_IDS)
def test_oracle_invariants(case, connectivity):
    """Axes alternate and loops close; per region the shoelace areas of its loops (outer positive, holes negative) add up to the area of
    regions_oracle's record; filling each region's loops by the even-odd rule gives the region's pixels back; L <= runs, V <= 4 runs."""
    plane = case[1]
    H, W = plane.shape
    answer = oracle.contour_plane(plane, connectivity)
    side = links_oracle.region_planes(plane[None], connectivity)[0]
    R, _, records = regions_oracle.label_planes(plane[None], connectivity)[0]
    polys = oracle.polygons(answer)
    assert answer[0][0] == len(polys) <= len(side["runs"]) and answer[0][1] <= 4 * len(side["runs"])
    area2 = np.zeros(R, dtype=np.int64)
    by_region = {}
    for r, hole, pts in polys:
        step = np.roll(pts, -1, axis=0) - pts
        assert len(pts) >= 4 and len(pts) % 2 == 0
        assert ((step != 0).sum(axis=1) == 1).all()                                              # one coordinate changes per step
        assert ((step[:, 0] != 0) != np.roll(step[:, 0] != 0, 1)).all()                          # and the axes alternate
        assert (pts[0, 1], pts[0, 0]) == min((y, x) for x, y in pts)
        a = oracle.shoelace2(pts)
        assert (a < 0) == bool(hole)
        area2[r] += a
        by_region.setdefault(r, []).append(pts)
    assert np.array_equal(area2, 2 * records[:, 1]) and sorted(by_region) == list(range(R))
    for r, loops in by_region.items():
        assert np.array_equal(oracle.fill_even_odd(loops, H, W), side["reg"] == r), r
    firsts = [(pts[0, 1], pts[0, 0], -hole) for _, hole, pts in polys]
    assert firsts == sorted(firsts)
    starts = answer[1][:, 1]
    assert np.array_equal(starts, np.cumsum(answer[1][:, 2]) - answer[1][:, 2])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", PLANES, ids=PLANE_IDS)
def test_contours_numpy_equals_the_oracle(case, connectivity):
    from arseg_amd import egress

    plane = case[1]
    H, W = plane.shape
    row_start, runs = rle_oracle.encode(plane[None])
    got = egress.contours_numpy(row_start[0], runs[0], H, W, connectivity)
    want = oracle.contour_plane(plane, connectivity)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_the_long_loops_are_long():
    """The spirals' walls and the comb are one loop each: more run ends (the loop's vertical length) than a wave has lanes, and in the
    larger spiral than a workgroup has threads."""
    for name, least in (("spiral-21x21", 65), ("comb-40-teeth", 65), ("spiral-33x33", 257)):
        longest = max(int(np.abs(np.roll(pts, -1, axis=0) - pts)[:, 1].sum()) for _, _, pts in oracle.polygons(oracle.contour_plane(oracle.LONG[name], 8)))
        assert longest >= least, (name, longest)


def test_contours_numpy_refusals():
    from arseg_amd import egress

    row_start, runs = rle_oracle.encode(oracle.hand_plane("one-row")[None])
    with pytest.raises(ValueError):
        egress.contours_numpy(row_start[0], runs[0], 1, 6, connectivity=6)
    with pytest.raises(ValueError):
        egress.contours_numpy(row_start[0], runs[0], 2, 6)
    with pytest.raises(ValueError):
        egress.contours_numpy(row_start[0], runs[0], 1, 65536)


def test_wrappers_refuse_without_a_gpu():
    from arseg_amd import _lib, egress, ops

    rs, runs = torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32)
    frames = egress.RleFrames(rs, runs, 3, 8)
    found = egress.RegionFrames(torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32),
                                torch.zeros((1, 4, 8), dtype=torch.int64), frames)
    counts, loops, verts = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 8, 4), dtype=torch.int32), torch.zeros((1, 32), dtype=torch.int32)
    with pytest.raises(ValueError):
        egress.contours(frames)
    with pytest.raises(ValueError):
        egress.contours(found, loop_capacity=-1)
    with pytest.raises(_lib.ArsegError):
        egress.contours(found)
    with pytest.raises(ValueError):
        egress.contours(found, out=frames)
    with pytest.raises(ValueError):
        ops.rle_contours(rs, runs, found.n_regions, found.run_region, 3, 8, counts, connectivity=6)
    with pytest.raises(ValueError):
        ops.rle_contours(rs, runs, found.n_regions, found.run_region, 65536, 8, counts)
    with pytest.raises(_lib.ArsegError):
        ops.rle_contours(rs, runs, found.n_regions, found.run_region, 3, 8, counts, loops, verts)
    with pytest.raises(ValueError):
        egress.ContourFrames(counts, loops, torch.zeros((2, 32), dtype=torch.int32), found)
    held = egress.ContourFrames(torch.tensor([[-1, -1]], dtype=torch.int32), loops, verts, found)
    assert held.needed() is held.counts and held.source is found and (held.loop_capacity, held.vertex_capacity) == (8, 32)
    with pytest.raises(_lib.ArsegError, match="frame 0 could not be processed"):
        held.to_host()
    held.counts[0] = torch.tensor([9, 20], dtype=torch.int32)
    with pytest.raises(_lib.ArsegError, match="frame 0 needs 9 loops and 20 vertices"):
        held.to_host()
    held.counts[0] = torch.tensor([1, 4], dtype=torch.int32)
    held.loops[0, 0] = torch.tensor([0, 0, 4, 0], dtype=torch.int32)
    held.verts[0, :4] = torch.tensor([0, 8, (3 << 16) | 8, 3 << 16], dtype=torch.int32)
    (region, hole, pts), = held.to_host()[0]
    assert (region, hole) == (0, 0) and pts.dtype == np.int32 and pts.tolist() == [[0, 0], [8, 0], [8, 3], [0, 3]]


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, egress, evaluation, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arseg_hip.h")).read(), flags=re.S)
    for name in ("arseg_rle_contours_fwd", "arseg_rle_contours_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
        declared = re.search(r"%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["arseg_rle_contours_fwd"][1]) == 17
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.rle_contours) and callable(evaluation.alter_res_batch_contours) and callable(egress.contours)
    assert callable(egress.contours_numpy)


def test_workspace_bytes():
    """80 bytes per run slot: per run end a successor, a corner and two 16-byte states; nothing for sizes the entry point refuses."""
    from arseg_amd import _lib

    f = _lib.load().arseg_rle_contours_workspace_bytes
    assert f(1, 1) == 80 and f(11, 40000) == 11 * 40000 * 80
    assert f(3, 1 << 29) == 3 * (1 << 29) * 80                                                   # beyond 32 bits
    for bad in ((0, 10), (-1, 10), (2, 0), (2, -5)):
        assert f(*bad) == 0
    sizes = [f(2, c) for c in (1, 2, 3, 64, 65, 1000)]
    assert sizes == sorted(set(sizes)) and all(s % 16 == 0 for s in sizes)


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    EINVAL = _lib.ARSEG_EINVAL
    N, cap, H = 2, 50, 8
    enough = N * cap * 80
    names = ("row_start", "runs", "n_regions", "run_region", "cap", "N", "H", "W", "connectivity", "counts", "loops", "lcap", "verts", "vcap",
             "workspace", "workspace_bytes")
    good = dict(zip(names, (one, one, one, one, cap, N, H, 24, 8, one, one, cap, one, 4 * cap, one, enough)))

    def call(**changed):
        return lib.arseg_rle_contours_fwd(*[dict(good, **changed)[k] for k in names], null)

    for name in ("row_start", "runs", "n_regions", "run_region", "counts"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer
    for name in ("row_start", "runs", "n_regions", "run_region", "counts", "loops", "verts", "workspace"):
        for address in (65, 66, 67):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte aligned
    for name in ("N", "H", "W", "cap"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(lcap=-1) == EINVAL and call(vcap=-1) == EINVAL
    assert call(loops=null) == EINVAL and call(verts=null) == EINVAL                            # wanted, nowhere to put them
    for connectivity in (0, 6, -8, 16):
        assert call(connectivity=connectivity) == EINVAL
    assert call(H=65536) == EINVAL and call(W=65536) == EINVAL                                  # the vertex word
    assert call(cap=(1 << 29) + 1, workspace_bytes=1 << 62) == EINVAL
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == _lib.ARSEG_EWORKSPACE and call(workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(loops=null, lcap=0, verts=null, vcap=0, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE      # the sizing forms pass the checks
    assert call(loops=null, lcap=0, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(H=65535, W=65535, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace_bytes=0, connectivity=5) == EINVAL and call(workspace_bytes=0, cap=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    assert lib.arseg_rle_contours_workspace_bytes(N, cap) == enough


def test_documented():
    """The header points from the "Not covered" lists of the regions and of the overlays to the new entry point and states the bounds
    behind the default capacities; DESIGN.md and README.md describe it."""
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    assert header.count("arseg_rle_contours_fwd, below") == 2 and "lcap = cap and vcap = 4 x cap never overflow" in header
    assert "### 6.12" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "contours" in open(os.path.join(ROOT, "README.md")).read()
