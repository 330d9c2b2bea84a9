"""CPU checks of the simplified outlines (include/arseg_hip.h, arseg_contours_simplify_fwd; arseg_amd.egress.simplify): the oracle against
kept vertices written out by hand, its invariants (a subsequence with the same first vertex, at least 3 vertices or the loop unchanged,
tolerance 0 the identity, every dropped vertex within the tolerance of the kept pair around it, first' the prefix sum, V' <= V), the
pure-numpy host form against the oracle, the wrappers' refusals and every ARSEG_EINVAL / ARSEG_EWORKSPACE case through ctypes (the
library loads without a GPU).  Everything is an integer: every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import contours_oracle
import simplify_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = oracle.cpu_planes()
PLANE_IDS = [p[0] for p in PLANES]
TOLS = list(oracle.TOLERANCES.items())

_TRACED = {}


def _traced(name, plane, connectivity):
    """contours_oracle's answer for a plane, computed once."""
    key = (name, connectivity)
    if key not in _TRACED:
        _TRACED[key] = contours_oracle.contour_plane(plane, connectivity)
    return _TRACED[key]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_oracle_against_the_literals(name, connectivity):
    loops = contours_oracle.trace_plane(oracle.hand_plane(name), connectivity)
    assert sorted(oracle.HAND[name][1]) == sorted(oracle.TOL2_QS)
    for tol2_q in oracle.TOL2_QS:
        assert oracle.simplify_loops(loops, tol2_q) == oracle.HAND[name][1][tol2_q], tol2_q


def test_the_literals_say_what_they_should():
    by = oracle.HAND
    assert oracle.TOLERANCES == {0.0: 0, 0.5: 4, 1.0: 16, 1.5: 36, 2.0: 64, 256.0: 1 << 20}
    assert all(16 * t * t == q for t, q in oracle.TOLERANCES.items())
    assert by["unit-square"][1][16] == [(0, 0, [(0, 0), (1, 0), (1, 1), (0, 1)])]                  # rule 3
    assert all(by["rectangle-4x2"][1][q] == [(0, 0, [(0, 0), (4, 0), (4, 2), (0, 2)])] for q in oracle.TOL2_QS)
    stairs = by["stairs"][1]
    assert len(stairs[0][0][2]) == 14 and len(stairs[4][0][2]) == 12 and stairs[16][0][2] == [(0, 0), (6, 6), (0, 6)]
    hole, inside = by["cup-hole"][1][16][1:]
    assert hole[1] == 1 and inside[1] == 0 and sorted(hole[2]) == sorted(inside[2]) and hole[2] != inside[2]      # either direction
    assert contours_oracle.shoelace2(hole[2]) < 0 < contours_oracle.shoelace2(inside[2])
    # the ties: the smaller position stays
    notch = by["notch-tie"][1]
    assert (2, 1) in notch[4][0][2] and (1, 1) not in notch[4][0][2]
    square = by["notched-square"][1]
    assert (4, 3) in square[16][0][2] and (3, 4) not in square[16][0][2]
    assert by["plus"][1][4][1][2] == [(1, 0), (3, 1), (2, 3), (0, 2)]


def _check_invariants(source, got, tol2_q):
    """source, got: (counts, loops, verts) before and after."""
    before, after = oracle.loops_of(source), oracle.loops_of(got)
    assert got[0][0] == source[0][0] == len(after) == len(before) and got[0][1] <= source[0][1]
    assert np.array_equal(got[1][:, 1], np.cumsum(got[1][:, 2]) - got[1][:, 2]) and got[0][1] == got[1][:, 2].sum() == len(got[2])
    assert np.array_equal(got[1][:, [0, 3]], source[1][:, [0, 3]])
    for (_, _, pts), (_, _, kept) in zip(before, after):
        assert kept[0] == pts[0]
        if kept == pts:
            continue
        assert tol2_q > 0 and len(kept) >= 3
        at, where = 0, []
        for q in kept:                                                                           # a subsequence, in order
            while pts[at] != q:
                at += 1
            where.append(at)
            at += 1
        assert where[0] == 0
        closed = pts + [pts[0]]
        for a, b in zip(where, where[1:] + [len(pts)]):
            len2 = (closed[b][0] - closed[a][0]) ** 2 + (closed[b][1] - closed[a][1]) ** 2
            assert len2 > 0
            for i in range(a + 1, b):
                c = abs((closed[b][0] - closed[a][0]) * (closed[i][1] - closed[a][1]) - (closed[b][1] - closed[a][1]) * (closed[i][0] - closed[a][0]))
                assert 16 * c * c <= tol2_q * len2, (a, i, b)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", PLANES, ids=PLANE_IDS)
def test_oracle_invariants_and_simplify_numpy(case, connectivity):
    """On every plane at every tolerance: the invariants of the contract hold for the oracle's answer, tolerance 0 is the identity, and
    egress.simplify_numpy gives the oracle's arrays."""
    from arseg_amd import egress

    source = _traced(case[0], case[1], connectivity)
    for tolerance, tol2_q in TOLS:
        want = oracle.simplify_frame(source, tol2_q)
        _check_invariants(source, want, tol2_q)
        if tol2_q == 0:
            assert all(np.array_equal(w, s) for w, s in zip(want, source))
        got = egress.simplify_numpy(*source, tolerance)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (tolerance,)


def test_simplification_shrinks_the_long_loops():
    """The cases are not all trivial: at 1 px the spirals and the blob-like planes lose vertices, and a loop stays above 64 vertices."""
    for name in ("spiral-33x33", "comb-40-teeth"):
        source = _traced(name, np.ascontiguousarray(contours_oracle.LONG[name]), 8)
        assert source[1][:, 2].max() > 64
    source = _traced("stairs-40", oracle.staircase(40), 8)
    got = oracle.simplify_frame(source, 16)
    assert source[1][0, 2] == 82 and got[1][0, 2] == 3


def test_simplify_numpy_refusals():
    from arseg_amd import egress

    source = contours_oracle.contour_plane(oracle.hand_plane("stairs"))
    for bad in (-1, -0.25, 0.1, 0.3, float("nan"), float("inf"), 1e9):
        with pytest.raises(ValueError):
            egress.simplify_numpy(*source, bad)
    with pytest.raises(ValueError):
        egress.simplify_numpy(np.array([2, 99], dtype=np.int32), source[1], source[2], 1)
    with pytest.raises(ValueError):
        egress.simplify_numpy(np.array([-1, -1], dtype=np.int32), source[1], source[2], 1)
    broken = source[1].copy()
    broken[1, 2] = 1000
    with pytest.raises(ValueError):
        egress.simplify_numpy(source[0], broken, source[2], 1)
    for fine in (0, 0.25, 0.75, 1, 2.5, np.float32(1.5)):
        egress.simplify_numpy(*source, fine)


def test_wrappers_refuse_without_a_gpu():
    from arseg_amd import _lib, egress, ops

    rs, runs = torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32)
    frames = egress.RleFrames(rs, runs, 3, 8)
    found = egress.RegionFrames(torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32),
                                torch.zeros((1, 4, 8), dtype=torch.int64), frames)
    counts, loops, verts = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 8, 4), dtype=torch.int32), torch.zeros((1, 32), dtype=torch.int32)
    held = egress.ContourFrames(counts, loops, verts, found)
    with pytest.raises(ValueError):
        egress.simplify(found, 1)
    for bad in (-1, 0.1, float("nan")):
        with pytest.raises(ValueError):
            egress.simplify(held, bad)
    with pytest.raises(ValueError):
        egress.simplify(held, 1, vertex_capacity=-1)
    with pytest.raises(_lib.ArsegError, match="simplify_numpy is the host form"):
        egress.simplify(held, 1)
    with pytest.raises(ValueError):
        egress.simplify(held, 1, out=held)
    with pytest.raises(ValueError):
        egress.SimplifiedContours(counts, loops, verts, found, 1)
    with pytest.raises(ValueError):
        egress.SimplifiedContours(counts, torch.zeros((1, 7, 4), dtype=torch.int32), verts, held, 1)
    done = egress.SimplifiedContours(counts.clone(), loops.clone(), torch.zeros((1, 16), dtype=torch.int32), held, 1.5)
    assert isinstance(done, egress.ContourFrames) and done.contours is held and done.tolerance == 1.5 and done.source is found
    assert done.needed() is done.counts and (done.loop_capacity, done.vertex_capacity) == (8, 16)
    with pytest.raises(ValueError):
        egress.simplify(egress.ContourFrames(counts, torch.zeros((1, 9, 4), dtype=torch.int32), verts, found), 1, out=done)
    done.counts[0] = torch.tensor([1, 3], dtype=torch.int32)
    done.loops[0, 0] = torch.tensor([0, 0, 3, 0], dtype=torch.int32)
    done.verts[0, :3] = torch.tensor([0, (3 << 16) | 8, 3 << 16], dtype=torch.int32)
    (region, hole, pts), = done.to_host()[0]
    assert (region, hole) == (0, 0) and pts.tolist() == [[0, 0], [8, 3], [0, 3]]
    out = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.contours_simplify(counts, loops, verts, 3, 8, 0.3, out)
    with pytest.raises(ValueError):
        ops.contours_simplify(counts, loops, verts, 16385, 8, 1, out)
    with pytest.raises(ValueError):
        ops.contours_simplify(counts, loops, verts, 3, 0, 1, out)
    with pytest.raises(_lib.ArsegError):
        ops.contours_simplify(counts, loops, verts, 3, 8, 1, out, loops.clone(), verts.clone())
    assert ops.tolerance_q(0) == 0 and ops.tolerance_q(0.5) == 4 and ops.tolerance_q(1) == 16 and ops.tolerance_q(1.5) == 36 and ops.tolerance_q(2) == 64
    assert ops.tolerance_q(8192) == 1 << 30
    with pytest.raises(ValueError):
        ops.tolerance_q(8192.25)


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, egress, evaluation, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arseg_hip.h")).read(), flags=re.S)
    for name in ("arseg_contours_simplify_fwd", "arseg_contours_simplify_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
        declared = re.search(r"%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["arseg_contours_simplify_fwd"][1]) == 16
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.contours_simplify) and callable(evaluation.alter_res_batch_polygons) and callable(egress.simplify)
    assert callable(egress.simplify_numpy) and issubclass(egress.SimplifiedContours, egress.ContourFrames)


def test_workspace_bytes():
    """Per frame 4 bytes per loop slot and a byte per vertex slot (rounded up to 4), in all rounded up to 16; nothing for sizes the
    entry point refuses."""
    from arseg_amd import _lib

    f = _lib.load().arseg_contours_simplify_workspace_bytes
    assert f(1, 1, 1) == 16 and f(1, 4, 16) == 32 and f(3, 100, 401) == 3 * (400 + 404) + 4 and f(2, 0, 0) == 0
    assert f(11, 40000, 160000) == 11 * (160000 + 160000)
    assert f(3, 1 << 29, 1 << 31) == 3 * ((1 << 31) + (1 << 31))                                  # beyond 32 bits
    for bad in ((0, 10, 10), (-1, 10, 10), (2, -1, 10), (2, 10, -5)):
        assert f(*bad) == 0
    for huge in ((2, 1 << 60, 1 << 62), (1, (1 << 63) - 1, 0), (1, 0, (1 << 63) - 1), ((1 << 31) - 1, 1 << 40, 1 << 40)):
        assert f(*huge) == (1 << 64) - 1                                                        # does not fit size_t: no workspace is that large
    sizes = [f(2, c, 4 * c) for c in (1, 2, 3, 64, 65, 1000)]
    assert sizes == sorted(set(sizes)) and all(s % 16 == 0 for s in sizes)


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(0)
    at = lambda k: ctypes.c_void_p(64 * k)
    EINVAL, EWORKSPACE = _lib.ARSEG_EINVAL, _lib.ARSEG_EWORKSPACE
    N, lcap, vcap = 2, 50, 200
    enough = lib.arseg_contours_simplify_workspace_bytes(N, lcap, vcap)
    assert enough == N * (4 * lcap + vcap)
    names = ("counts", "loops", "lcap", "verts", "vcap", "N", "H", "W", "tol2_q", "counts_out", "loops_out", "verts_out", "vcap_out", "workspace",
             "workspace_bytes")
    good = dict(zip(names, (at(1), at(2), lcap, at(3), vcap, N, 8, 24, 16, at(4), at(5), at(6), vcap, at(7), enough)))

    def call(**changed):
        return lib.arseg_contours_simplify_fwd(*[dict(good, **changed)[k] for k in names], null)

    for name in ("counts", "counts_out", "loops", "loops_out", "verts", "verts_out"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer with a positive capacity
    for name in ("counts", "loops", "verts", "counts_out", "loops_out", "verts_out", "workspace"):
        for address in (1025, 1026, 1027):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte aligned
    for name in ("N", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(lcap=-1) == EINVAL and call(vcap=-1) == EINVAL and call(vcap_out=-1) == EINVAL
    assert call(H=16385) == EINVAL and call(W=16385) == EINVAL                                  # the range of the 32-bit products
    assert call(tol2_q=-1) == EINVAL and call(tol2_q=(1 << 30) + 1) == EINVAL
    assert call(verts_out=good["verts"]) == EINVAL and call(loops_out=good["loops"]) == EINVAL  # in place
    assert call(counts_out=good["counts"]) == EINVAL
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == EWORKSPACE and call(workspace_bytes=0) == EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == EWORKSPACE
    assert call(verts_out=null, vcap_out=0, workspace_bytes=0) == EWORKSPACE                    # the sizing form passes the checks
    assert call(H=16384, W=16384, tol2_q=1 << 30, workspace_bytes=0) == EWORKSPACE and call(tol2_q=0, workspace_bytes=0) == EWORKSPACE
    assert call(vcap_out=1, workspace_bytes=0) == EWORKSPACE
    assert call(workspace_bytes=0, tol2_q=-1) == EINVAL and call(workspace_bytes=0, N=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    for huge in (dict(lcap=1 << 60, vcap=1 << 62), dict(lcap=(1 << 63) - 1), dict(vcap=(1 << 63) - 1), dict(N=(1 << 31) - 1, lcap=1 << 40)):
        assert call(workspace_bytes=0, **huge) == EWORKSPACE and call(workspace_bytes=(1 << 64) - 1, **huge) == EWORKSPACE      # a size beyond size_t
    assert call(loops=null, loops_out=null, lcap=0, verts=null, vcap=0, verts_out=null, vcap_out=0, workspace=null, workspace_bytes=0) == EINVAL


def test_documented():
    """The header, DESIGN.md, README.md and INTEGRATION.md describe the pass; what is left out is said."""
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    assert "tol2_q = 16 x the squared tolerance" in header and "simplified once per loop" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.13" in design and "simplified twice" in design
    assert "simplify" in open(os.path.join(ROOT, "README.md")).read()
    assert "egress.simplify" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
