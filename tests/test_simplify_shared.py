"""CPU checks of the outlines simplified with shared borders (include/arseg_hip.h, arseg_contours_simplify_shared_fwd;
arseg_amd.egress.simplify_shared): the oracle against kept loops written out by hand, its invariants on every plane -- the matching
property (every directed segment off the frame has its reverse in the neighbour's loop), tolerance 0 the expanded loop, a subsequence
in order, every junction passage kept, every dropped vertex within the tolerance of the kept pair around it, first' the prefix sum,
V' <= V + 2 runs, count' >= 2 --, the pure-numpy host form against the oracle, the wrappers' refusals and every ARSEG_EINVAL /
ARSEG_EWORKSPACE case through ctypes (the library loads without a GPU).  Everything is an integer: every comparison is exact."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import contours_oracle
import rle_oracle
import simplify_oracle
import simplify_shared_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = oracle.cpu_planes()
PLANE_IDS = [p[0] for p in PLANES]
TOLS = list(oracle.TOLERANCES.items())


@pytest.mark.parametrize("case", oracle.HAND, ids=oracle.HAND_IDS)
def test_oracle_against_the_literals(case):
    _, rows, connectivity, tol2_q, loops = case
    kept, segments, _, _ = oracle.simplify_plane(np.array(rows, dtype=np.uint8), connectivity, tol2_q)
    assert kept == loops and not oracle.unmatched(segments)


def test_the_literals_say_what_they_should():
    by = {(h[0], h[2], h[3]): h[4] for h in oracle.HAND}
    assert (1, 1) in by[("t-horizontal", 8, 0)][0][2] and by[("t-horizontal", 8, 0)] == by[("t-horizontal", 8, 1 << 20)]      # the inserted T stays
    assert by[("t-vertical", 8, 0)][0][2] == [(0, 0), (1, 0), (1, 1), (1, 2), (0, 2)]
    for q in (4, 16):                                                                          # the staircase: the same vertices on both sides
        a, b = by[("stairs", 8, q)]
        inner = lambda pts: set(p for p in pts if 0 < p[0] < 6 and 0 < p[1] < 6)
        assert inner(a[2]) == inner(b[2])
    assert by[("notch", 8, 16)][1][2] == [(2, 2), (1, 2)]                                       # a degenerate loop, emitted as it is
    hole, inside = by[("cup", 8, 4)][1:]
    assert hole[1] == 1 and inside[1] == 0 and sorted(hole[2]) == sorted(inside[2])
    # where simplify_oracle's rule kept different prong corners on the two sides
    theirs = simplify_oracle.HAND["cup-hole"][1][4]
    assert sorted(theirs[1][2]) != sorted(theirs[2][2])
    assert by[("head", 8, 16)] == by[("head", 8, 0)] and by[("head", 4, 16)][1][2] == [(1, 1), (2, 1), (2, 2), (1, 2)]
    assert [len(l[2]) for l in by[("framed-stairs", 8, 16)]] == [4, 4, 3, 3]


def test_the_parent_rule_violates_the_matching_property():
    """The check discriminates: simplify_oracle's per-loop rule leaves 7 directed segments of "stairs" at 0.5 px without their reverse."""
    plane = simplify_oracle.hand_plane("stairs")
    theirs = simplify_oracle.simplify_loops(contours_oracle.trace_plane(plane, 8), 4)
    assert len(oracle.unmatched(oracle.interior_segments(plane, theirs))) == 7
    ours = oracle.simplify_plane(plane, 8, 4)
    assert not oracle.unmatched(ours[1]) and not oracle.unmatched(oracle.interior_segments(plane, ours[0]))


def _check_invariants(plane, source, answer, tol2_q, runs):
    """source: trace_plane's loops; answer: simplify_plane's."""
    kept, segments, expanded, positions = answer
    assert not oracle.unmatched(segments)                                                       # the matching property
    got = contours_oracle.arrays(kept)
    assert got[0][0] == len(source) == len(kept) and got[0][1] <= sum(len(s[2]) for s in source) + 2 * runs
    assert np.array_equal(got[1][:, 1], np.cumsum(got[1][:, 2]) - got[1][:, 2]) and got[0][1] == got[1][:, 2].sum() == len(got[2])
    for (r, hole, pts), (kr, khole, kpts), full, where in zip(source, kept, expanded, positions):
        assert (r, hole) == (kr, khole) and len(kpts) >= 2 and kpts == [full[i] for i in where] and where == sorted(set(where))
        rest = iter(full)
        assert full[0] == tuple(pts[0]) and all(any(q == tuple(p) for q in rest) for p in pts)    # the source corners, in order, are in the expanded loop
        for i, p in enumerate(full):
            if oracle.is_junction(plane, *p):
                assert i in where                                                                # every junction passage is kept
        if tol2_q == 0:
            assert where == list(range(len(full)))                                              # tolerance 0: the expanded loop
        n = len(full)
        for a, b in zip(where, where[1:] + [where[0] + n]):
            pa, pb = full[a], full[b % n]
            len2 = (pb[0] - pa[0]) ** 2 + (pb[1] - pa[1]) ** 2
            for i in range(a + 1, b):
                p = full[i % n]
                c = abs((pb[0] - pa[0]) * (p[1] - pa[1]) - (pb[1] - pa[1]) * (p[0] - pa[0]))
                assert len2 > 0 and 16 * c * c <= tol2_q * len2, (a, i, b)                       # a dropped vertex lies within the tolerance


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", PLANES, ids=PLANE_IDS)
def test_oracle_invariants_and_simplify_shared_numpy(case, connectivity):
    """On every plane at every tolerance: the invariants of the contract hold for the oracle's answer, and
    egress.simplify_shared_numpy gives the oracle's arrays from the run code."""
    from arseg_amd import egress

    name, plane = case
    H, W = plane.shape
    source = contours_oracle.trace_plane(plane, connectivity)
    arrays = contours_oracle.arrays(source)
    row_start, runs = rle_oracle.encode(plane[None])
    for tolerance, tol2_q in TOLS:
        answer = oracle.simplify_plane(plane, connectivity, tol2_q, source)
        _check_invariants(plane, source, answer, tol2_q, len(runs[0]))
        want = contours_oracle.arrays(answer[0])
        got = egress.simplify_shared_numpy(row_start[0], runs[0], H, W, *arrays, tolerance)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (tolerance,)


def test_the_cases_are_not_trivial():
    """Junctions are inserted, long arcs lose vertices, degenerate loops occur, and a loop's first junction may lie behind position 0."""
    plane = oracle.bar_over_columns(5)
    assert oracle.simplify_plane(plane, 8, 0)[0][0][2] == [(0, 0), (5, 0), (5, 1), (4, 1), (3, 1), (2, 1), (1, 1), (0, 1)]
    down = oracle.simplify_plane(oracle.bar_over_columns(5, True), 8, 0)[0][0][2]
    assert down == [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (0, 5)]
    wave = oracle.wave_plane(40, 2)
    full, kept = oracle.simplify_plane(wave, 8, 0)[0], oracle.simplify_plane(wave, 8, 64)[0]
    assert len(full[0][2]) == 82 and 4 < len(kept[0][2]) < 82
    framed = oracle.wave_plane(9, 5, True, True)
    loops, _, expanded, _ = oracle.simplify_plane(framed, 8, 16)
    late = [full for full in expanded if not oracle.is_junction(framed, *full[0]) and any(oracle.is_junction(framed, *p) for p in full)]
    assert late and any(len(pts) == 2 for _, _, pts in oracle.simplify_plane(np.array([[0, 0, 0], [0, 1, 0]], dtype=np.uint8), 8, 16)[0])


def _frame(name="stairs"):
    plane = simplify_oracle.hand_plane(name)
    row_start, runs = rle_oracle.encode(plane[None])
    return (row_start[0], runs[0], plane.shape[0], plane.shape[1]) + tuple(contours_oracle.contour_plane(plane))


def test_simplify_shared_numpy_refusals():
    from arseg_amd import egress

    rs, runs, H, W, counts, loops, verts = _frame()
    for bad in (-1, -0.25, 0.1, 0.3, float("nan"), float("inf"), 1e9):
        with pytest.raises(ValueError):
            egress.simplify_shared_numpy(rs, runs, H, W, counts, loops, verts, bad)
    with pytest.raises(ValueError):
        egress.simplify_shared_numpy(rs, runs, H, W, np.array([2, 99], dtype=np.int32), loops, verts, 1)
    with pytest.raises(ValueError):
        egress.simplify_shared_numpy(rs, runs, H, W, np.array([-1, -1], dtype=np.int32), loops, verts, 1)
    broken = loops.copy()
    broken[1, 2] = 1000
    with pytest.raises(ValueError):
        egress.simplify_shared_numpy(rs, runs, H, W, counts, broken, verts, 1)
    with pytest.raises(ValueError):
        egress.simplify_shared_numpy(rs, runs[:-1], H, W, counts, loops, verts, 1)              # a run code that is not the frame's
    with pytest.raises(ValueError):
        egress.simplify_shared_numpy(rs, runs, H, W - 1, counts, loops, verts, 1)
    with pytest.raises(ValueError):
        egress.simplify_shared_numpy(rs, runs, 16385, W, counts, loops, verts, 1)
    for fine in (0, 0.25, 0.75, 1, 2.5, np.float32(1.5)):
        egress.simplify_shared_numpy(rs, runs, H, W, counts, loops, verts, fine)


def test_wrappers_refuse_without_a_gpu():
    from arseg_amd import _lib, egress, ops

    rs, runs = torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32)
    frames = egress.RleFrames(rs, runs, 3, 8)
    found = egress.RegionFrames(torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32),
                                torch.zeros((1, 4, 8), dtype=torch.int64), frames)
    counts, loops, verts = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 8, 4), dtype=torch.int32), torch.zeros((1, 32), dtype=torch.int32)
    held = egress.ContourFrames(counts, loops, verts, found)
    with pytest.raises(ValueError):
        egress.simplify_shared(found, 1)
    for bad in (-1, 0.1, float("nan")):
        with pytest.raises(ValueError):
            egress.simplify_shared(held, bad)
    with pytest.raises(ValueError):
        egress.simplify_shared(held, 1, vertex_capacity=-1)
    with pytest.raises(_lib.ArsegError, match="simplify_shared_numpy is the host form"):
        egress.simplify_shared(held, 1)
    with pytest.raises(ValueError):
        egress.simplify_shared(held, 1, out=held)
    plain = egress.SimplifiedContours(counts.clone(), loops.clone(), torch.zeros((1, 48), dtype=torch.int32), held, 1)
    with pytest.raises(ValueError):
        egress.simplify_shared(held, 1, out=plain)                                              # not a SharedContours
    with pytest.raises(ValueError):
        egress.SharedContours(counts, loops, verts, found, 1)
    with pytest.raises(ValueError):
        egress.SharedContours(counts, torch.zeros((1, 7, 4), dtype=torch.int32), verts, held, 1)
    done = egress.SharedContours(counts.clone(), loops.clone(), torch.zeros((1, 48), dtype=torch.int32), held, 1.5)
    assert isinstance(done, egress.SimplifiedContours) and done.contours is held and done.tolerance == 1.5 and done.source is found
    assert done.needed() is done.counts and (done.loop_capacity, done.vertex_capacity) == (8, 48)
    with pytest.raises(ValueError):
        egress.simplify_shared(egress.ContourFrames(counts, torch.zeros((1, 9, 4), dtype=torch.int32), verts, found), 1, out=done)
    # to_host: a triangle and a degenerate loop of two vertices
    done.counts[0] = torch.tensor([2, 5], dtype=torch.int32)
    done.loops[0, 0] = torch.tensor([0, 0, 3, 0], dtype=torch.int32)
    done.loops[0, 1] = torch.tensor([1, 3, 2, 0], dtype=torch.int32)
    done.verts[0, :5] = torch.tensor([0, (3 << 16) | 8, 3 << 16, (2 << 16) | 2, (2 << 16) | 1], dtype=torch.int32)
    both = done.to_host()[0]
    assert [(r, hole, pts.tolist()) for r, hole, pts in both] == [(0, 0, [[0, 0], [8, 3], [0, 3]]), (1, 0, [[2, 2], [1, 2]])]
    assert "drop_degenerate=False" in str(inspect.signature(egress.SharedContours.to_host))
    (region, hole, pts), = done.to_host(drop_degenerate=True)[0]
    assert (region, hole) == (0, 0) and pts.tolist() == [[0, 0], [8, 3], [0, 3]]
    out = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.contours_simplify_shared(rs, runs, counts, loops, verts, 3, 8, 0.3, out)
    with pytest.raises(ValueError):
        ops.contours_simplify_shared(rs, runs, counts, loops, verts, 16385, 8, 1, out)
    with pytest.raises(ValueError):
        ops.contours_simplify_shared(rs, runs, counts, loops, verts, 3, 0, 1, out)
    with pytest.raises(_lib.ArsegError):
        ops.contours_simplify_shared(rs, runs, counts, loops, verts, 3, 8, 1, out, loops.clone(), verts.clone())


def test_alter_res_batch_polygons_default_is_unchanged():
    """shared_borders is the last parameter and defaults to False: a call without it ends in egress.simplify as before."""
    from arseg_amd import egress, evaluation

    sig = inspect.signature(evaluation.alter_res_batch_polygons)
    assert list(sig.parameters)[-1] == "shared_borders" and sig.parameters["shared_borders"].default is False
    assert list(sig.parameters)[:7] == ["lr_net", "ref_ps", "imgs", "mv_qs", "capacity", "region_capacity", "tolerance"]
    seen = []
    real = evaluation.alter_res_batch_contours, egress.simplify, egress.simplify_shared
    try:
        evaluation.alter_res_batch_contours = lambda *a, **k: ("outlines", "labels")
        egress.simplify = lambda outlines, tolerance: seen.append("simplify") or ("plain", outlines, tolerance)
        egress.simplify_shared = lambda outlines, tolerance: seen.append("shared") or ("shared", outlines, tolerance)
        assert evaluation.alter_res_batch_polygons(None, [], None, None, 8, 8, 1.5) == (("plain", "outlines", 1.5), "labels")
        assert evaluation.alter_res_batch_polygons(None, [], None, None, 8, 8, 1.5, shared_borders=True) == (("shared", "outlines", 1.5), "labels")
    finally:
        evaluation.alter_res_batch_contours, egress.simplify, egress.simplify_shared = real
    assert seen == ["simplify", "shared"]


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, egress, evaluation, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arseg_hip.h")).read(), flags=re.S)
    for name in ("arseg_contours_simplify_shared_fwd", "arseg_contours_simplify_shared_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
        declared = re.search(r"%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["arseg_contours_simplify_shared_fwd"][1]) == 19
    assert len(_lib.PROTOTYPES["arseg_contours_simplify_shared_workspace_bytes"][1]) == 4
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.contours_simplify_shared) and callable(egress.simplify_shared) and callable(egress.simplify_shared_numpy)
    assert issubclass(egress.SharedContours, egress.SimplifiedContours)


def test_workspace_bytes():
    """Per frame 12 bytes per loop slot, 4 per vertex slot and 5 per slot of the expanded loops (vcap + 2 cap; the marks rounded up to 4),
    in all rounded up to 16; nothing for sizes the entry point refuses; SIZE_MAX for sizes beyond size_t."""
    from arseg_amd import _lib

    f = _lib.load().arseg_contours_simplify_shared_workspace_bytes
    frame = lambda cap, lcap, vcap: 12 * lcap + 4 * vcap + 4 * (vcap + 2 * cap) + (vcap + 2 * cap + 3) // 4 * 4
    up = lambda b: (b + 15) // 16 * 16
    for N, cap, lcap, vcap in ((1, 1, 1, 1), (1, 4, 4, 16), (3, 100, 100, 401), (2, 5, 0, 0), (11, 40000, 40000, 160000), (3, 1 << 29, 1 << 29, 1 << 31)):
        assert f(N, cap, lcap, vcap) == up(N * frame(cap, lcap, vcap)), (N, cap, lcap, vcap)
    for bad in ((0, 10, 10, 10), (-1, 10, 10, 10), (2, 0, 10, 10), (2, -1, 10, 10), (2, 10, -1, 10), (2, 10, 10, -5)):
        assert f(*bad) == 0
    for huge in ((2, 1 << 29, 1 << 60, 1 << 61), (1, 1, (1 << 63) - 1, 0), (1, 1, 0, (1 << 63) - 1), ((1 << 31) - 1, 1 << 29, 1 << 40, 1 << 40),
                 (1, (1 << 63) - 1, 0, 0)):
        assert f(*huge) == (1 << 64) - 1                                                        # does not fit size_t: no workspace is that large
    sizes = [f(2, c, c, 4 * c) for c in (1, 2, 3, 64, 65, 1000)]
    assert sizes == sorted(set(sizes)) and all(s % 16 == 0 for s in sizes)


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(0)
    at = lambda k: ctypes.c_void_p(64 * k)
    EINVAL, EWORKSPACE = _lib.ARSEG_EINVAL, _lib.ARSEG_EWORKSPACE
    N, cap, lcap, vcap = 2, 60, 50, 200
    enough = lib.arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap)
    assert enough == N * (12 * lcap + 4 * vcap + 5 * (vcap + 2 * cap))
    names = ("row_start", "runs", "cap", "counts", "loops", "lcap", "verts", "vcap", "N", "H", "W", "tol2_q", "counts_out", "loops_out", "verts_out",
             "vcap_out", "workspace", "workspace_bytes")
    good = dict(zip(names, (at(8), at(9), cap, at(1), at(2), lcap, at(3), vcap, N, 8, 24, 16, at(4), at(5), at(6), vcap + 2 * cap, at(7), enough)))

    def call(**changed):
        return lib.arseg_contours_simplify_shared_fwd(*[dict(good, **changed)[k] for k in names], null)

    for name in ("row_start", "runs", "counts", "counts_out", "loops", "loops_out", "verts", "verts_out"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer (with a positive capacity)
    for name in ("row_start", "runs", "counts", "loops", "verts", "counts_out", "loops_out", "verts_out", "workspace"):
        for address in (1025, 1026, 1027):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte aligned
    for name in ("N", "H", "W", "cap"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(lcap=-1) == EINVAL and call(vcap=-1) == EINVAL and call(vcap_out=-1) == EINVAL
    assert call(H=16385) == EINVAL and call(W=16385) == EINVAL                                  # the range of the 32-bit products
    assert call(tol2_q=-1) == EINVAL and call(tol2_q=(1 << 30) + 1) == EINVAL
    assert call(cap=(1 << 29) + 1) == EINVAL
    assert call(verts_out=good["verts"]) == EINVAL and call(loops_out=good["loops"]) == EINVAL  # in place
    assert call(counts_out=good["counts"]) == EINVAL
    for out in ("counts_out", "loops_out", "verts_out"):                                        # an output that is any of the inputs
        for src in ("row_start", "runs", "counts", "loops", "verts"):
            assert call(**{out: good[src]}) == EINVAL
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == EWORKSPACE and call(workspace_bytes=0) == EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == EWORKSPACE
    assert call(verts_out=null, vcap_out=0, workspace_bytes=0) == EWORKSPACE                    # the sizing form passes the checks
    assert call(H=16384, W=16384, tol2_q=1 << 30, workspace_bytes=0) == EWORKSPACE and call(tol2_q=0, workspace_bytes=0) == EWORKSPACE
    assert call(cap=1 << 29, workspace_bytes=0) == EWORKSPACE and call(vcap_out=1, workspace_bytes=0) == EWORKSPACE
    assert call(workspace_bytes=0, tol2_q=-1) == EINVAL and call(workspace_bytes=0, N=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    for huge in (dict(lcap=1 << 60, vcap=1 << 61), dict(lcap=(1 << 63) - 1), dict(vcap=(1 << 63) - 1), dict(N=(1 << 31) - 1, lcap=1 << 40)):
        assert call(workspace_bytes=0, **huge) == EWORKSPACE and call(workspace_bytes=(1 << 64) - 1, **huge) == EWORKSPACE      # a size beyond size_t
    assert call(loops=null, loops_out=null, lcap=0, verts=null, vcap=0, verts_out=null, vcap_out=0, workspace=null, workspace_bytes=0) == EWORKSPACE
    assert call(loops=null, loops_out=null, lcap=0, verts=null, vcap=0, verts_out=null, vcap_out=0, workspace=null, workspace_bytes=1 << 20) == EINVAL


def test_documented():
    """The header, DESIGN.md, README.md and INTEGRATION.md describe the pass; what is left out is said; the two earlier "later item"
    sentences point at the new entry."""
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    assert "smallest vertex word" in header.lower() and "Degenerate loops are emitted as they are" in header
    assert "(arseg_contours_simplify_shared_fwd, below, cuts the loops where three regions meet" in header and "is a later item" not in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.14" in design and "V′ <= V + 2·runs" in design and "drop_degenerate" in design and "is §6.14 (`egress.simplify_shared`)" in design
    assert "simplify_shared" in open(os.path.join(ROOT, "README.md")).read()
    assert "egress.simplify_shared" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
