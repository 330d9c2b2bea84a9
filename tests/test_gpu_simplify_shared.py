"""GPU checks of the outlines simplified with shared borders (csrc/simplify_shared.hip, arseg_contours_simplify_shared_fwd;
arseg_amd.egress.simplify_shared): counts, loops and kept vertices against the oracle written from the contract on the pixel plane
(tests/simplify_shared_oracle.py).  The unit tests upload the run code of rle_oracle and the outlines of contours_oracle, so they stand
on simplify_shared.hip alone; only the two chain tests at the end run the encoder, the labelling and the tracing too.  Every output is
an integer: every comparison is np.array_equal.  Nothing here provokes a fault: malformed input is exercised only through the argument
checks on the CPU (tests/test_simplify_shared.py)."""
import numpy as np
import pytest
import torch

import contours_oracle
import links_oracle
import regions_oracle
import rle_oracle
import simplify_oracle
import simplify_shared_oracle as oracle

pytestmark = pytest.mark.gpu

G32 = np.int32(oracle.GUARD_I32)
GW = np.uint32(oracle.GUARD_WORD)
EXTRA = 8
TOLS = list(oracle.TOLERANCES.items())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _guarded(dev, n, guard, dtype):
    return torch.from_numpy(np.full(n, guard, dtype=dtype)).to(dev)


_SOURCES, _ANSWERS = {}, {}


def _source(plane, connectivity):
    """contours_oracle's loops and arrays for a plane -- the input of the pass -- computed once."""
    key = (plane.shape, plane.tobytes(), connectivity)
    if key not in _SOURCES:
        loops = contours_oracle.trace_plane(plane, connectivity)
        _SOURCES[key] = (loops, contours_oracle.arrays(loops))
    return key, _SOURCES[key]


def _answer(plane, connectivity, tol2_q):
    """The oracle's answer for a plane at a tolerance, computed once."""
    key, (loops, _) = _source(plane, connectivity)
    if (key, tol2_q) not in _ANSWERS:
        _ANSWERS[(key, tol2_q)] = oracle.simplify_frame(plane, connectivity, tol2_q, loops)
    return _ANSWERS[(key, tol2_q)]


def _inputs(planes, connectivity, cap=None, lcap=None, vcap=None, refuse=None):
    """The five input arrays of N frames: the run code as arseg_labels_rle_fwd leaves it and the outlines as arseg_rle_contours_fwd
    leaves them (the capacities default to room for everything and 3 more; the slots beyond a frame's own are guard filled) ->
    ([row_start [N,H+1], runs [N,cap], counts [N,2], loops [N,lcap,4], verts [N,vcap]], processable [N]).  refuse: {frame: "negative" |
    "loops" | "verts" | "runs"} -- the frame's counts are made those of a refused source, of one that needs more loops than lcap or
    more vertices than vcap, or its row_start says that its run code overflowed."""
    planes = np.ascontiguousarray(planes)
    N = len(planes)
    sources = [_source(p, connectivity)[1][1] for p in planes]
    row_start, words = rle_oracle.encode(planes)
    cap = max(len(w) for w in words) + 3 if cap is None else cap
    lcap = max(len(s[1]) for s in sources) + 3 if lcap is None else lcap
    vcap = max(len(s[2]) for s in sources) + 3 if vcap is None else vcap
    runs = np.full((N, cap), GW, np.uint32)
    counts, loops, verts = np.zeros((N, 2), np.int32), np.full((N, lcap, 4), G32, np.int32), np.full((N, vcap), GW, np.uint32)
    ok = np.ones(N, dtype=bool)
    for n, (c, l, v) in enumerate(sources):
        runs[n, :len(words[n])] = words[n]
        counts[n] = c
        loops[n, :len(l)], verts[n, :len(v)] = l, v
    for n, how in (refuse or {}).items():
        if how == "runs":
            row_start[n, -1] = cap + 1
        else:
            counts[n] = {"negative": (-1, -1), "loops": (lcap + 1, counts[n, 1]), "verts": (counts[n, 0], vcap + 1)}[how]
        ok[n] = False
    return [row_start, runs, counts, loops, verts], ok


def _upload(dev, arrays):
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in arrays]


def _run(dev, planes, tolerance, connectivity=8, vcap_out=None, workspace=None, **how):
    """_inputs uploaded, ops.contours_simplify_shared into guard filled buffers with EXTRA guard words behind them -> the numpy copies
    (counts [N,2], loops [N,lcap,4], verts [N,vcap_out]) after checking them against the oracle frame by frame (oracle.expected: a
    refused frame fully intact but for its counts, counts and the loop rows exact, the words below vcap_out exact and the rest intact),
    the guards behind every buffer and the inputs intact.  vcap_out defaults to vcap + 2 cap; 0: the sizing form."""
    from arseg_amd import ops

    planes = np.ascontiguousarray(planes)
    N, H, W = planes.shape
    tol2_q = oracle.TOLERANCES[tolerance]
    host, ok = _inputs(planes, connectivity, **how)
    cap, lcap, vcap = host[1].shape[1], host[3].shape[1], host[4].shape[1]
    vcap_out = vcap + 2 * cap if vcap_out is None else vcap_out
    inputs = _upload(dev, host)
    counts_back = _guarded(dev, 2 * N + EXTRA, G32, np.int32)
    loops_back = _guarded(dev, 4 * N * lcap + EXTRA, G32, np.int32)
    verts_back = _guarded(dev, N * vcap_out + EXTRA, GW.view(np.int32), np.int32)
    ops.contours_simplify_shared(*inputs, H, W, tolerance, counts_back[:2 * N].view(N, 2), loops_back[:4 * N * lcap].view(N, lcap, 4),
                                 verts_back[:N * vcap_out].view(N, vcap_out) if vcap_out else None, workspace=workspace)
    counts_got, loops_got = counts_back.cpu().numpy(), loops_back.cpu().numpy()
    verts_got = verts_back.cpu().numpy().view(np.uint32)
    assert (counts_got[2 * N:] == G32).all() and (loops_got[4 * N * lcap:] == G32).all() and (verts_got[N * vcap_out:] == GW).all()
    for before, after in zip(host, inputs):
        assert np.array_equal(after.cpu().numpy().view(before.dtype), before)
    counts_got, loops_got, verts_got = counts_got[:2 * N].reshape(N, 2), loops_got[:4 * N * lcap].reshape(N, lcap, 4), verts_got[:N * vcap_out].reshape(N, vcap_out)
    for n in range(N):
        want = oracle.expected(_answer(planes[n], connectivity, tol2_q), ok[n], vcap_out, np.full(2, G32), np.full((lcap, 4), G32), np.full(vcap_out, GW))
        assert np.array_equal(counts_got[n], want[0]), (n, counts_got[n], want[0])
        assert np.array_equal(loops_got[n], want[1]), n
        assert np.array_equal(verts_got[n], want[2]), n
    return counts_got, loops_got, verts_got


def _expanded_counts(plane, connectivity=8):
    """The vertices of the frame's expanded loops: the kept counts at tolerance 0."""
    return _answer(plane, connectivity, 0)[1][:, 2].tolist()


@pytest.mark.parametrize("case", oracle.HAND, ids=oracle.HAND_IDS)
def test_hand_made_literals(dev, case):
    """The kept loops written out by hand, at the connectivity and tolerance they are written for."""
    _, rows, connectivity, tol2_q, loops = case
    tolerance = {q: t for t, q in TOLS}[tol2_q]
    counts, rec, verts = _run(dev, np.array(rows, dtype=np.uint8)[None], tolerance, connectivity)
    want = contours_oracle.arrays(loops)
    L, V = want[0]
    assert counts[0].tolist() == [L, V] and np.array_equal(rec[0, :L], want[1]) and np.array_equal(verts[0, :V], want[2])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_hand_made_planes(dev, connectivity):
    """The hand planes of both oracles at all six tolerances."""
    planes = [simplify_oracle.hand_plane(name) for name in simplify_oracle.HAND_IDS] + [np.array(h[1], dtype=np.uint8) for h in oracle.HAND]
    seen = set()
    for plane in planes:
        if plane.tobytes() + bytes(plane.shape) not in seen:
            seen.add(plane.tobytes() + bytes(plane.shape))
            for tolerance, _ in TOLS:
                _run(dev, plane[None], tolerance, connectivity)


@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("columns", [5, 9, 10, 64, 65, 66, 131])
def test_junctions_inside_one_edge(dev, columns, vertical):
    """A bar over single-pixel columns of alternating value: 4, 8 and 9 (what a lane takes on its own and the first edge the wave takes),
    63 / 64 / 65 and 130 T-junctions inside the bar's long edge -- along a row (two searches, a run each) and down a column (a lane per
    row, strided)."""
    plane = oracle.bar_over_columns(columns, vertical)
    assert _source(plane, 8)[1][1][1][0, 2] == 4 and _expanded_counts(plane)[0] == 4 + columns - 1
    for tolerance in (0.0, 1.0, 256.0):
        counts, _, _ = _run(dev, plane[None], tolerance)
        assert counts[0, 1] == 5 * columns + 3                                               # nothing can go: every vertex is a junction


@pytest.mark.parametrize("width,split", [(30, False), (31, False), (32, False), (21, True), (126, False), (127, False), (128, False), (85, True)])
def test_loops_around_the_wave_and_workgroup_strides(dev, width, split):
    """Expanded loops of 62 / 64 / 66 and 254 / 256 / 258 vertices (64 and 256 with inserted junctions too): one stride of a wave's 64
    lanes, one pass of the 256-wide scans."""
    plane = oracle.wave_plane(width, 11 + width, split)
    assert _expanded_counts(plane)[0] == (3 * width + 1 if split else 2 * width + 2)
    for tolerance, _ in TOLS:
        _run(dev, plane[None], tolerance)


@pytest.mark.parametrize("width,split,framed", [(1022, False, False), (1023, False, False), (1024, False, False), (682, True, False),
                                                (683, True, False), (1100, False, True)])
def test_loops_around_the_length_a_wave_stages(dev, width, split, framed):
    """Expanded loops of 2046 / 2048 / 2050 vertices, and of 2047 / 2050 with a third of them inserted junctions -- at most 2048 are
    walked in the wave's LDS stage, longer ones in place --, and one of 2202 whose first junction passage is position 2 (it starts at a
    plain corner inside a frame region)."""
    plane = oracle.wave_plane(width, 40 + width, split, framed)
    expanded = _expanded_counts(plane)
    assert (3 * width + 1 if split else 2 * width + 2) in expanded
    if framed:
        loops, _, full, kept = oracle.simplify_plane(plane, 8, 0)
        at = expanded.index(2 * width + 2)
        assert [oracle.is_junction(plane, *p) for p in full[at][:3]] == [False, False, True]
    for tolerance in (0.0, 0.5, 1.0, 2.0):
        _run(dev, plane[None], tolerance)


@pytest.mark.parametrize("count", [255, 256, 257])
def test_loop_counts_around_a_workgroup(dev, count):
    """A frame of exactly 255, 256 and 257 loops: the scans' carry and the last workgroups of the launches that give a wave a loop."""
    plane = regions_oracle.REGION_COUNT_PLANES[count]
    for tolerance in (0.0, 1.0, 256.0):
        counts, _, _ = _run(dev, plane, tolerance, 4)
        assert counts[0, 0] == count


@pytest.mark.parametrize("name", list(contours_oracle.LONG))
def test_long_loops(dev, name):
    """The spirals and the comb at both connectivities and all six tolerances."""
    plane = np.ascontiguousarray(contours_oracle.LONG[name])[None]
    for connectivity in (4, 8):
        for tolerance, _ in TOLS:
            _run(dev, plane, tolerance, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_seeded_planes_and_unlike_frames(dev, connectivity):
    """The seeded noise and the dense noise at all six tolerances, and N = 2 with frames of different sizes of problem in both orders: a
    frame's result is the one it has alone."""
    for tolerance, _ in TOLS:
        _run(dev, regions_oracle.noise_planes(*regions_oracle.NOISE), tolerance, connectivity)
        _run(dev, regions_oracle.dense_noise(*links_oracle.DENSE), tolerance, connectivity)
    a, b = np.zeros((1, 21, 21), np.uint8), np.zeros((1, 21, 21), np.uint8)
    a[0] = regions_oracle.HAND["spiral-21x21"][0]
    b[0, :6, :6] = regions_oracle.HAND["checkerboard-6x6"][0]
    for pair in (np.concatenate([a, b]), np.concatenate([b, a])):
        for tolerance in (0.5, 1.0):
            got = _run(dev, pair, tolerance, connectivity)
            host, _ = _inputs(pair, connectivity)
            for n in range(2):
                alone = _run(dev, pair[n:n + 1], tolerance, connectivity, cap=host[1].shape[1], lcap=host[3].shape[1], vcap=host[4].shape[1])
                assert all(np.array_equal(g[n], s[0]) for g, s in zip(got, alone))


@pytest.mark.parametrize("how", ["negative", "loops", "verts", "runs"])
def test_refused_frames(dev, how):
    """A frame whose source was refused (counts -1), one that needs more loops than lcap, one that needs more vertices than vcap and one
    whose run code overflowed: counts_out = {-1, -1} and every other buffer of that frame intact, the other frames of the call exact
    (_run checks both through oracle.expected)."""
    planes = rle_oracle.build(rle_oracle.CASES[0])
    assert len(planes) >= 2
    for n in range(len(planes)):
        counts, _, _ = _run(dev, planes, 1.0, refuse={n: how})
        assert counts[n].tolist() == [-1, -1] and all(counts[k, 0] > 0 for k in range(len(planes)) if k != n)


def test_output_capacity_and_sizing(dev):
    """vcap_out equal to, and one below, what the frame with the largest need asks for; far below; and the sizing form (no verts_out):
    counts stay exact, first' too.  At tolerance 0 the need is above the source's V."""
    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    for tolerance in (0.0, 1.0):
        needs = np.stack([_answer(p, 8, oracle.TOLERANCES[tolerance])[0] for p in planes])
        V = int(needs[:, 1].max())
        assert needs[:, 1].min() < V
        assert tolerance > 0 or V > max(len(_source(p, 8)[1][1][2]) for p in planes)
        for vcap_out in (V, V - 1, 1, 0):
            counts, _, _ = _run(dev, planes, tolerance, vcap_out=vcap_out)
            assert np.array_equal(counts, needs)


def test_own_workspace_and_bit_equality(dev):
    """Two runs of the same call are bit-equal; a caller's workspace of exactly the size asked for serves, with guards behind it; one byte
    less is refused."""
    from arseg_amd import _lib

    planes = np.concatenate([regions_oracle.noise_planes(*regions_oracle.NOISE), regions_oracle.dense_noise(9, 1, 12, 65)])
    first = _run(dev, planes, 1.0)
    host, _ = _inputs(planes, 8)
    N, cap, lcap, vcap = planes.shape[0], host[1].shape[1], host[3].shape[1], host[4].shape[1]
    nbytes = _lib.load().arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap)
    ecap = vcap + 2 * cap
    assert nbytes == (N * (12 * lcap + 4 * vcap + 4 * ecap + (ecap + 3) // 4 * 4) + 15) // 16 * 16
    ws_back = torch.full((nbytes + 4 * EXTRA,), 0x5A, dtype=torch.uint8, device=dev)
    second = _run(dev, planes, 1.0, workspace=ws_back[:nbytes])
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert (ws_back[nbytes:].cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.ArsegError):
        _run(dev, planes, 1.0, workspace=ws_back[:nbytes - 1])


def test_one_graph_replayed_on_refilled_inputs(dev):
    """ops.contours_simplify_shared captured once (every buffer given: nothing is allocated); the inputs are refilled in place with
    another frame's arrays; each replay equals the oracle for its own input."""
    from arseg_amd import _lib, ops

    frames = [regions_oracle.noise_planes(s, 1, 12, 65) for s in (31, 32)]
    N, H, W, cap, lcap, vcap = 1, 12, 65, 400, 400, 1600
    sides = [_inputs(f, 8, cap, lcap, vcap)[0] for f in frames]
    inputs = _upload(dev, sides[0])
    counts = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    loops, verts = torch.zeros((N, lcap, 4), dtype=torch.int32, device=dev), torch.zeros((N, vcap + 2 * cap), dtype=torch.int32, device=dev)
    ws = torch.zeros((_lib.load().arseg_contours_simplify_shared_workspace_bytes(N, cap, lcap, vcap) // 4,), dtype=torch.int32, device=dev)

    def call():
        ops.contours_simplify_shared(*inputs, H, W, 1.0, counts, loops, verts, workspace=ws)

    call()                                                                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    seen = []
    for side, plane in ((sides[1], frames[1]), (sides[0], frames[0])):
        for t, a in zip(inputs, _upload(dev, side)):
            t.copy_(a)
        for t in (counts, loops, verts):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        want = _answer(plane[0], 8, 16)
        L, V = want[0]
        assert np.array_equal(counts[0].cpu().numpy(), want[0])
        assert np.array_equal(loops[0, :L].cpu().numpy(), want[1]) and (loops[0, L:] == -7).all()
        assert np.array_equal(verts[0, :V].cpu().numpy().view(np.uint32), want[2]) and (verts[0, V:] == -7).all()
        seen.append(int(V))
    assert seen[0] != seen[1]


def _contour_frames(dev, planes, connectivity=8):
    """egress.ContourFrames holding contours_oracle's arrays over the run code of rle_oracle (the regions behind them are placeholders
    of the right N)."""
    from arseg_amd import egress

    N, H, W = planes.shape
    (rs, runs, counts, loops, verts), _ = _inputs(planes, connectivity)
    rs, runs, counts, loops, verts = _upload(dev, [rs, runs, counts, loops, verts])
    found = egress.RegionFrames(torch.zeros((N,), dtype=torch.int32, device=dev), torch.zeros((N, runs.shape[1]), dtype=torch.int32, device=dev),
                                torch.zeros((N, 1, 8), dtype=torch.int64, device=dev), egress.RleFrames(rs, runs, H, W), connectivity)
    return egress.ContourFrames(counts, loops, verts, found)


def test_egress_simplify_shared_with_and_without_out(dev):
    """egress.simplify_shared on ContourFrames built from the oracles' arrays: the host polygons equal the oracle's; with ``out`` the
    same buffers are written again; an overflowed frame is named by to_host; drop_degenerate leaves out the loops without area."""
    from arseg_amd import _lib, egress

    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    N = planes.shape[0]
    held = {c: _contour_frames(dev, planes, c) for c in (4, 8)}
    first = egress.simplify_shared(held[4], 1.5)
    assert isinstance(first, egress.SharedContours) and first.contours is held[4] and first.tolerance == 1.5 and first.source is held[4].source
    assert (first.loop_capacity, first.vertex_capacity) == (held[4].loop_capacity, held[4].vertex_capacity + 2 * held[4].source.frames.capacity)
    lcap8 = held[8].loop_capacity
    other = egress.SharedContours(torch.empty((N, 2), dtype=torch.int32, device=dev), torch.empty((N, lcap8, 4), dtype=torch.int32, device=dev),
                                  torch.empty((N, first.vertex_capacity), dtype=torch.int32, device=dev), held[8], 0)
    again = egress.simplify_shared(held[8], 1.0, out=other)
    assert again is other and again.contours is held[8] and again.tolerance == 1.0
    degenerate = 0
    for connectivity, tolerance, got in ((8, 1.0, again), (4, 1.5, first), (4, 0.0, egress.simplify_shared(held[4], 0))):
        host, proper = got.to_host(), got.to_host(drop_degenerate=True)
        for n in range(N):
            want = contours_oracle.polygons(_answer(planes[n], connectivity, oracle.TOLERANCES[tolerance]))
            assert len(host[n]) == len(want) == int(got.needed()[n, 0])
            for (r, hole, pts), (wr, whole, wpts) in zip(host[n], want):
                assert (r, hole) == (wr, whole) and pts.dtype == np.int32 and np.array_equal(pts, wpts)
            with_area = [(r, hole, pts) for r, hole, pts in want if contours_oracle.shoelace2(pts) != 0]
            degenerate += len(want) - len(with_area)
            assert len(proper[n]) == len(with_area) and all(np.array_equal(p[2], w[2]) for p, w in zip(proper[n], with_area))
    assert degenerate > 0
    with pytest.raises(_lib.ArsegError, match="frame 0 needs .* vertices, the capacities are"):
        egress.simplify_shared(held[8], 1.0, vertex_capacity=4).to_host()


def test_real_chain_on_a_blob_plane(dev):
    """ops.labels_rle -> ops.rle_regions -> egress.contours -> egress.simplify_shared -> to_host() on a 64x65 blob plane: the polygons
    are simplify_shared_numpy's on the run code and the outlines brought to the host, and the oracle's; no segment is left without its
    reverse in the neighbour's loop."""
    from arseg_amd import egress

    planes = rle_oracle.blob_planes(5, 1, 64, 65, n_cls=7, cell=8)
    N, H, W = planes.shape
    frames = egress.rle_of_planes(torch.from_numpy(planes).to(dev), H * W)
    outlines = egress.contours(egress.regions(frames, 1024))
    traced = contours_oracle.trace_plane(planes[0])
    source = contours_oracle.arrays(traced)
    L, V = source[0]
    assert np.array_equal(outlines.counts[0].cpu().numpy(), source[0]) and np.array_equal(outlines.verts[0, :V].cpu().numpy().view(np.uint32), source[2])
    row_start, runs = frames.to_host()[0]
    for tolerance in (0.5, 1.0, 2.0):
        got = egress.simplify_shared(outlines, tolerance)
        counts, loops, verts = egress.simplify_shared_numpy(row_start, runs, H, W, source[0], outlines.loops[0, :L].cpu().numpy(),
                                                            outlines.verts[0, :V].cpu().numpy(), tolerance)
        kept, segments, _, _ = oracle.simplify_plane(planes[0], 8, oracle.TOLERANCES[tolerance], traced)
        want = contours_oracle.arrays(kept)
        assert np.array_equal(counts, want[0]) and np.array_equal(loops, want[1]) and np.array_equal(verts, want[2]) and not oracle.unmatched(segments)
        host = got.to_host()[0]
        assert len(host) == counts[0] > 8 and np.array_equal(got.counts[0].cpu().numpy(), counts)
        for (r, hole, pts), (wr, whole, wpts) in zip(host, contours_oracle.polygons(want)):
            assert (r, hole) == (wr, whole) and np.array_equal(pts, wpts)


def test_alter_res_batch_polygons_with_shared_borders(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_polygons(shared_borders=True) gives simplify_shared_numpy's
    polygons on the run code and the outlines of the same call, with and without min_area; the default is egress.simplify's result."""
    import test_gpu_ingest_formats as tf
    from arseg_amd import egress, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop, min_area, tolerance = 64, 96, 4, 12, 1.0
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"][1:gop]).to(dev)
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * (gop - 1)
        polygons, labels = ev.alter_res_batch_polygons(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, tolerance, shared_borders=True)
        cleaned, _ = ev.alter_res_batch_polygons(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, tolerance, min_area=min_area, shared_borders=True)
        plain, _ = ev.alter_res_batch_polygons(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, tolerance)
    assert isinstance(polygons, egress.SharedContours) and isinstance(cleaned.source.frames, egress.AbsorbedFrames)
    assert type(plain) is egress.SimplifiedContours and torch.equal(plain.counts, egress.simplify(polygons.contours, tolerance).counts)
    for which in (polygons, cleaned):
        host = which.to_host()
        before = which.contours
        need = before.counts.cpu().numpy()
        codes = which.source.frames.to_host()
        for n in range(gop - 1):
            L, V = need[n]
            counts, loops, verts = egress.simplify_shared_numpy(*codes[n], H, W, need[n], before.loops[n, :L].cpu().numpy(),
                                                                before.verts[n, :V].cpu().numpy(), tolerance)
            assert np.array_equal(which.counts[n].cpu().numpy(), counts) and len(host[n]) == counts[0]
            for (r, hole, pts), (wr, whole, wpts) in zip(host[n], contours_oracle.polygons((counts, loops, verts))):
                assert (r, hole) == (wr, whole) and np.array_equal(pts, wpts)
    print(f"\nvertices per frame {polygons.contours.counts[:, 1].cpu().tolist()} -> {polygons.counts[:, 1].cpu().tolist()} at {tolerance} px "
          f"with shared borders, {plain.counts[:, 1].cpu().tolist()} without")
