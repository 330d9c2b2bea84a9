"""GPU checks of the simplified outlines (csrc/simplify.hip, arseg_contours_simplify_fwd; arseg_amd.egress.simplify): counts, loops and
kept vertices against the oracle written from the contract as the plain recursion (tests/simplify_oracle.py).  The unit tests upload
counts, loops and vertices made by contours_oracle, so they stand on simplify.hip alone; only the two chain tests at the end run the
encoder, the labelling and the tracing too.  Every output is an integer: every comparison is np.array_equal.  Nothing here provokes a
fault: malformed input is exercised only through the argument checks on the CPU (tests/test_simplify.py)."""
import numpy as np
import pytest
import torch

import contours_oracle
import links_oracle
import regions_oracle
import rle_oracle
import simplify_oracle as oracle

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
    """contours_oracle's answer for a plane -- the input of the pass -- computed once."""
    key = (plane.shape, plane.tobytes(), connectivity)
    if key not in _SOURCES:
        _SOURCES[key] = contours_oracle.contour_plane(plane, connectivity)
    return key, _SOURCES[key]


def _answer(plane, connectivity, tol2_q):
    """The oracle's answer for a plane at a tolerance, computed once."""
    key, source = _source(plane, connectivity)
    if (key, tol2_q) not in _ANSWERS:
        _ANSWERS[(key, tol2_q)] = oracle.simplify_frame(source, tol2_q)
    return _ANSWERS[(key, tol2_q)]


def _inputs(sources, lcap=None, vcap=None, refuse=None):
    """The three input arrays of N frames as arseg_rle_contours_fwd leaves them, from each frame's (counts, loops, verts) (lcap / vcap
    default: room for everything and 3 more; the slots beyond a frame's own are guard filled) -> (counts [N,2], loops [N,lcap,4], verts
    [N,vcap], processable [N]).  refuse: {frame: "negative" | "loops" | "verts"} -- the frame's counts are made those of a refused
    source, of one that needs more loops than lcap or more vertices than vcap."""
    N = len(sources)
    lcap = max(len(s[1]) for s in sources) + 3 if lcap is None else lcap
    vcap = max(len(s[2]) for s in sources) + 3 if vcap is None else vcap
    counts, loops, verts = np.zeros((N, 2), np.int32), np.full((N, lcap, 4), G32, np.int32), np.full((N, vcap), GW, np.uint32)
    ok = np.ones(N, dtype=bool)
    for n, (c, l, v) in enumerate(sources):
        counts[n] = c
        loops[n, :len(l)], verts[n, :len(v)] = l, v
    for n, how in (refuse or {}).items():
        counts[n] = {"negative": (-1, -1), "loops": (lcap + 1, counts[n, 1]), "verts": (counts[n, 0], vcap + 1)}[how]
        ok[n] = False
    return counts, loops, verts, ok


def _run(dev, planes, tolerance, connectivity=8, **how):
    """_run_frames on the outlines of planes: the inputs by contours_oracle, the answers by the oracle (each computed once)."""
    planes = np.ascontiguousarray(planes)
    tol2_q = oracle.TOLERANCES[tolerance]
    return _run_frames(dev, [_source(p, connectivity)[1] for p in planes], [_answer(p, connectivity, tol2_q) for p in planes], planes.shape[1],
                       planes.shape[2], tolerance, **how)


def _run_frames(dev, sources, answers, H, W, tolerance, lcap=None, vcap=None, vcap_out=None, refuse=None, workspace=None):
    """_inputs uploaded, ops.contours_simplify into guard filled buffers with EXTRA guard words behind them -> the numpy copies (counts
    [N,2], loops [N,lcap,4], verts [N,vcap_out]) after checking them against the answers frame by frame (oracle.expected: a refused frame
    fully intact but for its counts, counts and the loop rows exact, the words below vcap_out exact and the rest intact), the guards
    behind every buffer and the inputs intact.  vcap_out defaults to vcap; 0: the sizing form."""
    from arseg_amd import ops

    N = len(sources)
    counts, loops, verts, ok = _inputs(sources, lcap, vcap, refuse)
    lcap, vcap = loops.shape[1], verts.shape[1]
    vcap_out = vcap if vcap_out is None else vcap_out
    host = [counts, loops, verts]
    inputs = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in host]
    counts_back = _guarded(dev, 2 * N + EXTRA, G32, np.int32)
    loops_back = _guarded(dev, 4 * N * lcap + EXTRA, G32, np.int32)
    verts_back = _guarded(dev, N * vcap_out + EXTRA, GW.view(np.int32), np.int32)
    ops.contours_simplify(*inputs, H, W, tolerance, counts_back[:2 * N].view(N, 2), loops_back[:4 * N * lcap].view(N, lcap, 4),
                          verts_back[:N * vcap_out].view(N, vcap_out) if vcap_out else None, workspace=workspace)
    counts_got, loops_got = counts_back.cpu().numpy(), loops_back.cpu().numpy()
    verts_got = verts_back.cpu().numpy().view(np.uint32)
    assert (counts_got[2 * N:] == G32).all() and (loops_got[4 * N * lcap:] == G32).all() and (verts_got[N * vcap_out:] == GW).all()
    for before, after in zip(host, inputs):
        assert np.array_equal(after.cpu().numpy().view(before.dtype), before)
    counts_got, loops_got, verts_got = counts_got[:2 * N].reshape(N, 2), loops_got[:4 * N * lcap].reshape(N, lcap, 4), verts_got[:N * vcap_out].reshape(N, vcap_out)
    for n in range(N):
        want = oracle.expected(answers[n], ok[n], vcap_out, np.full(2, G32), np.full((lcap, 4), G32), np.full(vcap_out, GW))
        assert np.array_equal(counts_got[n], want[0]), (n, counts_got[n], want[0])
        assert np.array_equal(loops_got[n], want[1]), n
        assert np.array_equal(verts_got[n], want[2]), n
    return counts_got, loops_got, verts_got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_hand_made_planes(dev, name, connectivity):
    """Against the oracle, and against the kept vertices written out by hand, at all six tolerances."""
    for tolerance, tol2_q in TOLS:
        counts, loops, verts = _run(dev, oracle.hand_plane(name)[None], tolerance, connectivity)
        want = contours_oracle.arrays(oracle.HAND[name][1][tol2_q])
        L, V = want[0]
        assert counts[0].tolist() == [L, V] and np.array_equal(loops[0, :L], want[1]) and np.array_equal(verts[0, :V], want[2])


@pytest.mark.parametrize("steps", [30, 31, 32, 62, 63, 64, 126, 127, 128])
def test_staircases_around_the_wave_strides(dev, steps):
    """Staircase loops of 62 / 64 / 66 and 126 / 128 / 130 vertices (and their neighbours' of two fewer) -- one and two strides of a
    wave's 64 lanes -- and of 254 / 256 / 258 -- one pass of the 256-wide scans -- at all six tolerances."""
    plane = oracle.staircase(steps)[None]
    assert _source(plane[0], 8)[1][1][:, 2].tolist() == [2 * steps + 2, 2 * steps]
    for tolerance, _ in TOLS:
        counts, _, _ = _run(dev, plane, tolerance)
        if tolerance in (1.0, 1.5, 2.0):
            assert counts[0].tolist() == [2, 6]                                                  # two triangles


@pytest.mark.parametrize("vertices", [2046, 2048, 2050, 4100])
def test_loops_around_the_length_a_wave_stages(dev, vertices):
    """Loops of 2046 / 2048 / 2050 vertices -- at most 2048 are walked in the wave's LDS stage, longer ones in place -- and one of twice
    that, each with a short loop before and behind it in its frame, and both kinds in one call.  The loops are uneven staircases written
    down as vertices (tracing a plane of that size would take the oracle long); the pass only sees loops."""
    frames = [oracle.stair_frame(vertices, 40 + vertices), oracle.stair_frame(300, 7)]
    side = max(f[1] for f in frames)
    for tolerance in (0.0, 0.5, 1.0, 2.0):
        tol2_q = oracle.TOLERANCES[tolerance]
        counts, _, _ = _run_frames(dev, [f[0] for f in frames], [oracle.simplify_frame(f[0], tol2_q) for f in frames], side, side, tolerance)
        assert counts[:, 0].tolist() == [3, 3] and (tolerance == 0.0) == (counts[0, 1] == 4 + vertices + 8) and counts[0, 1] <= 4 + vertices + 8


@pytest.mark.parametrize("count", [255, 256, 257])
def test_loop_counts_around_a_workgroup(dev, count):
    """A frame of exactly 255, 256 and 257 loops: the scan's carry and the last workgroups of the keep and emit launches."""
    plane = regions_oracle.REGION_COUNT_PLANES[count]
    for tolerance in (0.0, 1.0, 256.0):
        counts, _, _ = _run(dev, plane, tolerance, 4)
        assert counts[0].tolist() == [count, 4 * count]                                          # every loop a rectangle: rule 3 or its corners


@pytest.mark.parametrize("name", list(contours_oracle.LONG))
def test_long_loops(dev, name):
    """The spirals and the comb -- loops of 44, 68 and 164 vertices that wind and fold back -- at both connectivities and all six
    tolerances."""
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
            for n in range(2):
                alone = _run(dev, pair[n:n + 1], tolerance, connectivity, lcap=got[1].shape[1], vcap=got[2].shape[1])
                assert all(np.array_equal(g[n], s[0]) for g, s in zip(got, alone))


@pytest.mark.parametrize("how", ["negative", "loops", "verts"])
def test_refused_frames(dev, how):
    """A frame whose source was refused (counts -1), one that needs more loops than lcap and one that needs more vertices than vcap:
    counts_out = {-1, -1} and every other buffer of that frame intact, the other frames of the call exact (_run checks both through
    oracle.expected)."""
    planes = rle_oracle.build(rle_oracle.CASES[1])
    assert len(planes) >= 2
    for n in range(len(planes)):
        counts, _, _ = _run(dev, planes, 1.0, refuse={n: how})
        assert counts[n].tolist() == [-1, -1] and all(counts[k, 0] > 0 for k in range(len(planes)) if k != n)


def test_output_capacity_and_sizing(dev):
    """vcap_out equal to, and one below, what the frame with the largest need asks for; far below; and the sizing form (no verts_out):
    counts stay exact, first' too."""
    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    needs = np.stack([_answer(p, 8, 16)[0] for p in planes])
    V = int(needs[:, 1].max())
    assert needs[:, 1].min() < V < max(len(_source(p, 8)[1][2]) for p in planes)                 # the other frame still fits; something is dropped
    for vcap_out in (V, V - 1, 1, 0):
        counts, _, _ = _run(dev, planes, 1.0, vcap_out=vcap_out)
        assert np.array_equal(counts, needs)


def test_own_workspace_and_bit_equality(dev):
    """Two runs of the same call are bit-equal; a caller's workspace of exactly the size asked for serves, with guards behind it; one byte
    less is refused."""
    from arseg_amd import _lib

    planes = np.concatenate([regions_oracle.noise_planes(*regions_oracle.NOISE), regions_oracle.dense_noise(9, 1, 12, 65)])
    first = _run(dev, planes, 1.0)
    N, lcap, vcap = planes.shape[0], first[1].shape[1], first[2].shape[1]
    nbytes = _lib.load().arseg_contours_simplify_workspace_bytes(N, lcap, vcap)
    assert nbytes == (N * (4 * lcap + (vcap + 3) // 4 * 4) + 15) // 16 * 16
    ws_back = torch.full((nbytes + 4 * EXTRA,), 0x5A, dtype=torch.uint8, device=dev)
    second = _run(dev, planes, 1.0, workspace=ws_back[:nbytes])
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert (ws_back[nbytes:].cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.ArsegError):
        _run(dev, planes, 1.0, workspace=ws_back[:nbytes - 1])


def test_one_graph_replayed_on_refilled_inputs(dev):
    """ops.contours_simplify captured once (every buffer given: nothing is allocated); the inputs are refilled in place with another
    frame's arrays; each replay equals the oracle for its own input."""
    from arseg_amd import _lib, ops

    frames = [regions_oracle.noise_planes(s, 1, 12, 65) for s in (31, 32)]
    N, H, W, lcap, vcap = 1, 12, 65, 400, 1600
    sides = [_inputs([_source(f[0], 8)[1]], lcap, vcap)[:3] for f in frames]
    upload = lambda side: [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in side]
    inputs = upload(sides[0])
    counts = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    loops, verts = torch.zeros((N, lcap, 4), dtype=torch.int32, device=dev), torch.zeros((N, vcap), dtype=torch.int32, device=dev)
    ws = torch.zeros((_lib.load().arseg_contours_simplify_workspace_bytes(N, lcap, vcap) // 4,), dtype=torch.int32, device=dev)

    def call():
        ops.contours_simplify(*inputs, H, W, 1.0, counts, loops, verts, workspace=ws)

    call()                                                                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    seen = []
    for side, plane in ((sides[1], frames[1]), (sides[0], frames[0])):
        for t, a in zip(inputs, upload(side)):
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
    """egress.ContourFrames holding contours_oracle's arrays (the run code and the regions behind them are placeholders of the right N)."""
    from arseg_amd import egress

    N, H, W = planes.shape
    counts, loops, verts, _ = _inputs([_source(p, connectivity)[1] for p in planes])
    rs, runs = torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.zeros((N, 8), dtype=torch.int32, device=dev)
    found = egress.RegionFrames(torch.zeros((N,), dtype=torch.int32, device=dev), torch.zeros((N, 8), dtype=torch.int32, device=dev),
                                torch.zeros((N, 1, 8), dtype=torch.int64, device=dev), egress.RleFrames(rs, runs, H, W), connectivity)
    return egress.ContourFrames(torch.from_numpy(counts).to(dev), torch.from_numpy(loops).to(dev), torch.from_numpy(verts.view(np.int32)).to(dev), found)


def test_egress_simplify_with_and_without_out(dev):
    """egress.simplify on ContourFrames built from the oracle's arrays: the host polygons equal the oracle's; with ``out`` the same
    buffers are written again; an overflowed frame is named by to_host."""
    from arseg_amd import _lib, egress

    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    N = planes.shape[0]
    held = {c: _contour_frames(dev, planes, c) for c in (4, 8)}
    first = egress.simplify(held[4], 1.5)
    assert isinstance(first, egress.SimplifiedContours) and first.contours is held[4] and first.tolerance == 1.5
    assert first.source is held[4].source and (first.loop_capacity, first.vertex_capacity) == (held[4].loop_capacity, held[4].vertex_capacity)
    lcap8 = held[8].loop_capacity
    other = egress.SimplifiedContours(torch.empty((N, 2), dtype=torch.int32, device=dev), torch.empty((N, lcap8, 4), dtype=torch.int32, device=dev),
                                      torch.empty((N, held[8].vertex_capacity), dtype=torch.int32, device=dev), held[8], 0)
    again = egress.simplify(held[8], 1.0, out=other)
    assert again is other and again.contours is held[8] and again.tolerance == 1.0
    for connectivity, tolerance, got in ((8, 1.0, again), (4, 1.5, first), (4, 0.0, egress.simplify(held[4], 0))):
        host = got.to_host()
        for n in range(N):
            want = contours_oracle.polygons(_answer(planes[n], connectivity, oracle.TOLERANCES[tolerance]))
            assert len(host[n]) == len(want) == int(got.needed()[n, 0])
            for (r, hole, pts), (wr, whole, wpts) in zip(host[n], want):
                assert (r, hole) == (wr, whole) and pts.dtype == np.int32 and np.array_equal(pts, wpts)
    with pytest.raises(_lib.ArsegError, match="frame 0 needs .* vertices, the capacities are"):
        egress.simplify(held[8], 1.0, vertex_capacity=4).to_host()


def test_real_chain_on_a_blob_plane(dev):
    """ops.labels_rle -> ops.rle_regions -> egress.contours -> egress.simplify -> to_host() on a 64x65 blob plane: the polygons are
    simplify_numpy's on the outlines brought to the host, and the oracle's."""
    from arseg_amd import egress

    planes = rle_oracle.blob_planes(5, 1, 64, 65, n_cls=7, cell=8)
    N, H, W = planes.shape
    frames = egress.rle_of_planes(torch.from_numpy(planes).to(dev), H * W)
    outlines = egress.contours(egress.regions(frames, 1024))
    source = contours_oracle.contour_plane(planes[0])
    L, V = source[0]
    assert np.array_equal(outlines.counts[0].cpu().numpy(), source[0]) and np.array_equal(outlines.verts[0, :V].cpu().numpy().view(np.uint32), source[2])
    for tolerance in (0.5, 1.0, 2.0):
        got = egress.simplify(outlines, tolerance)
        counts, loops, verts = egress.simplify_numpy(source[0], outlines.loops[0, :L].cpu().numpy(), outlines.verts[0, :V].cpu().numpy(), tolerance)
        want = oracle.simplify_frame(source, oracle.TOLERANCES[tolerance])
        assert np.array_equal(counts, want[0]) and np.array_equal(loops, want[1]) and np.array_equal(verts, want[2])
        host = got.to_host()[0]
        assert len(host) == counts[0] > 8 and np.array_equal(got.counts[0].cpu().numpy(), counts) and counts[1] < V
        for (r, hole, pts), (wr, whole, wpts) in zip(host, contours_oracle.polygons(want)):
            assert (r, hole) == (wr, whole) and np.array_equal(pts, wpts)


def test_alter_res_batch_polygons(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_polygons' polygons are simplify_numpy's on the outlines of
    alter_res_batch_contours, with and without min_area."""
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
        polygons, labels = ev.alter_res_batch_polygons(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, tolerance)
        cleaned, labels_c = ev.alter_res_batch_polygons(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, tolerance, min_area=min_area)
        exact, _ = ev.alter_res_batch_contours(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, 0.5)
    assert isinstance(polygons, egress.SimplifiedContours) and isinstance(cleaned.source.frames, egress.AbsorbedFrames) and torch.equal(labels, labels_c)
    assert torch.equal(polygons.contours.counts, exact.counts)
    for which in (polygons, cleaned):
        host = which.to_host()
        before = which.contours
        need = before.counts.cpu().numpy()
        for n in range(gop - 1):
            L, V = need[n]
            counts, loops, verts = egress.simplify_numpy(need[n], before.loops[n, :L].cpu().numpy(), before.verts[n, :V].cpu().numpy(), tolerance)
            assert np.array_equal(which.counts[n].cpu().numpy(), counts) and len(host[n]) == counts[0]
            for (r, hole, pts), (wr, whole, wpts) in zip(host[n], contours_oracle.polygons((counts, loops, verts))):
                assert (r, hole) == (wr, whole) and np.array_equal(pts, wpts)
    print(f"\nvertices per frame {polygons.contours.counts[:, 1].cpu().tolist()} -> {polygons.counts[:, 1].cpu().tolist()} at {tolerance} px; "
          f"after absorbing regions below {min_area} pixels {cleaned.contours.counts[:, 1].cpu().tolist()} -> {cleaned.counts[:, 1].cpu().tolist()}")
