"""GPU checks of the region outlines (csrc/contours.hip, arseg_rle_contours_fwd; arseg_amd.egress.contours): counts, loops and vertices
against the oracle written from the contract on the pixel plane (tests/contours_oracle.py).  The unit tests upload run codes and
run_region made by the numpy oracles, so they stand on contours.hip alone; only the two chain tests at the end run the encoder and the
labelling too.  Every output is an integer: every comparison is np.array_equal.  Nothing here provokes a fault: malformed input is
exercised only through the argument checks on the CPU (tests/test_contours.py)."""
import numpy as np
import pytest
import torch

import contours_oracle as oracle
import links_oracle
import regions_oracle
import rle_oracle

pytestmark = pytest.mark.gpu

G32 = np.int32(oracle.GUARD_I32)
GW = np.uint32(oracle.GUARD_WORD)
EXTRA = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _guarded(dev, n, guard, dtype):
    return torch.from_numpy(np.full(n, guard, dtype=dtype)).to(dev)


def _upload(dev, arrays):
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in arrays]


_ANSWERS = {}


def _answer(plane, connectivity):
    """The oracle's answer for a plane, computed once."""
    key = (plane.shape, plane.tobytes(), connectivity)
    if key not in _ANSWERS:
        _ANSWERS[key] = oracle.contour_plane(plane, connectivity)
    return _ANSWERS[key]


def _run(dev, planes, connectivity=8, cap=None, lcap=None, vcap=None, n_regions=None, workspace=None):
    """The four input arrays made by the oracles (cap default: room for every run and 3 more) uploaded, ops.rle_contours into guard filled
    buffers with EXTRA guard words behind them -> the numpy copies (counts [N,2], loops [N,lcap,4], verts [N,vcap]) after checking them
    against the oracle frame by frame (oracle.expected: a refused frame fully intact but for its counts, counts exact, the rows below
    lcap and the words below vcap exact and the rest intact), the guards behind every buffer and the inputs intact.  lcap / vcap default
    to the bounds that cannot overflow; 0: that buffer is not handed over."""
    from arseg_amd import ops

    planes = np.ascontiguousarray(planes)
    N, H, W = planes.shape
    host = list(oracle.device_inputs(planes, cap, connectivity))
    if n_regions is not None:
        host[2] = np.array(n_regions, dtype=np.int32)
    row_start, runs, nreg, run_region = host
    cap = runs.shape[1]
    lcap = cap if lcap is None else lcap
    vcap = 4 * cap if vcap is None else vcap
    inputs = _upload(dev, host)
    counts_back = _guarded(dev, 2 * N + EXTRA, G32, np.int32)
    loops_back = _guarded(dev, 4 * N * lcap + EXTRA, G32, np.int32)
    verts_back = _guarded(dev, N * vcap + EXTRA, GW.view(np.int32), np.int32)
    ops.rle_contours(*inputs, H, W, counts_back[:2 * N].view(N, 2), loops=loops_back[:4 * N * lcap].view(N, lcap, 4) if lcap else None,
                     verts=verts_back[:N * vcap].view(N, vcap) if vcap else None, connectivity=connectivity, workspace=workspace)
    counts_got, loops_got = counts_back.cpu().numpy(), loops_back.cpu().numpy()
    verts_got = verts_back.cpu().numpy().view(np.uint32)
    assert (counts_got[2 * N:] == G32).all() and (loops_got[4 * N * lcap:] == G32).all() and (verts_got[N * vcap:] == GW).all()
    for before, after in zip(host, inputs):
        assert np.array_equal(after.cpu().numpy().view(before.dtype), before)
    counts_got, loops_got, verts_got = counts_got[:2 * N].reshape(N, 2), loops_got[:4 * N * lcap].reshape(N, lcap, 4), verts_got[:N * vcap].reshape(N, vcap)
    for n in range(N):
        processable = row_start[n, H] <= cap and nreg[n] >= 0
        want = oracle.expected(_answer(planes[n], connectivity), processable, lcap, vcap, np.full(2, G32), np.full((lcap, 4), G32), np.full(vcap, GW))
        assert np.array_equal(counts_got[n], want[0]), (n, counts_got[n], want[0])
        assert np.array_equal(loops_got[n], want[1]), n
        assert np.array_equal(verts_got[n], want[2]), n
    return counts_got, loops_got, verts_got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_hand_made_planes(dev, name, connectivity):
    """Against the oracle, and against the loops written out by hand."""
    counts, loops, verts = _run(dev, oracle.hand_plane(name)[None], connectivity)
    want = oracle.hand_arrays(name, connectivity)
    L, V = want[0]
    assert counts[0].tolist() == [L, V] and np.array_equal(loops[0, :L], want[1]) and np.array_equal(verts[0, :V], want[2])


@pytest.mark.parametrize("shape", links_oracle.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_edge_shapes(dev, shape):
    """H = 3 at the widths around a wave of runs, small heights at W = 16: row noise (its constant rows meet everything above and below)
    and dense three-valued noise (every run has neighbours, many saddles), two unlike frames per call."""
    H, W = shape
    _run(dev, regions_oracle.noise_planes(700 + W, 2, H, W), 8)
    _run(dev, regions_oracle.dense_noise(800 + H + W, 2, H, W), 4)
    _run(dev, regions_oracle.dense_noise(900 + H + W, 2, H, W), 8)


@pytest.mark.parametrize("count", [255, 256, 257])
def test_run_and_region_counts(dev, count):
    """Exactly 255, 256 and 257 runs and regions: the 64-run passes of a wave over a row of that many runs, the scan's carry, the edge
    array across a workgroup's 256 edges."""
    counts, _, _ = _run(dev, regions_oracle.RUN_COUNT_PLANES[count])
    assert counts[0, 0] >= 16
    counts, _, _ = _run(dev, regions_oracle.REGION_COUNT_PLANES[count], 4)
    assert counts[0].tolist() == [count, 4 * count]                                              # every region a column of two pixels
    _run(dev, regions_oracle.alternating(count))


@pytest.mark.parametrize("name", list(oracle.LONG))
def test_long_loops_and_the_number_of_jumps(dev, name):
    """The spirals and the comb -- one loop longer than a wave, in the larger spiral than a workgroup -- with cap equal to the run count and
    with a cap many times larger: the number of jump launches changes, the answer does not."""
    plane = np.ascontiguousarray(oracle.LONG[name])[None]
    need = len(rle_oracle.encode(plane)[1][0])
    for connectivity in (4, 8):
        tight = _run(dev, plane, connectivity, cap=need)
        wide = _run(dev, plane, connectivity, cap=37 * need + 5)
        L, V = tight[0][0]
        assert np.array_equal(tight[0], wide[0]) and np.array_equal(tight[1][0, :L], wide[1][0, :L]) and np.array_equal(tight[2][0, :V], wide[2][0, :V])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_seeded_planes_and_unlike_frames(dev, connectivity):
    """The seeded noise and the dense noise, and N = 2 with frames of different sizes of problem in both orders: a frame's result is the
    one it has alone."""
    _run(dev, regions_oracle.noise_planes(*regions_oracle.NOISE), connectivity)
    _run(dev, regions_oracle.dense_noise(*links_oracle.DENSE), connectivity)
    a, b = np.zeros((1, 21, 21), np.uint8), np.zeros((1, 21, 21), np.uint8)
    a[0] = regions_oracle.HAND["spiral-21x21"][0]
    b[0, :6, :6] = regions_oracle.HAND["checkerboard-6x6"][0]
    for pair in (np.concatenate([a, b]), np.concatenate([b, a])):
        got = _run(dev, pair, connectivity)
        for n in range(2):
            alone = _run(dev, pair[n:n + 1], connectivity, cap=got[2].shape[1] // 4)
            assert all(np.array_equal(g[n], s[0]) for g, s in zip(got, alone))


def test_refused_frames(dev):
    """A frame whose run code overflowed and one with n_regions = -1: counts = {-1, -1} and every other buffer of that frame intact, the
    other frames of the call exact (_run checks both through oracle.expected)."""
    planes = rle_oracle.build(rle_oracle.CASES[1])
    need = [len(r) for r in rle_oracle.encode(planes)[1]]
    worst = int(np.argmax(need))
    counts, _, _ = _run(dev, planes, cap=max(need) - 1)
    assert counts[worst].tolist() == [-1, -1] and all(counts[n, 0] > 0 for n in range(len(need)) if n != worst)
    R = [l[0] for l in regions_oracle.label_planes(planes, 8)]
    counts, _, _ = _run(dev, planes, n_regions=[R[0], -1, R[2]])
    assert counts[1].tolist() == [-1, -1] and counts[0, 0] > 0 and counts[2, 0] > 0


def test_output_capacities_and_sizing(dev):
    """lcap and vcap equal to, and one below, what the frame with the largest need asks for; far below; and the two sizing forms (no
    loops, no vertices): counts stay exact, `first` too."""
    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    needs = np.stack([_answer(p, 8)[0] for p in planes])
    L, V = needs.max(axis=0)
    assert needs[:, 0].min() < L and needs[:, 1].min() < V                                      # the other frame still fits one below
    for lcap, vcap in ((L, V), (L - 1, V), (L, V - 1), (L - 1, V - 1), (1, 1), (0, V), (L, 0), (0, 0)):
        counts, _, _ = _run(dev, planes, lcap=int(lcap), vcap=int(vcap))
        assert np.array_equal(counts, needs)


def test_own_workspace_and_bit_equality(dev):
    """Two runs of the same call are bit-equal; a caller's workspace of exactly the size asked for serves, with guards behind it; one byte
    less is refused."""
    from arseg_amd import _lib

    planes = np.concatenate([regions_oracle.noise_planes(*regions_oracle.NOISE), regions_oracle.dense_noise(9, 1, 12, 65)])
    first = _run(dev, planes)
    N, cap = planes.shape[0], first[1].shape[1]
    nbytes = _lib.load().arseg_rle_contours_workspace_bytes(N, cap)
    assert nbytes == N * cap * 80
    ws_back = torch.full((nbytes // 4 + EXTRA,), int(G32), dtype=torch.int32, device=dev)
    second = _run(dev, planes, workspace=ws_back[:nbytes // 4])
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert (ws_back[nbytes // 4:].cpu().numpy() == G32).all()
    with pytest.raises(_lib.ArsegError):
        _run(dev, planes, workspace=ws_back[:nbytes // 4 - 1])


def test_one_graph_replayed_on_refilled_inputs(dev):
    """ops.rle_contours captured once (every buffer given: nothing is allocated); the inputs are refilled in place with another frame's
    arrays; each replay equals the oracle for its own input."""
    from arseg_amd import _lib, ops

    frames = [regions_oracle.noise_planes(s, 1, 12, 65) for s in (31, 32)]
    N, H, W, cap = 1, 12, 65, 400
    sides = [oracle.device_inputs(f, cap=cap) for f in frames]
    inputs = _upload(dev, sides[0])
    counts = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    loops, verts = torch.zeros((N, cap, 4), dtype=torch.int32, device=dev), torch.zeros((N, 4 * cap), dtype=torch.int32, device=dev)
    ws = torch.zeros((_lib.load().arseg_rle_contours_workspace_bytes(N, cap) // 4,), dtype=torch.int32, device=dev)

    def call():
        ops.rle_contours(*inputs, H, W, counts, loops=loops, verts=verts, workspace=ws)

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
        want = _answer(plane[0], 8)
        L, V = want[0]
        assert np.array_equal(counts[0].cpu().numpy(), want[0])
        assert np.array_equal(loops[0, :L].cpu().numpy(), want[1]) and (loops[0, L:] == -7).all()
        assert np.array_equal(verts[0, :V].cpu().numpy().view(np.uint32), want[2]) and (verts[0, V:] == -7).all()
        seen.append(int(V))
    assert seen[0] != seen[1]


def test_egress_contours_with_and_without_out(dev):
    """egress.contours on RegionFrames built from the oracles' arrays, at the connectivity they carry: the host polygons equal the
    oracle's; with ``out`` the same buffers are written again; an overflowed frame is named by to_host."""
    from arseg_amd import _lib, egress

    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    N, H, W = planes.shape
    made = {}
    for connectivity in (4, 8):
        row_start, runs, nreg, run_region = _upload(dev, oracle.device_inputs(planes, connectivity=connectivity))
        records = torch.zeros((N, 1, 8), dtype=torch.int64, device=dev)
        made[connectivity] = egress.RegionFrames(nreg, run_region, records, egress.RleFrames(row_start, runs, H, W), connectivity)
    first = egress.contours(made[4])
    cap = made[4].frames.capacity
    assert isinstance(first, egress.ContourFrames) and first.source is made[4] and (first.loop_capacity, first.vertex_capacity) == (cap, 4 * cap)
    again = egress.contours(made[8], out=first)
    assert again is first and again.source is made[8]
    for connectivity, got in ((8, again), (4, egress.contours(made[4]))):
        host = got.to_host()
        for n in range(N):
            want = oracle.polygons(_answer(planes[n], connectivity))
            assert len(host[n]) == len(want) == int(got.needed()[n, 0])
            for (r, hole, pts), (wr, whole, wpts) in zip(host[n], want):
                assert (r, hole) == (wr, whole) and pts.dtype == np.int32 and np.array_equal(pts, wpts)
    with pytest.raises(_lib.ArsegError, match="frame 0 needs .* the capacities are 1 and 4"):
        egress.contours(made[8], loop_capacity=1, vertex_capacity=4).to_host()


def test_real_chain_on_a_blob_plane(dev):
    """ops.labels_rle -> ops.rle_regions -> egress.contours -> to_host() on a 64x65 blob plane: the polygons are contours_numpy's on the
    code brought to the host, and the oracle's."""
    from arseg_amd import egress

    planes = rle_oracle.blob_planes(5, 1, 64, 65, n_cls=7, cell=8)
    N, H, W = planes.shape
    frames = egress.rle_of_planes(torch.from_numpy(planes).to(dev), H * W)
    found = egress.regions(frames, 1024)
    got = egress.contours(found).to_host()[0]
    row_start, runs = frames.to_host()[0]
    counts, loops, verts = egress.contours_numpy(row_start, runs, H, W)
    want = oracle.contour_plane(planes[0])
    assert np.array_equal(counts, want[0]) and np.array_equal(loops, want[1]) and np.array_equal(verts, want[2])
    assert len(got) == counts[0] > 8
    for (r, hole, pts), (wr, whole, wpts) in zip(got, oracle.polygons(want)):
        assert (r, hole) == (wr, whole) and np.array_equal(pts, wpts)


def test_alter_res_batch_contours(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_contours' polygons are contours_numpy's on
    alter_res_batch_regions' run code; with min_area they are those of the absorbed masks."""
    import test_gpu_ingest_formats as tf
    from arseg_amd import egress, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop, min_area = 64, 96, 4, 12
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"][1:gop]).to(dev)
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * (gop - 1)
        outlines, labels = ev.alter_res_batch_contours(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, 0.5)
        cleaned, labels_c = ev.alter_res_batch_contours(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, 0.5, min_area=min_area)
    assert isinstance(outlines, egress.ContourFrames) and isinstance(cleaned.source.frames, egress.AbsorbedFrames) and torch.equal(labels, labels_c)
    for which in (outlines, cleaned):
        host = which.to_host()
        for n, (rs, words) in enumerate(which.source.frames.to_host()):
            counts, loops, verts = egress.contours_numpy(rs, words, H, W)
            assert np.array_equal(which.counts[n].cpu().numpy(), counts) and len(host[n]) == counts[0]
            for (r, hole, pts), (wr, whole, wpts) in zip(host[n], oracle.polygons((counts, loops, verts))):
                assert (r, hole) == (wr, whole) and np.array_equal(pts, wpts)
    for n in range(gop - 1):
        want = oracle.contour_plane(labels[n].cpu().numpy())
        assert np.array_equal(outlines.counts[n].cpu().numpy(), want[0])
    print(f"\nloops per frame {outlines.counts[:, 0].cpu().tolist()}, vertices {outlines.counts[:, 1].cpu().tolist()}; after absorbing "
          f"regions below {min_area} pixels {cleaned.counts[:, 0].cpu().tolist()} and {cleaned.counts[:, 1].cpu().tolist()}")
