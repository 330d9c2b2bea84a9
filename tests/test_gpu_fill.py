"""GPU checks of the polygon fill (csrc/fill.hip, arseg_contours_fill_fwd; arseg_amd.egress.fill): planes, crossing counts and fidelity
counters against the oracle written from the contract on the pixel centres (tests/fill_oracle.py).  The unit tests upload outlines and
region records made by the oracles, so they stand on fill.hip alone; only the chain tests at the end run the encoder, the labelling,
the tracing and the simplification too.  Every output is an integer: every comparison is np.array_equal.  Nothing here provokes a
fault: malformed input is exercised only through the argument checks on the CPU (tests/test_fill.py)."""
import numpy as np
import pytest
import torch

import contours_oracle
import fill_oracle as oracle
import links_oracle
import regions_oracle
import rle_oracle
import simplify_oracle
import simplify_shared_oracle

pytestmark = pytest.mark.gpu

G32 = np.int32(contours_oracle.GUARD_WORD - (1 << 32))
GW = np.uint32(contours_oracle.GUARD_WORD)
G8 = np.uint8(0xA5)
EXTRA = 8
TOLERANCES = (0, 0.5, 1, 2, 4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _frame(loops, values, H, W, ref=None):
    """One frame of input with the oracle's answer: the arrays as the tracing and the simplify passes leave them, the values, the
    expected plane, crossings and counters."""
    values = np.asarray(values, dtype=np.int64)
    return dict(arrays=contours_oracle.arrays(loops), loops=loops, values=values, H=H, W=W, ref=ref, E=oracle.crossings(loops))


_OUTLINES = {}


def _outlines(plane, connectivity, kind="exact", tolerance=0):
    """The loops of a plane from the oracles -- contours_oracle's, simplify_oracle's ("plain") or simplify_shared_oracle's ("shared") --
    and the regions' values, computed once."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    key = (plane.shape, plane.tobytes(), connectivity)
    if key not in _OUTLINES:
        source = contours_oracle.trace_plane(plane, connectivity)
        _OUTLINES[key] = {"exact": source, "values": oracle.values_of(plane, source)}
    held, tol2_q = _OUTLINES[key], int(4 * tolerance) ** 2
    if kind != "exact" and (kind, tol2_q) not in held:
        if kind == "plain":
            held[(kind, tol2_q)] = simplify_oracle.simplify_loops(held["exact"], tol2_q)
        else:
            held[(kind, tol2_q)] = simplify_shared_oracle.simplify_plane(plane, connectivity, tol2_q, held["exact"])[0]
    return held["exact" if kind == "exact" else (kind, tol2_q)], held["values"]


def _of_plane(plane, connectivity=8, kind="exact", tolerance=0, ref=True):
    loops, values = _outlines(plane, connectivity, kind, tolerance)
    return _frame(loops, values, plane.shape[0], plane.shape[1], np.ascontiguousarray(plane, dtype=np.uint8) if ref else None)


def _upload(dev, a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def _run(dev, frames, background=255, ecap=None, pad=0, tail=0, with_stats=True, with_ref=None, workspace=None, refuse=None, sizing=False,
         lcap=None, vcap=None, rcap=None):
    """The frames' arrays uploaded (capacities: room for everything and 3 more; the slots beyond a frame's own guard filled),
    ops.contours_fill into guard filled buffers with EXTRA guard words behind them -> (planes [N,H,W], counts [N], stats [N,NSTATS])
    as numpy copies after checking them against the oracle frame by frame: a refused frame fully intact but for its count, an
    overflowed one too, the others exact; the guards behind and between the rows and images (``pad`` bytes behind every row, ``tail``
    behind every image); the inputs intact.  refuse: {frame: "negative" | "loops" | "verts" | "regions" | "records"}."""
    from arseg_amd import ops

    N, H, W = len(frames), frames[0]["H"], frames[0]["W"]
    lcap = max(len(f["arrays"][1]) for f in frames) + 3 if lcap is None else lcap
    vcap = max(len(f["arrays"][2]) for f in frames) + 3 if vcap is None else vcap
    rcap = max(len(f["values"]) for f in frames) + 3 if rcap is None else rcap
    ecap = (0 if sizing else max(f["E"] for f in frames)) if ecap is None else ecap
    with_ref = all(f["ref"] is not None for f in frames) if with_ref is None else with_ref
    counts, loops, verts = np.zeros((N, 2), np.int32), np.full((N, lcap, 4), G32, np.int32), np.full((N, vcap), GW, np.uint32)
    n_regions, records = np.zeros(N, np.int32), np.full((N, rcap, 8), oracle.GUARD_I64, np.int64)
    for n, f in enumerate(frames):
        c, l, v = f["arrays"]
        counts[n], loops[n, :len(l)], verts[n, :len(v)], n_regions[n] = c, l, v, len(f["values"])
        records[n] = oracle.records_of(f["values"], rcap)
    ok = np.ones(N, dtype=bool)
    for n, how in (refuse or {}).items():
        if how in ("regions", "records"):
            n_regions[n] = -1 if how == "regions" else rcap + 1
        else:
            counts[n] = {"negative": (-1, -1), "loops": (lcap + 1, counts[n, 1]), "verts": (counts[n, 0], vcap + 1)}[how]
        ok[n] = False
    host = [counts, loops, verts, n_regions, records]
    if with_ref:
        host.append(np.stack([f["ref"] for f in frames]))
    inputs = [_upload(dev, a) for a in host]
    pitch, stride = W + pad, H * (W + pad) + tail
    plane_back = torch.full((N * stride + EXTRA,), int(G8), dtype=torch.uint8, device=dev)
    counts_back = torch.from_numpy(np.full(N + EXTRA, G32, np.int32)).to(dev)
    stats_back = torch.from_numpy(np.full(N * oracle.NSTATS + EXTRA, oracle.GUARD_I64, np.int64)).to(dev)
    labels = None if sizing else plane_back.as_strided((N, H, W), (stride, pitch, 1))
    ops.contours_fill(*inputs[:5], H, W, labels, counts_back[:N], background=background, ref_labels=inputs[5] if with_ref else None,
                      stats=stats_back[:N * oracle.NSTATS].view(N, oracle.NSTATS) if with_stats else None, event_capacity=ecap,
                      workspace=workspace)
    plane_got, counts_got, stats_got = plane_back.cpu().numpy(), counts_back.cpu().numpy(), stats_back.cpu().numpy()
    for before, after in zip(host, inputs):
        assert np.array_equal(after.cpu().numpy().view(before.dtype), before)
    assert (counts_got[N:] == G32).all() and (stats_got[N * oracle.NSTATS:] == oracle.GUARD_I64).all()
    images = np.full((N, H, W + pad), G8, np.uint8)
    for n in range(N):
        assert (plane_got[n * stride + H * pitch:(n + 1) * stride] == G8).all(), n          # behind the image
        images[n] = plane_got[n * stride:n * stride + H * pitch].reshape(H, pitch)
    assert (plane_got[N * stride:] == G8).all() and (images[:, :, W:] == G8).all()                # behind the buffer and the rows
    planes, stats = images[:, :, :W], stats_got[:N * oracle.NSTATS].reshape(N, oracle.NSTATS)
    for n, f in enumerate(frames):
        assert counts_got[n] == (f["E"] if ok[n] else -1), (n, counts_got[n], f["E"])
        if not ok[n] or f["E"] > ecap or sizing:
            assert (planes[n] == G8).all() and (stats[n] == oracle.GUARD_I64).all(), n
            continue
        want, _, _, k = oracle.fill(f["loops"], f["values"], H, W, background)
        assert np.array_equal(planes[n], want), (n, np.argwhere(planes[n] != want)[:8])
        if with_stats:
            want_stats = oracle.stats(want, k, f["ref"] if with_ref else None)
            assert np.array_equal(stats[n], want_stats), (n, stats[n][:3], want_stats[:3], np.flatnonzero(stats[n] != want_stats)[:8])
        else:
            assert (stats[n] == oracle.GUARD_I64).all()
    return planes, counts_got[:N], stats


@pytest.mark.parametrize("case", oracle.HAND, ids=oracle.HAND_IDS)
def test_hand_made_cases(dev, case):
    """The planes written out by hand -- the centre on an edge, the bow-tie, the hole that is a region, the painter's rule, a loop listed
    twice (zero-length spans and gaps only), a two-vertex loop, an edge of dy = H, an edge along x = W --, at two backgrounds."""
    _, H, W, loops, _, gaps, excess, E = case
    for background in (255, 7):
        planes, counts, stats = _run(dev, [_frame(loops, oracle.HAND_VALUES, H, W)], background)
        assert np.array_equal(planes[0], oracle.hand_plane(case, background)) and counts[0] == E and stats[0, :3].tolist() == [gaps, excess, 0]


def _hand_planes():
    planes = [simplify_oracle.hand_plane(name) for name in simplify_oracle.HAND_IDS] + [np.array(h[1], dtype=np.uint8) for h in simplify_shared_oracle.HAND]
    seen, out = set(), []
    for plane in planes:
        if (plane.shape, plane.tobytes()) not in seen:
            seen.add((plane.shape, plane.tobytes()))
            out.append(plane)
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
def test_hand_made_planes(dev, connectivity):
    """Every hand plane of the simplify oracles: the exact outlines and both simplifications at the five tolerances, the eleven sets
    of outlines of a plane as the frames of one call, against the plane as the reference.  The shared borders leave no gap and no
    overlap; the exact outlines and tolerance 0 give the plane back."""
    for plane in _hand_planes():
        frames = [_of_plane(plane, connectivity)] + [_of_plane(plane, connectivity, kind, t) for kind in ("plain", "shared") for t in TOLERANCES]
        planes, _, stats = _run(dev, frames)
        assert (stats[6:, :2] == 0).all()
        for n in (0, 1, 6):
            assert np.array_equal(planes[n], plane) and (stats[n, :3] == 0).all()


def test_rows_with_chosen_numbers_of_crossings(dev):
    """Rows with 0, 2, 62, 64, 66, 126, 128 and 130 crossings -- around one and two strides of a wave and half a chunk of the pairing --
    as unit squares over every other column, dealt to three regions; and slivers whose two sides give the same column (zero-length
    spans)."""
    loops, H, W = oracle.bar_loops([0, 2, 62, 64, 66, 126, 128, 130])
    _, counts, stats = _run(dev, [_frame(loops, [3, 4, 5], H, W)])
    assert counts[0] == 578 and stats[0, :2].tolist() == [H * W - 289, 0]
    slivers = [(0, 0, [(0, 0), (1, 8), (0, 8)]), (1, 0, [(5, 0), (6, 0), (5, 8)]), (1, 0, [(9, 0), (9, 8)]), (0, 0, [(3, 1), (3, 7), (4, 4)])]
    _run(dev, [_frame(slivers, [3, 4], 8, 10)])


def test_a_row_beyond_the_staged_bucket(dev):
    """1024 crossings are paired in LDS; 1026 in place, from the bucket in global memory -- next to a row of 1024 and one of 4."""
    loops, H, W = oracle.bar_loops([1026, 1024, 4])
    _, counts, stats = _run(dev, [_frame(loops, [3, 4, 5], H, W)])
    assert counts[0] == 2054 and stats[0, 0] == H * W - 1027


def _blocks(seed, H, W, cell, values=4):
    """A seeded plane of cell x cell blocks of `values` values."""
    g = np.random.Generator(np.random.PCG64(seed))
    coarse = g.integers(0, values, size=((H + cell - 1) // cell, (W + cell - 1) // cell)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:H, :W])


@pytest.mark.parametrize("H,W", [(3, 1), (5, 63), (5, 64), (5, 65), (5, 257), (1, 40), (2, 8193)])
def test_widths_and_heights(dev, H, W):
    """W = 1, around a wave's stride and a workgroup's, H = 1, and one row wider than the owner line held in LDS (8192 columns): the
    exact outlines and both simplifications at 1 px give the oracle's planes."""
    plane = _blocks(W, H, W, 64 if W > 1000 else 2)
    frames = [_of_plane(plane), _of_plane(plane, 8, "plain", 1), _of_plane(plane, 8, "shared", 1)]
    planes, _, stats = _run(dev, frames)
    assert np.array_equal(planes[0], plane) and (stats[[0, 2], :2] == 0).all()


def test_pitch_and_image_stride(dev):
    """labels_out with 5 bytes behind every row and 7 behind every image: only the pixels are written."""
    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    got, _, _ = _run(dev, [_of_plane(p, 8, "shared", 1) for p in planes], pad=5, tail=7)
    assert got.shape == planes.shape
    got, _, _ = _run(dev, [_of_plane(p) for p in planes], pad=1, tail=0)
    assert np.array_equal(got, planes)


@pytest.mark.parametrize("count", [255, 256, 257])
def test_loop_counts_around_a_workgroup(dev, count):
    """A frame of exactly 255, 256 and 257 loops: the last workgroups of the launches that give a wave a loop."""
    plane = regions_oracle.REGION_COUNT_PLANES[count][0]
    frame = _of_plane(plane, 4)
    assert frame["arrays"][0][0] == count
    planes, _, _ = _run(dev, [frame, _of_plane(plane, 4, "shared", 1)])
    assert np.array_equal(planes[0], plane)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_seeded_planes_and_unlike_frames(dev, connectivity):
    """The seeded noise and the dense noise, exact and simplified both ways at 1 px; N = 2 with frames of different sizes of problem in
    both orders: a frame's result is the one the oracle gives for it alone."""
    for planes in (regions_oracle.noise_planes(*regions_oracle.NOISE), regions_oracle.dense_noise(*links_oracle.DENSE)):
        for kind in ("exact", "plain", "shared"):
            got, _, stats = _run(dev, [_of_plane(p, connectivity, kind, 1) for p in planes])
            assert kind == "plain" or ((stats[:, :2] == 0).all() and (kind == "shared" or np.array_equal(got, planes)))
    a, b = np.zeros((21, 21), np.uint8), np.zeros((21, 21), np.uint8)
    a[:] = regions_oracle.HAND["spiral-21x21"][0]
    b[:6, :6] = regions_oracle.HAND["checkerboard-6x6"][0]
    for pair in ((a, b), (b, a)):
        got, counts, _ = _run(dev, [_of_plane(p, connectivity) for p in pair])
        assert np.array_equal(got, np.stack(pair)) and counts[0] != counts[1]


@pytest.mark.parametrize("how", ["negative", "loops", "verts", "regions", "records"])
def test_refused_frames(dev, how):
    """A frame whose source was refused (counts -1), one that needs more loops than lcap or more vertices than vcap, one without
    regions (n_regions -1) and one with more regions than rcap: counts_out = -1 and every other buffer of that frame intact, the other
    frame of the call exact (_run checks both)."""
    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    for n in range(len(planes)):
        _, counts, _ = _run(dev, [_of_plane(p) for p in planes], refuse={n: how})
        assert counts[n] == -1 and all(counts[k] > 0 for k in range(len(planes)) if k != n)


def test_event_capacity_and_sizing(dev):
    """ecap equal to what the frame with the larger need asks for, one below it (that frame gets its count and nothing else, the other
    is exact), far below; and the sizing form (no labels_out, ecap 0): the counts stay exact."""
    frames = [_of_plane(p) for p in regions_oracle.noise_planes(*regions_oracle.NOISE)]
    need = [f["E"] for f in frames]
    assert need[0] != need[1]
    for ecap in (max(need), max(need) - 1, min(need), 1):
        _, counts, _ = _run(dev, frames, ecap=ecap)
        assert counts.tolist() == need
    _, counts, _ = _run(dev, frames, sizing=True)
    assert counts.tolist() == need


def test_own_workspace_and_bit_equality(dev):
    """Two runs of the same call are bit-equal; a caller's workspace of exactly the size asked for serves, with guards behind it; one byte
    less is refused; stats=None writes no counter."""
    from arseg_amd import _lib

    frames = [_of_plane(p, 8, "plain", 1) for p in regions_oracle.noise_planes(*regions_oracle.NOISE)]
    first = _run(dev, frames)
    N, H, W = len(frames), frames[0]["H"], frames[0]["W"]
    lcap, vcap, ecap = max(len(f["arrays"][1]) for f in frames) + 3, max(len(f["arrays"][2]) for f in frames) + 3, max(f["E"] for f in frames)
    nbytes = _lib.load().arseg_contours_fill_workspace_bytes(N, H, W, lcap, vcap, ecap)
    assert nbytes == (N * (8 * ecap + 8 * (H + 1)) + 15) // 16 * 16
    ws_back = torch.full((nbytes + 4 * EXTRA,), 0x5A, dtype=torch.uint8, device=dev)
    second = _run(dev, frames, workspace=ws_back[:nbytes])
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert (ws_back[nbytes:].cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.ArsegError):
        _run(dev, frames, workspace=ws_back[:nbytes - 1])
    third = _run(dev, frames, with_stats=False)
    assert np.array_equal(third[0], first[0])


def test_counters_against_a_reference(dev):
    """stats against the oracle's counts (_run compares all 771 of them) where the polygons changed pixels: plain simplification at 2 px
    (gaps, which count as changed, and overlaps) and shared borders at 2 px, with a background that is one of the plane's values, and
    the same outlines without a reference (changed, ref_area and both stay 0)."""
    plane = rle_oracle.blob_planes(3, 1, 32, 65, n_cls=5, cell=8)[0]
    background = int(plane[0, 0])
    frames = [_of_plane(plane, 8, "plain", 2), _of_plane(plane, 8, "shared", 2)]
    _, _, stats = _run(dev, frames, background=background)
    assert stats[0, 0] > 0 and stats[0, 1] > 0 and stats[0, 2] >= stats[0, 0] and stats[1, :2].tolist() == [0, 0] and stats[1, 2] > 0
    assert stats[:, 3:259].sum(axis=1).tolist() == [plane.size] * 2
    _, _, bare = _run(dev, frames, background=background, with_ref=False)
    assert np.array_equal(bare[:, :2], stats[:, :2]) and (bare[:, 2] == 0).all() and (bare[:, 3:259] == 0).all() and (bare[:, 515:] == 0).all()
    assert np.array_equal(bare[:, 259:515], stats[:, 259:515])


def _contour_frames(dev, frames, cap):
    """egress.ContourFrames holding the frames' arrays over RegionFrames with the oracle's values (the run code behind them is a
    placeholder of capacity cap)."""
    from arseg_amd import egress

    N, H, W = len(frames), frames[0]["H"], frames[0]["W"]
    lcap, vcap, rcap = (max(len(f["arrays"][i]) for f in frames) + 3 for i in (1, 2, 2))
    counts, loops, verts = np.zeros((N, 2), np.int32), np.zeros((N, lcap, 4), np.int32), np.zeros((N, vcap), np.uint32)
    n_regions, records = np.zeros(N, np.int32), np.zeros((N, rcap, 8), np.int64)
    for n, f in enumerate(frames):
        c, l, v = f["arrays"]
        counts[n], loops[n, :len(l)], verts[n, :len(v)], n_regions[n] = c, l, v, len(f["values"])
        records[n, :len(f["values"]), 0] = f["values"]
    code = egress.RleFrames(torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev), H, W)
    found = egress.RegionFrames(_upload(dev, n_regions), torch.zeros((N, cap), dtype=torch.int32, device=dev), _upload(dev, records), code)
    return egress.ContourFrames(_upload(dev, counts), _upload(dev, loops), _upload(dev, verts), found)


def test_one_graph_replayed_on_refilled_inputs(dev):
    """ops.contours_fill captured once (every buffer given: nothing is allocated); the inputs are refilled in place with another
    frame's arrays; each replay equals the oracle for its own input."""
    from arseg_amd import _lib, ops

    sides = [_of_plane(regions_oracle.noise_planes(s, 1, 12, 65)[0], 8, "shared", 1) for s in (31, 32)]
    H, W, ecap = 12, 65, 2 * 12 * 65
    held = [_contour_frames(dev, [f], 8) for f in sides]
    lcap, vcap = (max(h.loops.shape[1] for h in held), max(h.verts.shape[1] for h in held))
    rcap = max(h.source.records.shape[1] for h in held)

    def fit(t, shape):
        out = torch.zeros(shape, dtype=t.dtype, device=dev)
        out[tuple(slice(0, k) for k in t.shape)] = t
        return out

    sets = [[h.counts, fit(h.loops, (1, lcap, 4)), fit(h.verts, (1, vcap)), h.source.n_regions, fit(h.source.records, (1, rcap, 8)),
             _upload(dev, f["ref"][None])] for h, f in zip(held, sides)]
    inputs = [t.clone() for t in sets[0]]
    labels, counts = torch.zeros((1, H, W), dtype=torch.uint8, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    stats = torch.zeros((1, oracle.NSTATS), dtype=torch.int64, device=dev)
    ws = torch.zeros((_lib.load().arseg_contours_fill_workspace_bytes(1, H, W, lcap, vcap, ecap) // 8,), dtype=torch.int64, device=dev)

    def call():
        ops.contours_fill(*inputs[:5], H, W, labels, counts, ref_labels=inputs[5], stats=stats, event_capacity=ecap, workspace=ws)

    call()                                                                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    seen = []
    for which in (1, 0):
        for t, a in zip(inputs, sets[which]):
            t.copy_(a)
        labels.fill_(9)
        counts.fill_(-7)
        stats.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        f = sides[which]
        want, _, _, k = oracle.fill(f["loops"], f["values"], H, W)
        assert np.array_equal(labels[0].cpu().numpy(), want) and int(counts[0]) == f["E"]
        assert np.array_equal(stats[0].cpu().numpy(), oracle.stats(want, k, f["ref"]))
        seen.append(f["E"])
    assert seen[0] != seen[1]


def test_egress_fill_with_and_without_out(dev):
    """egress.fill on ContourFrames built from the oracles' arrays: planes, fidelity and the run code of the filled planes; with ``out``
    the same buffers are written again; a refused reference and an overflowed frame are named."""
    from arseg_amd import _lib, egress

    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    N, H, W = planes.shape
    frames = [_of_plane(p, 8, "plain", 1) for p in planes]
    held = _contour_frames(dev, frames, H * W)
    ref = torch.from_numpy(planes).to(dev)
    first = egress.fill(held, ref=ref)
    assert isinstance(first, egress.FilledFrames) and first.contours is held and first.event_capacity == 2 * H * W and first.needed() is first.counts
    again = egress.fill(held, background=3, ref=ref, out=first)
    assert again is first and again.background == 3
    other = egress.fill(held)
    for got, background, with_ref in ((again, 3, True), (other, 255, False)):
        rows = got.fidelity()
        for n, f in enumerate(frames):
            want, gaps, excess, k = oracle.fill(f["loops"], f["values"], H, W, background)
            assert np.array_equal(got.labels[n].cpu().numpy(), want) and int(got.counts[n]) == f["E"]
            counters = oracle.stats(want, k, planes[n] if with_ref else None)
            assert (rows[n]["gaps"], rows[n]["excess"], rows[n]["changed"]) == (gaps, excess, counters[2])
            union = counters[3:259] + counters[259:515] - counters[515:]
            assert rows[n]["iou"] == {int(v): float(counters[515 + v]) / float(union[v]) for v in np.flatnonzero(union)}
            assert rows[n]["miou"] == float(np.mean(list(rows[n]["iou"].values())))
    coded = again.rle(H * W)
    assert isinstance(coded, egress.RleFrames) and coded.labels is again.labels and torch.equal(coded.decode(), again.labels)
    with pytest.raises(_lib.ArsegError, match="frame 0 needs .* crossings, the capacity is 4"):
        egress.fill(held, event_capacity=4).fidelity()
    with pytest.raises(ValueError):
        egress.fill(held, ref=ref[:, :, :-1])


def test_real_chain_on_a_blob_plane(dev):
    """rle_of_planes -> regions -> contours -> simplify_shared -> fill(ref=True) -> fidelity() on a 64x65 blob plane: the filled plane
    is fill_numpy's on the polygons brought to the host, and the oracle's; the shared borders leave no gap and no overlap; the exact
    outlines give the plane back."""
    from arseg_amd import egress

    planes = rle_oracle.blob_planes(5, 1, 64, 65, n_cls=7, cell=8)
    N, H, W = planes.shape
    frames = egress.rle_of_planes(torch.from_numpy(planes).to(dev), H * W)
    found = egress.regions(frames, 1024)
    outlines = egress.contours(found)
    values = found.to_host()[0]["value"]
    back = egress.fill(outlines, ref=True)
    assert torch.equal(back.labels, torch.from_numpy(planes).to(dev)) and int(back.counts[0]) == 2 * int(frames.needed()[0])
    assert [back.fidelity()[0][key] for key in ("gaps", "excess", "changed", "miou")] == [0, 0, 0, 1.0]
    for tolerance in (0.5, 1.0, 2.0):
        got = egress.simplify_shared(outlines, tolerance)
        filled = egress.fill(got, ref=True)
        L, V = got.counts[0].cpu().numpy()
        arrays = (np.array([L, V]), got.loops[0, :L].cpu().numpy(), got.verts[0, :V].cpu().numpy())
        host = egress.fill_numpy(*arrays, values, H, W)
        want, gaps, excess, k = oracle.fill(contours_oracle.polygons(arrays), values, H, W)
        assert np.array_equal(host[0], want) and host[1:] == (gaps, excess) == (0, 0)
        assert np.array_equal(filled.labels[0].cpu().numpy(), want) and int(filled.counts[0]) <= 2 * int(frames.needed()[0])
        row = filled.fidelity()[0]
        assert (row["gaps"], row["excess"], row["changed"]) == (0, 0, int((want != planes[0]).sum()))
        assert row["miou"] == 1.0 if row["changed"] == 0 else (tolerance >= 1 and 0.5 < row["miou"] < 1)
        assert np.array_equal(filled.stats[0].cpu().numpy(), oracle.stats(want, k, planes[0]))
    plain = egress.fill(egress.simplify(outlines, 1.0), ref=True).fidelity()[0]
    assert plain["gaps"] > 0 and plain["excess"] > 0


def test_alter_res_batch_polygon_fidelity(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_polygon_fidelity gives, with and without shared borders, the
    plane fill_numpy gives for the polygons of the same call, compared with the labels of the same call."""
    import test_gpu_ingest_formats as tf
    from arseg_amd import egress, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop, tolerance = 64, 96, 4, 1.0
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"][1:gop]).to(dev)
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * (gop - 1)
        for shared in (False, True):
            polygons, filled, labels = ev.alter_res_batch_polygon_fidelity(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, tolerance,
                                                                           shared_borders=shared, background=254)
            assert isinstance(polygons, egress.SharedContours) == shared and isinstance(filled, egress.FilledFrames) and filled.contours is polygons
            rows, need, values = filled.fidelity(), polygons.counts.cpu().numpy(), polygons.source.to_host()
            truth = labels.cpu().numpy()
            for n in range(gop - 1):
                L, V = need[n]
                plane, gaps, excess = egress.fill_numpy(need[n], polygons.loops[n, :L].cpu().numpy(), polygons.verts[n, :V].cpu().numpy(),
                                                        values[n]["value"], H, W, 254)
                assert np.array_equal(filled.labels[n].cpu().numpy(), plane) and (rows[n]["gaps"], rows[n]["excess"]) == (gaps, excess)
                assert rows[n]["changed"] == int(((plane != truth[n]) | (plane == 254)).sum()) and (not shared or gaps == excess == 0)
            print(f"\nshared_borders={shared}: gaps {[r['gaps'] for r in rows]}, excess {[r['excess'] for r in rows]}, changed "
                  f"{[r['changed'] for r in rows]}, mIoU {[round(r['miou'], 4) for r in rows]} at {tolerance} px")
