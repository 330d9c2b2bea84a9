"""GPU checks of the absorption of small regions (csrc/absorb.hip, arseg_rle_absorb_fwd; arseg_amd.egress.absorb): the new run code, target
and n_absorbed against the oracle written from the contract (tests/absorb_oracle.py).  The unit tests upload run codes, run_region and
records made by the numpy oracles, so they stand on absorb.hip alone; only the two chain tests at the end run the encoder and the labelling
too.  Every output is an integer: every comparison is np.array_equal.  Nothing here provokes a fault: malformed input is exercised only
through the argument checks on the CPU (tests/test_absorb.py)."""
import numpy as np
import pytest
import torch

import absorb_oracle as oracle
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


def _run(dev, planes, min_area, protect=None, connectivity=8, cap=None, rcap=None, pcap=None, out_cap=None, tcap=None, n_regions=None,
         workspace=None):
    """The five input arrays made by the oracles (cap / rcap default: room for everything and 3 more) uploaded, ops.rle_absorb into guard
    filled buffers with EXTRA guard words behind them -> the numpy copies (n_absorbed [N], out_row_start [N,H+1], out_runs [N,out_cap],
    target [N,tcap]) after checking them against the oracle frame by frame (oracle.expected: a refused or overflowed frame fully intact,
    out_row_start exact, the words below out_cap exact and the rest intact, target exact below min(R, tcap) and intact above), the guards
    behind every buffer and the inputs intact."""
    from arseg_amd import ops

    N, H, W = planes.shape
    host = list(oracle.device_inputs(planes, cap, rcap, connectivity))
    if n_regions is not None:
        host[2] = np.array(n_regions, dtype=np.int32)
    row_start, runs, nreg, run_region, records = host
    cap, rcap = runs.shape[1], records.shape[1]
    out_cap = cap if out_cap is None else out_cap
    tcap = rcap if tcap is None else tcap
    pcap = 3 * cap if pcap is None else pcap
    inputs = _upload(dev, host)
    rs_back = _guarded(dev, N * (H + 1) + EXTRA, G32, np.int32)
    words_back = _guarded(dev, N * out_cap + EXTRA, GW.view(np.int32), np.int32)
    target_back = _guarded(dev, N * tcap + EXTRA, G32, np.int32)
    n_back = _guarded(dev, N + EXTRA, G32, np.int32)
    ops.rle_absorb(*inputs, H, W, min_area, rs_back[:N * (H + 1)].view(N, H + 1), words_back[:N * out_cap].view(N, out_cap), n_back[:N],
                   target=target_back[:N * tcap].view(N, tcap) if tcap else None, protect=protect, pair_capacity=pcap, workspace=workspace)
    rs_got, words_got = rs_back.cpu().numpy(), words_back.cpu().numpy().view(np.uint32)
    target_got, n_got = target_back.cpu().numpy(), n_back.cpu().numpy()
    assert (rs_got[N * (H + 1):] == G32).all() and (words_got[N * out_cap:] == GW).all()
    assert (target_got[N * tcap:] == G32).all() and (n_got[N:] == G32).all()
    for before, after in zip(host, inputs):
        assert np.array_equal(after.cpu().numpy().view(before.dtype), before)
    rs_got, words_got = rs_got[:N * (H + 1)].reshape(N, H + 1), words_got[:N * out_cap].reshape(N, out_cap)
    target_got = target_got[:N * tcap].reshape(N, tcap)
    for n in range(N):
        answer = oracle.absorb_plane(planes[n], min_area, protect, connectivity)
        processable = row_start[n, H] <= cap and 0 <= nreg[n] <= rcap
        want = oracle.expected(answer, processable, pcap, out_cap, tcap, np.full(H + 1, G32), np.full(out_cap, GW), np.full(tcap, G32))
        assert n_got[n] == want[0], (n, int(n_got[n]), want[0])
        assert np.array_equal(rs_got[n], want[1]), n
        assert np.array_equal(words_got[n], want[2]), n
        assert np.array_equal(target_got[n], want[3]), n
    return n_got[:N], rs_got, words_got, target_got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_hand_made_planes(dev, name, connectivity):
    """Against the oracle, and against the answers written out by hand."""
    _, options, _, want_start, want_words, want_target, want_absorbed = oracle.HAND[name]
    n_got, rs_got, words_got, target_got = _run(dev, oracle.hand_plane(name)[None], connectivity=connectivity, **options)
    assert n_got[0] == want_absorbed and rs_got[0].tolist() == want_start
    assert words_got[0, :len(want_words)].tolist() == want_words and target_got[0, :len(want_target)].tolist() == want_target


@pytest.mark.parametrize("shape", links_oracle.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_edge_shapes(dev, shape):
    """H = 3 at the widths around a wave of runs, small heights at W = 16: row noise (its constant rows meet everything above and below)
    and dense three-valued noise (every run has neighbours), two unlike frames per call."""
    H, W = shape
    _run(dev, regions_oracle.noise_planes(700 + W, 2, H, W), 3, connectivity=8)
    _run(dev, regions_oracle.dense_noise(800 + H + W, 2, H, W), 3, connectivity=4)
    _run(dev, regions_oracle.dense_noise(900 + H + W, 2, H, W), 4, protect={0}, connectivity=8)


@pytest.mark.parametrize("count", [255, 256, 257])
def test_run_and_region_counts(dev, count):
    """Exactly 255, 256 and 257 runs and regions: the 64-run passes of a wave over a row of that many runs, the predecessor across a pass
    boundary, the scan's carry.  All regions of these planes have one area, so a protected value makes half of them stable."""
    stripes = regions_oracle.RUN_COUNT_PLANES[count]
    n_got, _, _, _ = _run(dev, stripes, 33, protect={10})
    assert n_got[0] >= 8
    pairs = regions_oracle.REGION_COUNT_PLANES[count]
    n_got, rs_got, _, _ = _run(dev, pairs, 3, protect={1}, connectivity=4)
    assert n_got[0] == count // 2 and rs_got[0].tolist() == [0, 1, 2]                            # every 8 went into the 1 to its left
    _run(dev, regions_oracle.alternating(count), 2, protect={8})


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H", [256, 257, 513])
def test_tall_planes(dev, H, connectivity):
    """More rows than one 256-entry pass of the scan over out_row_start: exactly one pass, one row into the second, one into the third.
    Narrow dense noise, so that every row has runs and specks; two unlike frames per call."""
    _run(dev, regions_oracle.dense_noise(1000 + H, 2, H, 5), 3, connectivity=connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_seeded_planes_and_unlike_frames(dev, connectivity):
    """The seeded noise, and N = 2 with frames of different sizes of problem in both orders: a frame's result is the one it has alone."""
    noise = regions_oracle.noise_planes(*regions_oracle.NOISE)
    _run(dev, noise, 4, connectivity=connectivity)
    _run(dev, noise, 6, protect={0, 127}, connectivity=connectivity)
    a, b = np.zeros((1, 21, 21), np.uint8), np.zeros((1, 21, 21), np.uint8)
    a[0] = regions_oracle.HAND["spiral-21x21"][0]
    a[0, 5, 5], a[0, 10, 11], a[0, 10, 12] = 9, 9, 9                                              # specks on the wall and in the corridor
    b[0, :6, :6] = regions_oracle.HAND["checkerboard-6x6"][0]
    for pair in (np.concatenate([a, b]), np.concatenate([b, a])):
        got = _run(dev, pair, 3, connectivity=connectivity)
        for n in range(2):
            alone = _run(dev, pair[n:n + 1], 3, connectivity=connectivity, cap=got[2].shape[1], rcap=got[3].shape[1])
            assert all(np.array_equal(g[n], s[0]) for g, s in zip(got, alone))


def test_seeded_blob_planes(dev):
    for _, planes, min_area, protect in oracle.seeded_cases()[:2]:
        n_got, _, _, _ = _run(dev, planes, min_area, protect)
        assert (n_got > 0).all()


def test_refused_frames(dev):
    """A frame whose run code overflowed, one with more regions than records and one with n_regions = -1: n_absorbed = -1 and every other
    buffer of that frame intact, the other frames of the call exact (_run checks both through oracle.expected)."""
    planes = rle_oracle.build(rle_oracle.CASES[1])
    min_area = oracle.median_area(planes[0])
    need = [len(r) for r in rle_oracle.encode(planes)[1]]
    worst = int(np.argmax(need))
    n_got, _, _, _ = _run(dev, planes, min_area, cap=max(need) - 1)
    assert n_got[worst] == -1 and all(n_got[n] > 0 for n in range(len(need)) if n != worst)
    R = [l[0] for l in regions_oracle.label_planes(planes, 8)]
    most = int(np.argmax(R))
    assert min(R) < max(R)
    n_got, _, _, _ = _run(dev, planes, min_area, rcap=max(R) - 1)
    assert n_got[most] == -1 and all(n_got[n] > 0 for n in range(len(R)) if R[n] < max(R))
    n_got, _, _, _ = _run(dev, planes, min_area, n_regions=[R[0], -1, R[2]])
    assert n_got.tolist()[1] == -1 and n_got[0] > 0 and n_got[2] > 0


def test_pair_capacity(dev):
    """pcap = 1 on a frame with two pairs: -2 and the frame intact; pcap = exactly the pairs: every slot taken, the answer exact; on the
    noise planes one pair fewer than the frame with most pairs has refuses that frame alone."""
    plane = oracle.hand_plane("tie-to-the-smaller-index")[None]
    assert oracle.absorb_plane(plane[0], 2)["pairs"] == 2
    assert _run(dev, plane, 2, pcap=1)[0][0] == -2
    assert _run(dev, plane, 2, pcap=2)[0][0] == 1
    noise = regions_oracle.noise_planes(*regions_oracle.NOISE)
    pairs = [oracle.absorb_plane(p, 4)["pairs"] for p in noise]
    assert min(pairs) < max(pairs) and min(pairs) > 2
    n_got = _run(dev, noise, 4, pcap=max(pairs))[0]
    assert (n_got > 0).all()
    n_got = _run(dev, noise, 4, pcap=max(pairs) - 1)[0]
    assert sorted(n_got.tolist())[0] == -2 and n_got.max() > 0


def test_output_capacities(dev):
    """out_cap below what the result needs: the words below it exact, the rest intact, out_row_start exact; target capacities R, R // 2 and
    0 (not wanted)."""
    planes = rle_oracle.build(rle_oracle.CASES[0])
    min_area = oracle.median_area(planes[0])
    need = [len(oracle.absorb_plane(p, min_area)["runs"]) for p in planes]
    for out_cap in (max(need), min(need) - 1, min(need) // 2, 1):
        n_got, rs_got, _, _ = _run(dev, planes, min_area, out_cap=out_cap)
        assert rs_got[:, -1].tolist() == need and (n_got > 0).all()
    R = min(l[0] for l in regions_oracle.label_planes(planes, 8))
    for tcap in (R, R // 2, 0):
        _run(dev, planes, min_area, tcap=tcap)


def test_own_workspace_and_bit_equality(dev):
    """Two runs of the same call are bit-equal (integer atomics); a caller's workspace of exactly the size asked for serves, with guards
    behind it; one byte less is refused."""
    from arseg_amd import _lib

    planes = np.concatenate([regions_oracle.noise_planes(*regions_oracle.NOISE), regions_oracle.dense_noise(9, 1, 12, 65)])
    first = _run(dev, planes, 4)
    N, H, W = planes.shape
    cap, rcap = first[2].shape[1], first[3].shape[1]
    nbytes = _lib.load().arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, 3 * cap)
    assert nbytes == N * (48 * cap + 8 * rcap + 8)
    ws_back = torch.full((nbytes // 8 + EXTRA,), int(oracle.GUARD_I64), dtype=torch.int64, device=dev)
    second = _run(dev, planes, 4, workspace=ws_back[:nbytes // 8])
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert (ws_back[nbytes // 8:].cpu().numpy() == np.int64(oracle.GUARD_I64)).all()
    with pytest.raises(_lib.ArsegError):
        _run(dev, planes, 4, workspace=ws_back[:nbytes // 8 - 1])


def test_one_graph_replayed_on_refilled_inputs(dev):
    """ops.rle_absorb captured once (every buffer given: nothing is allocated); the inputs are refilled in place with another frame's arrays;
    each replay equals the oracle for its own input."""
    from arseg_amd import _lib, ops

    frames = [regions_oracle.noise_planes(s, 1, 12, 65) for s in (31, 32)]
    sides = [oracle.device_inputs(f, cap=400, rcap=400) for f in frames]
    N, H, W, cap, rcap = 1, 12, 65, 400, 400
    inputs = _upload(dev, sides[0])
    out_rs = torch.zeros((N, H + 1), dtype=torch.int32, device=dev)
    out_runs, target = torch.zeros((N, cap), dtype=torch.int32, device=dev), torch.zeros((N, rcap), dtype=torch.int32, device=dev)
    n_abs = torch.zeros((N,), dtype=torch.int32, device=dev)
    ws = torch.zeros((_lib.load().arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, 3 * cap) // 8,), dtype=torch.int64, device=dev)

    def call():
        ops.rle_absorb(*inputs, H, W, 4, out_rs, out_runs, n_abs, target=target, protect={0}, workspace=ws)

    call()                                                                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    counts = []
    for side, plane in ((sides[1], frames[1]), (sides[0], frames[0])):
        for t, a in zip(inputs, _upload(dev, side)):
            t.copy_(a)
        for t in (out_rs, out_runs, target, n_abs):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        want = oracle.absorb_plane(plane[0], 4, {0})
        k, R = len(want["runs"]), len(want["target"])
        assert int(n_abs[0]) == want["n_absorbed"] and np.array_equal(out_rs[0].cpu().numpy(), want["row_start"])
        assert np.array_equal(out_runs[0, :k].cpu().numpy().view(np.uint32), want["runs"]) and (out_runs[0, k:] == -7).all()
        assert np.array_equal(target[0, :R].cpu().numpy(), want["target"]) and (target[0, R:] == -7).all()
        counts.append(k)
    assert counts[0] != counts[1]


def test_egress_absorb_with_and_without_out(dev):
    """egress.absorb on RegionFrames built from the oracles' arrays: the AbsorbedFrames' host copies equal the oracle; with ``out`` the same
    buffers are written again; a refused frame is named by to_host."""
    from arseg_amd import _lib, egress

    planes = regions_oracle.noise_planes(*regions_oracle.NOISE)
    N, H, W = planes.shape
    row_start, runs, nreg, run_region, records = _upload(dev, oracle.device_inputs(planes))
    found = egress.RegionFrames(nreg, run_region, records, egress.RleFrames(row_start, runs, H, W))
    first = egress.absorb(found, 4, protect={127})
    assert isinstance(first, egress.AbsorbedFrames) and first.source is found and first.pair_capacity == 3 * runs.shape[1]
    again = egress.absorb(found, 6, out=first)
    assert again is first
    for min_area, protect, got in ((6, None, again), (4, [0], egress.absorb(found, 4, protect=[0]))):
        host, targets = got.to_host(), got.targets_to_host()
        for n in range(N):
            want = oracle.absorb_plane(planes[n], min_area, protect)
            assert np.array_equal(host[n][0], want["row_start"]) and np.array_equal(host[n][1], want["runs"])
            assert np.array_equal(targets[n], want["target"]) and int(got.n_absorbed[n]) == want["n_absorbed"]
        assert np.array_equal(got.decode().cpu().numpy(), np.stack([oracle.absorb_plane(p, min_area, protect)["plane"] for p in planes]))
    with pytest.raises(_lib.ArsegError, match="frame 0 has more neighbour pairs than the pair capacity 1"):
        egress.absorb(found, 4, pair_capacity=1).to_host()


def test_real_chain_on_a_blob_plane(dev):
    """ops.labels_rle -> ops.rle_regions -> ops.rle_absorb -> ops.rle_decode on a 64x65 blob plane: the decoded plane is the oracle's, and
    labelling the new code gives no region below min_area that has a stable neighbour."""
    from arseg_amd import ops

    planes = rle_oracle.blob_planes(5, 1, 64, 65, n_cls=7, cell=8)
    N, H, W = planes.shape
    min_area = oracle.median_area(planes[0])
    want = oracle.absorb_plane(planes[0], min_area)
    assert want["n_absorbed"] > 3
    cap, rcap = H * W, 1024
    row_start, runs = torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev)
    nreg, run_region = torch.zeros((N,), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev)
    records = torch.zeros((N, rcap, 8), dtype=torch.int64, device=dev)
    ops.labels_rle(torch.from_numpy(planes).to(dev), row_start, runs)
    ops.rle_regions(row_start, runs, H, W, nreg, run_region, records)
    out_rs, out_runs = torch.zeros_like(row_start), torch.zeros_like(runs)
    n_abs, target = torch.zeros_like(nreg), torch.zeros((N, rcap), dtype=torch.int32, device=dev)
    ops.rle_absorb(row_start, runs, nreg, run_region, records, H, W, min_area, out_rs, out_runs, n_abs, target=target)
    back = ops.rle_decode(out_rs, out_runs, torch.full((N, H, W), 77, dtype=torch.uint8, device=dev))
    assert int(n_abs[0]) == want["n_absorbed"] and np.array_equal(back[0].cpu().numpy(), want["plane"])
    assert np.array_equal(out_rs[0].cpu().numpy(), want["row_start"])
    assert np.array_equal(target[0, :int(nreg[0])].cpu().numpy(), want["target"])
    ops.rle_regions(out_rs, out_runs, H, W, nreg, run_region, records)
    assert int(nreg[0]) == regions_oracle.label_planes(want["plane"][None], 8)[0][0]


def test_alter_res_batch_absorb(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_absorb's code and regions are absorb_numpy's and the oracle's
    on alter_res_batch_regions' run code."""
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
        before, labels_b = ev.alter_res_batch_regions(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, 0.5)
        found, labels = ev.alter_res_batch_absorb(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, min_area, 0.5)
    assert isinstance(found, egress.RegionFrames) and isinstance(found.frames, egress.AbsorbedFrames) and torch.equal(labels, labels_b)
    host, targets = found.frames.to_host(), found.frames.targets_to_host()
    records = found.to_host()
    for n, (rs, words) in enumerate(before.frames.to_host()):
        want = egress.absorb_numpy(rs, words, H, W, min_area)
        assert np.array_equal(host[n][0], want[0]) and np.array_equal(host[n][1], want[1]) and np.array_equal(targets[n], want[2])
        answer = oracle.absorb_plane(labels_b[n].cpu().numpy(), min_area)
        assert np.array_equal(found.frames.decode()[n].cpu().numpy(), answer["plane"])
        assert len(records[n]) == regions_oracle.label_planes(answer["plane"][None], 8)[0][0]
    print(f"\nabsorbed per frame {found.frames.n_absorbed.cpu().tolist()}, regions before {before.n_regions.cpu().tolist()} after "
          f"{found.n_regions.cpu().tolist()}")
