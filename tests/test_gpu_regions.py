"""GPU checks of the connected regions of a run code (csrc/regions.hip, arseg_rle_regions_fwd; arseg_amd.egress.regions): n_regions, the
region number of every run and the records against the oracle written from the contract (tests/regions_oracle.py), on run codes the
encoder of csrc/rle.hip wrote.  Every output is an integer: every comparison is np.array_equal.  Nothing here provokes a fault: malformed
run codes are exercised only through the argument checks on the CPU (tests/test_regions.py)."""
import numpy as np
import pytest
import torch

import consistency_oracle
import regions_oracle as oracle
import rle_oracle

pytestmark = pytest.mark.gpu

G32 = np.int32(oracle.GUARD_I32)
G64 = np.int64(oracle.GUARD_I64)
EXTRA = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from arseg_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _guarded(dev, n, guard, dtype):
    return torch.from_numpy(np.full(n, guard, dtype=dtype)).to(dev)


def _run(dev, planes, connectivity, cap=None, rcap=None, with_regions=True):
    """ops.labels_rle into runs [N,cap] (default: room for every run), then ops.rle_regions into 0x5A-filled buffers with EXTRA guard words /
    rows behind them (rcap default: room for every region) -> the numpy copies (n_regions, run_region [N,cap], regions [N,rcap,8] | None)
    after checking them against the oracle: n_regions exact, run_region exact below the needed runs and intact above, the records exact
    below min(R, rcap) and intact above, a frame whose run code overflowed intact, the guards behind every buffer intact."""
    from arseg_amd import ops

    N, H, W = planes.shape
    want_start, want_runs = rle_oracle.encode(planes)
    cap = max(len(r) for r in want_runs) + 3 if cap is None else cap
    labelled = [oracle.label(want_start[n], want_runs[n], H, W, connectivity) for n in range(N)]
    rcap = max(l[0] for l in labelled) + 2 if rcap is None else rcap
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    runs = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    ops.labels_rle(torch.from_numpy(planes).to(dev), row_start, runs)
    n_back = _guarded(dev, N + EXTRA, G32, np.int32)
    rr_back = _guarded(dev, N * cap + EXTRA, G32, np.int32)
    rec_back = _guarded(dev, (N * rcap + EXTRA) * 8, G64, np.int64)
    regions = rec_back[:N * rcap * 8].view(N, rcap, 8) if with_regions else None
    ops.rle_regions(row_start, runs, H, W, n_back[:N], rr_back[:N * cap].view(N, cap), regions, connectivity=connectivity)
    n_got, rr_got, rec_got = n_back.cpu().numpy(), rr_back.cpu().numpy(), rec_back.cpu().numpy()
    assert (n_got[N:] == G32).all() and (rr_got[N * cap:] == G32).all()
    rr_got, rec_all = rr_got[:N * cap].reshape(N, cap), rec_got[:N * rcap * 8].reshape(N, rcap, 8)
    if with_regions:
        assert (rec_got[N * rcap * 8:] == G64).all()
    else:
        assert (rec_got == G64).all()
    for n in range(N):
        R, rr, rec = oracle.expected(want_start[n], want_runs[n], cap, rcap, H, W, connectivity, np.full(cap, G32), np.full((rcap, 8), G64))
        assert n_got[n] == R, (n, int(n_got[n]), R)
        assert np.array_equal(rr_got[n], rr), n
        if with_regions:
            assert np.array_equal(rec_all[n], rec), n
    return n_got[:N], rr_got, rec_all if with_regions else None


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_hand_made_planes(dev, name, connectivity):
    """Against the oracle, and against the answers written out by hand."""
    plane = oracle.hand_plane(name)
    n_got, rr_got, rec_got = _run(dev, plane, connectivity)
    want_R, want_rr, want_rec = oracle.HAND[name][1][connectivity]
    assert n_got[0] == want_R and rec_got[0, :want_R].tolist() == [list(r) for r in want_rec]
    if not isinstance(want_rr, dict):
        assert rr_got[0, :len(want_rr)].tolist() == list(want_rr)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", rle_oracle.CASES, ids=rle_oracle.CASE_IDS)
def test_seeded_blob_planes(dev, case, connectivity):
    _run(dev, rle_oracle.build(case), connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_two_different_frames_do_not_leak(dev, connectivity):
    """N = 2 with frames of different sizes of problem in one call, in both orders: a frame's regions are those it has alone."""
    a, b = np.zeros((1, 21, 21), np.uint8), np.zeros((1, 21, 21), np.uint8)
    a[0] = oracle.HAND["spiral-21x21"][0]
    b[0, :6, :6] = oracle.HAND["checkerboard-6x6"][0]
    for pair in (np.concatenate([a, b]), np.concatenate([b, a])):
        n_got, rr_got, rec_got = _run(dev, pair, connectivity)
        for n in range(2):
            alone = _run(dev, pair[n:n + 1], connectivity, cap=rr_got.shape[1], rcap=rec_got.shape[1])
            assert n_got[n] == alone[0][0] and np.array_equal(rr_got[n], alone[1][0]) and np.array_equal(rec_got[n], alone[2][0])
    _run(dev, oracle.noise_planes(*oracle.NOISE), connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 1025])
def test_widths_around_a_wave_of_runs(dev, W, connectivity):
    """H = 3: up to a few hundred runs per row -- the lanes' stride of 64 over a row and both ends of the binary search in the row above.
    Row-noise planes (their middle row is one run: everything above meets it) and dense three-valued noise (every run has neighbours)."""
    _run(dev, oracle.noise_planes(300 + W, 2, 3, W), connectivity)
    _run(dev, oracle.dense_noise(400 + W, 2, 3, W), connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H", [1, 2, 257])
def test_heights(dev, H, connectivity):
    _run(dev, oracle.noise_planes(500 + H, 2, H, 16), connectivity)
    _run(dev, oracle.dense_noise(600 + H, 2, H, 16), connectivity)


@pytest.mark.parametrize("count", [255, 256, 257])
def test_scan_carry(dev, count):
    """Exactly 255, 256 and 257 runs (in 16 or 17 regions: sparse root flags) and exactly 255, 256 and 257 regions (in twice as many runs):
    the numbering works 256 runs at a time with a carry; and a frame with more than 256 regions among dense flags."""
    n_got, rr_got, _ = _run(dev, oracle.RUN_COUNT_PLANES[count], 8, cap=count)
    assert n_got[0] < 64
    n_got, _, _ = _run(dev, oracle.REGION_COUNT_PLANES[count], 4)
    assert n_got[0] == count
    n_got, _, _ = _run(dev, oracle.alternating(count), 8, cap=count)                            # one row: count runs, count regions
    assert n_got[0] == count
    assert _run(dev, oracle.dense_noise(3, 1, 24, 40), 4)[0][0] > 256


@pytest.mark.parametrize("connectivity", [4, 8])
def test_record_capacities(dev, connectivity):
    """rcap = R, R - 1, R // 2, 0 and regions=None (R: of the frame with most regions): n_regions and run_region stay exact, the records
    below min(R, rcap) are exact, the 0x5A rows from there on intact (_run checks all of it)."""
    planes = rle_oracle.build(rle_oracle.CASES[1])
    R = max(l[0] for l in oracle.label_planes(planes, connectivity))
    assert min(l[0] for l in oracle.label_planes(planes, connectivity)) < R
    for rcap in (R, R - 1, R // 2, 0):
        n_got, _, _ = _run(dev, planes, connectivity, rcap=rcap)
        assert [int(k) > rcap for k in n_got] == [l[0] > rcap for l in oracle.label_planes(planes, connectivity)]
    _run(dev, planes, connectivity, with_regions=False)
    noise = oracle.noise_planes(*oracle.NOISE)
    _run(dev, noise, connectivity, rcap=100)
    _run(dev, noise, connectivity, with_regions=False)


def test_run_code_overflow(dev):
    """A run code made with cap = needed - 1 (needed: of the frame that needs most): that frame gets n_regions == -1 and its run_region and
    records stay fully intact; the other frames of the call are labelled as usual (_run checks both through oracle.expected)."""
    planes = rle_oracle.build(rle_oracle.CASES[1])
    need = [len(r) for r in rle_oracle.encode(planes)[1]]
    assert min(need) < max(need)
    n_got, rr_got, rec_got = _run(dev, planes, 8, cap=max(need) - 1)
    worst = int(np.argmax(need))
    assert n_got[worst] == -1 and (rr_got[worst] == G32).all() and (rec_got[worst] == G64).all()
    assert all(n_got[n] > 0 for n in range(len(need)) if n != worst)
    n_got, _, _ = _run(dev, planes, 4, cap=min(need))
    assert sorted(n_got.tolist())[:2] == [-1, -1] and n_got.max() > 0


def test_own_workspace_and_bit_equality(dev):
    """Two runs of the same call are bit-equal (integer atomics); a caller's workspace of exactly the size asked for serves, with guards
    behind it."""
    from arseg_amd import _lib, ops

    planes = np.concatenate([oracle.noise_planes(*oracle.NOISE), oracle.dense_noise(9, 1, 12, 65)])
    first = _run(dev, planes, 8)
    second = _run(dev, planes, 8)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    N, H, W = planes.shape
    cap, rcap = first[1].shape[1], first[2].shape[1]
    nbytes = _lib.load().arseg_rle_regions_workspace_bytes(N, cap)
    assert nbytes == 4 * N * cap
    ws_back = _guarded(dev, nbytes // 4 + EXTRA, G32, np.int32)
    row_start = torch.empty((N, H + 1), dtype=torch.int32, device=dev)
    runs = torch.empty((N, cap), dtype=torch.int32, device=dev)
    ops.labels_rle(torch.from_numpy(planes).to(dev), row_start, runs)
    n_regions, run_region = torch.empty((N,), dtype=torch.int32, device=dev), torch.full((N, cap), int(G32), dtype=torch.int32, device=dev)
    regions = torch.full((N, rcap, 8), int(G64), dtype=torch.int64, device=dev)
    ops.rle_regions(row_start, runs, H, W, n_regions, run_region, regions, connectivity=8, workspace=ws_back[:nbytes // 4])
    assert np.array_equal(n_regions.cpu().numpy(), first[0]) and np.array_equal(run_region.cpu().numpy(), first[1])
    assert np.array_equal(regions.cpu().numpy(), first[2]) and (ws_back[nbytes // 4:].cpu().numpy() == G32).all()
    with pytest.raises(_lib.ArsegError):
        ops.rle_regions(row_start, runs, H, W, n_regions, run_region, regions, workspace=ws_back[:nbytes // 4 - 1])


def _check_frames(found, pred, connectivity, lut=None):
    """A RegionFrames against the oracle applied to the label planes ``pred`` [N,H,W]."""
    import test_regions

    planes = (pred if lut is None else lut[pred]).astype(np.uint8)
    N, H, W = planes.shape
    want = oracle.label_planes(planes, connectivity)
    assert found.needed().cpu().tolist() == [w[0] for w in want]
    rr = found.run_region.cpu().numpy()
    host = found.to_host()
    for n, (R, want_rr, rows) in enumerate(want):
        assert np.array_equal(rr[n, :len(want_rr)], want_rr)
        assert np.array_equal(found.records[n, :R].cpu().numpy(), rows)
        test_regions._same_records(host[n], rows)
    return want


@pytest.mark.parametrize("case", [consistency_oracle.CASES[0], consistency_oracle.CASES[1]], ids=lambda c: c[0])
def test_full_chain_from_logits(dev, case):
    """egress.regions(egress.rle(logits, ...)) on the same-size and the bilinear route equals the oracle applied to ops.argmax_confusion's
    pred, at both connectivities and with a lut; regions_numpy gives the same records from the run code brought to the host."""
    import test_regions
    from arseg_amd import egress, ops

    _, _, N, n_cls, h, w, H, W, align, _ = case
    logits = torch.from_numpy(consistency_oracle.build(case)["logits"]).to(dev)
    pred = ops.argmax_confusion(logits, None, H, W, align_corners=align)[0].cpu().numpy()
    frames = egress.rle(logits, H, W, H * W, align_corners=align)
    for connectivity in (4, 8):
        found = egress.regions(frames, 512, connectivity=connectivity)
        assert isinstance(found, egress.RegionFrames) and found.frames is frames and found.capacity == 512
        want = _check_frames(found, pred, connectivity)
        for n, (rs, words) in enumerate(frames.to_host()):
            test_regions._same_records(egress.regions_numpy(rs, words, H, W, connectivity), want[n][2])
    lut = np.random.Generator(np.random.PCG64(2)).integers(0, 256, n_cls, dtype=np.uint8)
    mapped = egress.rle(logits, H, W, H * W, lut=lut, align_corners=align)
    _check_frames(egress.regions(mapped, 512), pred, 8, lut=lut)
    big = int(np.median(want[0][2][:, 1]))
    kept = egress.regions(frames, 512).to_host(min_area=big)[0]
    assert 0 < len(kept) < want[0][0] and (kept["area"] >= big).all()


def test_chain_in_one_graph(dev):
    """labels8 + encode + regions captured once (every buffer given: nothing is allocated); the logits are refilled in place; each replay
    equals the oracle for its own logits, and the two replays have different numbers of regions."""
    from arseg_amd import egress, ops

    case = consistency_oracle.CASES[4]
    _, seed, N, n_cls, h, w, H, W, align, _ = case
    logits = torch.from_numpy(consistency_oracle.build(case)["logits"]).to(dev)
    cap, rcap = H * W // 2, 256
    labels = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    coded = egress.RleFrames(torch.zeros((N, H + 1), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev), H, W)
    found = egress.RegionFrames(torch.zeros((N,), dtype=torch.int32, device=dev), torch.zeros((N, cap), dtype=torch.int32, device=dev),
                                torch.zeros((N, rcap, 8), dtype=torch.int64, device=dev), coded, 8,
                                torch.zeros((N, cap), dtype=torch.int32, device=dev))

    def chain():
        egress.regions(egress.rle(logits, H, W, cap, labels_out=labels, out=coded, align_corners=align), rcap, out=found)

    chain()                                                                                     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    totals = []
    for s in (seed + 60, seed + 61):
        fresh = torch.from_numpy(consistency_oracle.build((case[0], s) + case[2:])["logits"]).to(dev)
        logits.copy_(fresh)
        labels.zero_()
        coded.row_start.fill_(-7)
        coded.runs.fill_(-1)
        found.n_regions.fill_(-7)
        found.run_region.fill_(-7)
        found.records.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        pred = ops.argmax_confusion(fresh, None, H, W, align_corners=align)[0].cpu().numpy()
        want = _check_frames(found, pred, 8)
        totals.append(sum(w[0] for w in want))
    assert totals[0] != totals[1]


def test_alter_res_batch_regions(dev, manifest):
    """The small PSPNet (fp32) of tests/test_gpu_models.py: alter_res_batch_regions' regions are the oracle's on alter_res_batch_render's
    planes."""
    import test_gpu_ingest_formats as tf
    from arseg_amd import egress, synth
    from arseg_amd import evaluation as ev

    hr, lr = tf._nets(manifest, dev, "psp")
    H, W, gop = 64, 96, 4
    clip = synth.make_clip(9, H, W, gop=gop, mean=synth.CAMVID_MEAN, std=synth.CAMVID_STD)
    frames = torch.from_numpy(clip["frames"]).to(dev)
    mvs = torch.from_numpy(clip["mv"][1:gop]).to(dev)
    with torch.no_grad():
        _, feat_k = hr.forward_keyframe(frames[0:1])
        refs = [feat_k[0]] * (gop - 1)
        labels_r, _ = ev.alter_res_batch_render(lr, refs, frames[1:gop], mvs, 0.5)
        found, labels = ev.alter_res_batch_regions(lr, refs, frames[1:gop], mvs, H * W, H * W // 4, 0.5)
    assert isinstance(found, egress.RegionFrames) and torch.equal(labels, labels_r) and torch.equal(found.frames.decode(), labels_r)
    want = _check_frames(found, labels_r.cpu().numpy(), 8)
    print(f"\nregions per frame {[w[0] for w in want]}, runs per frame {found.frames.needed().cpu().tolist()}")


def test_full_size_frame(dev):
    """One 1024x2048 frame of blob-like labels (19 classes): tens of thousands of runs over more than 256 workgroups of rows, a background of
    hundreds of runs.  The oracle's time follows the run count, which is kept in check here."""
    planes = rle_oracle.blob_planes(77, 1, 1024, 2048)
    needed = int(rle_oracle.encode(planes)[0][0, -1])
    assert 1024 < needed < 100000
    n_got, rr_got, _ = _run(dev, planes, 8)
    assert np.bincount(rr_got[0, :needed]).max() > 256 and n_got[0] > 256
