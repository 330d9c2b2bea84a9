"""CPU checks of the connected regions of a run code (include/arseg_hip.h, arseg_rle_regions_fwd; arseg_amd.egress.regions): the oracle
against answers written out by hand and against scipy, the pure-numpy receiving side against the oracle, RegionFrames' host side, the
wrappers' refusals, every ARSEG_EINVAL / ARSEG_EWORKSPACE case through ctypes (the library loads without a GPU), and the spread of the planes
the GPU tests use.  Everything is an integer: every comparison is np.array_equal."""
import ctypes

import numpy as np
import pytest
import torch

import regions_oracle as oracle
import rle_oracle

FIELDS = ("value", "area", "x_min", "y_min", "x_max", "y_max")


def _same_records(rec, rows):
    """A structured array of egress against the oracle's int64 [R,8] rows: the integers exactly, the centroids as the float64 quotients."""
    assert len(rec) == len(rows)
    for k, name in enumerate(FIELDS):
        assert np.array_equal(rec[name], rows[:, k]), name
    assert np.array_equal(rec["cx"], rows[:, 6] / rows[:, 1]) and np.array_equal(rec["cy"], rows[:, 7] / rows[:, 1])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_oracle_against_the_literals(name, connectivity):
    plane, answers = oracle.HAND[name]
    want_R, want_rr, want_rec = answers[connectivity]
    row_start, runs = rle_oracle.encode(plane[None])
    R, rr, rec = oracle.label(row_start[0], runs[0], plane.shape[0], plane.shape[1], connectivity)
    if isinstance(want_rr, dict):                                                               # the region of a run by its value
        want_rr = [want_rr[int(w) & 0xFF] for w in runs[0]]
    assert R == want_R and rr.tolist() == list(want_rr) and rec.tolist() == [list(r) for r in want_rec]


def test_the_literals_say_what_they_should():
    by = oracle.HAND
    assert by["checkerboard-6x6"][1][4][0] == 36 and by["checkerboard-6x6"][1][8][0] == 2
    assert by["corner-contact"][0].tolist() == [[1, 1, 0, 0], [0, 0, 1, 1]] and by["corner-contact"][1][4][0] == 4 and by["corner-contact"][1][8][0] == 2
    comb = by["comb-40-teeth"]
    assert comb[0].shape == (3, 81) and int((comb[0][0] == 5).sum()) == 40 and comb[1][4][1].count(1) == 81          # 2 x 40 teeth and the bottom row
    assert by["spiral-21x21"][0].shape == (21, 21) and by["u-shape"][1][4][1][2] == 0                                   # the right arm belongs to region 0
    rings = by["ring-in-ring"]
    assert rings[1][4][2][0][0] == rings[1][4][2][2][0] == 2 and rings[1][8][0] == 4                                    # one value, two regions
    assert by["one-row"][0].shape[0] == 1 and by["one-column"][0].shape[1] == 1
    inter = by["interleaved"][1][4][1]
    assert inter[:5] == [0, 1, 2, 3, 2]                                                         # the fifth run met is the third region


def _all_planes():
    planes = [oracle.hand_plane(n) for n in oracle.HAND_IDS] + [rle_oracle.build(c) for c in rle_oracle.CASES]
    return planes + [oracle.noise_planes(*oracle.NOISE), oracle.dense_noise(3, 1, 24, 40)] + list(oracle.RUN_COUNT_PLANES.values())


@pytest.mark.parametrize("connectivity", [4, 8])
def test_regions_numpy_against_the_oracle(connectivity):
    from arseg_amd import egress

    for planes in _all_planes():
        N, H, W = planes.shape
        row_start, runs = rle_oracle.encode(planes)
        for n in range(N):
            R, rr, rows = oracle.label(row_start[n], runs[n], H, W, connectivity)
            padded = np.concatenate([runs[n], np.full(3, rle_oracle.GUARD_WORD, np.uint32)]).view(np.int32)          # a buffer longer than needed
            rec, got_rr = egress.regions_numpy(row_start[n], padded, H, W, connectivity, return_run_region=True)
            assert got_rr.dtype == np.int32 and np.array_equal(got_rr, rr)
            _same_records(rec, rows)
            _same_records(egress.regions_numpy(row_start[n], runs[n], H, W, connectivity), rows)
    row_start, runs = rle_oracle.encode(oracle.hand_plane("u-shape"))
    with pytest.raises(ValueError):
        egress.regions_numpy(row_start[0], runs[0], 3, 3, connectivity=6)
    with pytest.raises(ValueError):
        egress.regions_numpy(row_start[0], runs[0][:-1], 3, 3)
    with pytest.raises(ValueError):
        egress.regions_numpy(row_start[0][:-1], runs[0], 3, 3)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_against_scipy(connectivity):
    """Region count and areas per value against scipy.ndimage.label on the pixels (an implementation that never sees a run)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    for planes in _all_planes():
        for n, (R, rr, rows) in enumerate(oracle.label_planes(planes, connectivity)):
            total = 0
            for v in np.unique(planes[n]):
                lab, k = ndimage.label(planes[n] == v, structure=structure)
                total += k
                assert sorted(np.bincount(lab.ravel())[1:].tolist()) == sorted(rows[rows[:, 0] == v, 1].tolist())
            assert total == R and rows[:, 1].sum() == planes[n].size


def test_inputs_are_spread():
    """So that the GPU tests cannot pass vacuously.  The seeded blob planes have 5, 5 and 12, 13, 11 regions, the same at either
    connectivity; so the suite also holds noise planes on which 8-connectivity joins what 4-connectivity does not, a frame with more than
    256 regions, and frames with more than 256 runs in fewer than 64 regions (the numbering scan's carry, dense and sparse flags)."""
    counts = []
    for case in rle_oracle.CASES:
        planes = rle_oracle.build(case)
        four, eight = oracle.label_planes(planes, 4), oracle.label_planes(planes, 8)
        assert [f[0] for f in four] == [e[0] for e in eight]
        counts += [f[0] for f in four]
        row_start, _ = rle_oracle.encode(planes)
        for n, (R, rr, rows) in enumerate(four):
            assert 118 <= row_start[n, -1] <= 306 and 31 <= np.bincount(rr).max() <= 110
    assert counts == [5, 5, 12, 13, 11]
    noise = oracle.noise_planes(*oracle.NOISE)
    for n in range(2):
        assert oracle.label_planes(noise, 8)[n][0] < oracle.label_planes(noise, 4)[n][0]
    assert oracle.label_planes(oracle.dense_noise(3, 1, 24, 40), 8)[0][0] < oracle.label_planes(oracle.dense_noise(3, 1, 24, 40), 4)[0][0]
    dense = oracle.label_planes(oracle.dense_noise(3, 1, 24, 40), 4)[0]
    assert dense[0] > 256
    for total, plane in oracle.RUN_COUNT_PLANES.items():
        R, rr, _ = oracle.label_planes(plane, 8)[0]
        assert len(rr) == total and R < 64
    for count, plane in oracle.REGION_COUNT_PLANES.items():
        R, rr, _ = oracle.label_planes(plane, 4)[0]
        assert R == count and len(rr) == 2 * count


def _cpu_region_frames(planes, connectivity, capacity, run_cap=None):
    """RegionFrames on CPU tensors, filled by the oracle."""
    from arseg_amd import egress

    N, H, W = planes.shape
    row_start, runs = rle_oracle.encode(planes)
    cap = max(len(r) for r in runs) + 2 if run_cap is None else run_cap
    words = np.full((N, cap), rle_oracle.GUARD_WORD, dtype=np.uint32)
    n_regions, run_region = np.zeros(N, np.int32), np.full((N, cap), -9, np.int32)
    records = np.full((N, capacity, 8), -9, np.int64)
    want = []
    for n in range(N):
        words[n, :min(cap, len(runs[n]))] = runs[n][:cap]
        n_regions[n], run_region[n], records[n] = oracle.expected(row_start[n], runs[n], cap, capacity, H, W, connectivity, run_region[n], records[n])
        want.append(oracle.label(row_start[n], runs[n], H, W, connectivity)[2])
    frames = egress.RleFrames(torch.from_numpy(row_start), torch.from_numpy(words.view(np.int32)), H, W)
    return egress.RegionFrames(torch.from_numpy(n_regions), torch.from_numpy(run_region), torch.from_numpy(records), frames, connectivity), want


def test_region_frames_to_host_on_cpu_tensors():
    from arseg_amd import _lib, egress

    planes = rle_oracle.build(rle_oracle.CASES[1])
    found, want = _cpu_region_frames(planes, 8, 20)
    assert found.N == 3 and found.capacity == 20 and found.needed().tolist() == [len(w) for w in want] == [12, 13, 11]
    host = found.to_host()
    assert len(host) == 3
    for rec, rows in zip(host, want):
        assert rec.dtype.names == FIELDS + ("cx", "cy") and rec["cx"].dtype == np.float64
        _same_records(rec, rows)
    # filters, on the host: the order stays
    rows = want[0]
    big = int(np.median(rows[:, 1]))
    _same_records(found.to_host(min_area=big)[0], rows[rows[:, 1] >= big])
    assert 0 < (rows[:, 1] >= big).sum() < len(rows)
    v = int(rows[0, 0])
    _same_records(found.to_host(values=v)[0], rows[rows[:, 0] == v])
    _same_records(found.to_host(values=[v, int(rows[1, 0])], min_area=2)[0], rows[np.isin(rows[:, 0], [v, rows[1, 0]]) & (rows[:, 1] >= 2)])
    # more regions than records: the frame, its need and the capacity
    short, _ = _cpu_region_frames(planes, 8, 12)
    with pytest.raises(_lib.ArsegError) as e:
        short.to_host()
    assert "frame 1" in str(e.value) and "13" in str(e.value) and "12" in str(e.value)
    exact, _ = _cpu_region_frames(planes, 8, 13)
    _same_records(exact.to_host()[1], want[1])                                                  # needed == capacity is no overflow
    # a frame whose run code overflowed has n_regions == -1: the frame, the runs it needs and the run capacity
    need = [int(k) for k in rle_oracle.encode(planes)[0][:, -1]]
    cut, _ = _cpu_region_frames(planes, 8, 20, run_cap=max(need) - 1)
    worst = int(np.argmax(need))
    assert cut.needed().tolist()[worst] == -1 and sorted(cut.needed().tolist())[1] > 0
    with pytest.raises(_lib.ArsegError) as e:
        cut.to_host()
    assert f"frame {worst}" in str(e.value) and str(max(need)) in str(e.value) and str(max(need) - 1) in str(e.value) and "run" in str(e.value)
    with pytest.raises(ValueError):
        egress.RegionFrames(found.n_regions[:2], found.run_region, found.records, found.frames)


def test_host_layer_argument_checks():
    """The wrappers refuse CPU tensors (there is no fallback: regions_numpy is the host form) and malformed arguments before any ABI call."""
    from arseg_amd import _lib, egress, ops

    row_start = torch.zeros((2, 5), dtype=torch.int32)
    runs = torch.zeros((2, 16), dtype=torch.int32)
    n_regions, run_region = torch.zeros((2,), dtype=torch.int32), torch.zeros((2, 16), dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):
        ops.rle_regions(row_start, runs, 4, 8, n_regions, run_region)
    with pytest.raises(ValueError):
        ops.rle_regions(row_start, runs, 4, 8, n_regions, run_region, connectivity=6)
    with pytest.raises(ValueError):
        ops.rle_regions(row_start, runs, 4, (1 << 24) + 1, n_regions, run_region)
    frames = egress.RleFrames(row_start, runs, 4, 8)
    with pytest.raises(_lib.ArsegError):
        egress.regions(frames, 8)
    with pytest.raises(ValueError):
        egress.regions(frames, -1)
    with pytest.raises(ValueError):
        egress.regions(frames, 8, connectivity=5)
    with pytest.raises(ValueError):
        egress.regions((row_start, runs), 8)
    with pytest.raises(ValueError):
        egress.regions(frames, 8, out=frames)


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, evaluation, ops

    lib = _lib.load()
    for name in ("arseg_rle_regions_fwd", "arseg_rle_regions_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.rle_regions) and callable(evaluation.alter_res_batch_regions)


def test_workspace_bytes():
    """One int32 parent per run slot; nothing for sizes the entry point refuses."""
    from arseg_amd import _lib

    lib = _lib.load()
    assert lib.arseg_rle_regions_workspace_bytes(1, 1) == 4
    assert lib.arseg_rle_regions_workspace_bytes(11, 10000) == 11 * 10000 * 4
    assert lib.arseg_rle_regions_workspace_bytes(3, 1 << 31) == 3 * (1 << 31) * 4             # beyond 32 bits
    assert lib.arseg_rle_regions_workspace_bytes(0, 100) == 0 and lib.arseg_rle_regions_workspace_bytes(2, 0) == 0
    assert lib.arseg_rle_regions_workspace_bytes(-1, 100) == 0 and lib.arseg_rle_regions_workspace_bytes(2, -5) == 0


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    EINVAL = _lib.ARSEG_EINVAL
    N, H, W, cap = 2, 8, 24, 100
    enough = N * cap * 4

    def call(row_start=one, runs=one, cap=cap, N=N, H=H, W=W, connectivity=8, n_regions=one, run_region=one, regions=one, rcap=10,
             workspace=one, workspace_bytes=enough):
        return lib.arseg_rle_regions_fwd(row_start, runs, cap, N, H, W, connectivity, n_regions, run_region, regions, rcap, workspace,
                                         workspace_bytes, null)

    for name in ("row_start", "runs", "n_regions", "run_region"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer
        for address in (65, 66, 67):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte aligned
    assert call(workspace=ctypes.c_void_p(66)) == EINVAL
    assert call(regions=ctypes.c_void_p(68)) == EINVAL and call(regions=ctypes.c_void_p(65)) == EINVAL          # regions: 8 bytes
    for name in ("N", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(cap=0) == EINVAL and call(cap=-1) == EINVAL
    assert call(rcap=-1) == EINVAL
    assert call(regions=null, rcap=1) == EINVAL                                                 # records wanted, nowhere to put them
    for connectivity in (0, 1, 6, -8, 16):
        assert call(connectivity=connectivity) == EINVAL
    big = (1 << 24) + 1
    assert call(H=1, W=big) == EINVAL                                                           # x_first has 24 bits
    assert call(H=1 << 16, W=1 << 15) == EINVAL and call(H=46341, W=46341) == EINVAL            # H * W > INT32_MAX
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == _lib.ARSEG_EWORKSPACE and call(workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace_bytes=0, connectivity=5) == EINVAL and call(workspace_bytes=0, cap=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    assert lib.arseg_rle_regions_workspace_bytes(N, cap) == enough
