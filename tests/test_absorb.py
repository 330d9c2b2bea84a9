"""CPU checks of the absorption of small regions (include/arseg_hip.h, arseg_rle_absorb_fwd; arseg_amd.egress.absorb): the oracle against
answers written out by hand, its invariants, the pure-numpy host form against the oracle, the bound on the neighbour pairs, the wrappers'
refusals and every ARSEG_EINVAL / ARSEG_EWORKSPACE case through ctypes (the library loads without a GPU).  Everything is an integer: every
comparison is np.array_equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import absorb_oracle as oracle
import regions_oracle
import rle_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDED = oracle.seeded_cases()
SEEDED_IDS = [c[0] for c in SEEDED]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_oracle_against_the_literals(name, connectivity):
    rows, options, want_rows, want_start, want_words, want_target, want_absorbed = oracle.HAND[name]
    got = oracle.absorb_plane(oracle.hand_plane(name), connectivity=connectivity, **options)
    assert got["plane"].tolist() == [list(r) for r in want_rows]
    assert got["row_start"].tolist() == want_start and got["runs"].tolist() == want_words
    assert got["target"].tolist() == want_target and got["n_absorbed"] == want_absorbed


def test_the_literals_say_what_they_should():
    by = oracle.HAND
    assert by["specks-into-background"][0] == by["protected-value-stays"][0] == [[0] * 8, [0, 9, 9, 4, 4, 9, 9, 0], [0] * 8]
    assert by["specks-into-background"][2] == [[0] * 8] * 3 and len(by["specks-into-background"][4]) == 3 and by["specks-into-background"][6] == 3
    assert by["protected-value-stays"][2][1] == [0, 0, 0, 4, 4, 0, 0, 0] and by["protected-value-stays"][1]["protect"] == {4}
    assert by["tie-to-the-smaller-index"][0] == [[1, 1, 1, 5, 2, 2, 2]] and by["tie-to-the-smaller-index"][2] == [[1, 1, 1, 1, 2, 2, 2]]
    assert by["row-merging"][0] == [[1, 1, 5, 1, 1]] and by["row-merging"][3] == [0, 1]                          # one run, from two regions of 1s
    assert regions_oracle.label_planes(oracle.hand_plane("row-merging")[None], 8)[0][0] == 3
    assert by["only-small-neighbours"][5] == [-2] * 4 and by["only-small-neighbours"][0] == by["only-small-neighbours"][2]
    assert by["min-area-1-is-the-identity"][0] == by["min-area-1-is-the-identity"][2] and by["min-area-1-is-the-identity"][1] == {"min_area": 1}


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", SEEDED, ids=SEEDED_IDS)
def test_oracle_invariants(case, connectivity):
    """The output has no more runs than the input; the pixels of stable regions are unchanged; a region with a target went into a stable
    neighbour; with nothing small the plane is identical; and the seeded inputs do absorb, leave alone and merge runs."""
    _, planes, min_area, protect = case
    absorbed = left_alone = merged = 0
    for plane in planes:
        got = oracle.absorb_plane(plane, min_area, protect, connectivity)
        side = got["side"]
        assert len(got["runs"]) <= len(side["runs"])
        stable = got["target"][side["reg"]] == -1
        assert np.array_equal(got["plane"][stable], plane[stable])
        assert np.array_equal(got["plane"][got["target"][side["reg"]] == -2], plane[got["target"][side["reg"]] == -2])
        went = got["target"][got["target"] >= 0]
        assert (got["target"][went] == -1).all()
        same = oracle.absorb_plane(plane, 1, None, connectivity)
        assert np.array_equal(same["plane"], plane) and (same["target"] == -1).all() and same["n_absorbed"] == 0
        assert np.array_equal(same["runs"], side["runs"]) and np.array_equal(same["row_start"], side["row_start"])
        absorbed += got["n_absorbed"]
        left_alone += int((got["target"] == -2).sum())
        merged += len(side["runs"]) - len(got["runs"])
    assert absorbed > 0 and merged > 0
    if case[0].startswith("noise"):
        assert left_alone > 0


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_absorb_numpy_on_the_hand_cases(name, connectivity):
    from arseg_amd import egress

    plane = oracle.hand_plane(name)
    H, W = plane.shape
    options = oracle.HAND[name][1]
    row_start, runs = rle_oracle.encode(plane[None])
    got = egress.absorb_numpy(row_start[0], runs[0], H, W, connectivity=connectivity, **options)
    want = oracle.absorb_plane(plane, connectivity=connectivity, **options)
    for g, key, dtype in zip(got, ("row_start", "runs", "target"), (np.int32, np.uint32, np.int32)):
        assert g.dtype == dtype and np.array_equal(g, want[key]), key
    assert np.array_equal(egress.rle_decode_numpy(got[0], got[1], H, W), want["plane"])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", SEEDED, ids=SEEDED_IDS)
def test_absorb_numpy_on_seeded_planes_and_the_pair_bound(case, connectivity):
    """absorb_numpy equals the oracle; the distinct (small, stable) pairs stay below 3 x runs, the bound behind the default pair capacity."""
    from arseg_amd import egress

    _, planes, min_area, protect = case
    N, H, W = planes.shape
    row_start, runs = rle_oracle.encode(planes)
    for n in range(N):
        want = oracle.absorb_plane(planes[n], min_area, protect, connectivity)
        got = egress.absorb_numpy(row_start[n], runs[n], H, W, min_area, protect=protect, connectivity=connectivity)
        assert np.array_equal(got[0], want["row_start"]) and np.array_equal(got[1], want["runs"]) and np.array_equal(got[2], want["target"])
        assert 0 < want["pairs"] <= 3 * len(runs[n])
    table = np.zeros(256, dtype=bool)
    table[[0, 127]] = True
    a = egress.absorb_numpy(row_start[0], runs[0], H, W, min_area, protect=table, connectivity=connectivity)
    b = egress.absorb_numpy(row_start[0], runs[0], H, W, min_area, protect=[127, 0], connectivity=connectivity)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_absorb_numpy_refusals():
    from arseg_amd import egress

    row_start, runs = rle_oracle.encode(oracle.hand_plane("row-merging")[None])
    with pytest.raises(ValueError):
        egress.absorb_numpy(row_start[0], runs[0], 1, 5, 0)
    with pytest.raises(ValueError):
        egress.absorb_numpy(row_start[0], runs[0], 1, 5, 2, protect=[256])
    with pytest.raises(ValueError):
        egress.absorb_numpy(row_start[0], runs[0], 1, 5, 2, connectivity=6)
    with pytest.raises(ValueError):
        egress.absorb_numpy(row_start[0], runs[0], 2, 5, 2)


def test_wrappers_refuse_without_a_gpu():
    from arseg_amd import _lib, egress, ops

    rs, runs = torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32)
    frames = egress.RleFrames(rs, runs, 3, 8)
    found = egress.RegionFrames(torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32),
                                torch.zeros((1, 4, 8), dtype=torch.int64), frames)
    with pytest.raises(ValueError):
        egress.absorb(frames, 4)
    with pytest.raises(ValueError):
        egress.absorb(found, 4, pair_capacity=0)
    with pytest.raises(_lib.ArsegError):
        egress.absorb(found, 4)
    with pytest.raises(ValueError):
        egress.absorb(found, 4, out=frames)
    with pytest.raises(ValueError):
        ops.rle_absorb(rs, runs, found.n_regions, found.run_region, found.records, 3, 8, 0, rs, runs, found.n_regions)
    with pytest.raises(ValueError):
        egress.AbsorbedFrames(rs, runs, 3, 8, torch.zeros((1, 4), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32), found, 24)
    held = egress.AbsorbedFrames(rs, runs, 3, 8, torch.zeros((1, 4), dtype=torch.int32), torch.tensor([-2], dtype=torch.int32), found, 24)
    with pytest.raises(_lib.ArsegError, match="frame 0 .* pair capacity 24"):
        held.to_host()
    held.n_absorbed[0] = -1
    with pytest.raises(_lib.ArsegError, match="frame 0 could not be processed"):
        held.targets_to_host()


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, egress, evaluation, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arseg_hip.h")).read(), flags=re.S)
    for name in ("arseg_rle_absorb_fwd", "arseg_rle_absorb_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
        declared = re.search(r"%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["arseg_rle_absorb_fwd"][1]) == 22
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.rle_absorb) and callable(evaluation.alter_res_batch_absorb) and callable(egress.absorb) and callable(egress.absorb_numpy)


def test_workspace_bytes():
    """A table of pcap slots of 16 bytes, 8 bytes per region record and 8 bytes of flags per frame; nothing for sizes the entry point
    refuses; rising in pcap and rcap."""
    from arseg_amd import _lib

    f = _lib.load().arseg_rle_absorb_workspace_bytes
    assert f(1, 1, 0, 1, 1) == 24 and f(11, 40000, 5000, 1024, 120000) == 11 * (16 * 120000 + 8 * 5000 + 8)
    assert f(3, 1 << 31, 1 << 31, 7, 3 << 31) == 3 * (16 * (3 << 31) + 8 * (1 << 31) + 8)              # beyond 32 bits
    for bad in ((0, 10, 10, 10, 10), (-1, 10, 10, 10, 10), (2, 0, 10, 10, 10), (2, 10, -1, 10, 10), (2, 10, 10, 0, 10), (2, 10, 10, 10, 0)):
        assert f(*bad) == 0
    sizes = [f(2, 100, 10, 8, p) for p in (1, 2, 3, 64, 65, 1000)] + [f(2, 100, r, 8, 1000) for r in (11, 12, 500)]
    assert sizes == sorted(set(sizes)) and all(s % 8 == 0 for s in sizes)


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced; protect is a host table and stays NULL here)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    EINVAL = _lib.ARSEG_EINVAL
    N, cap, rcap, H, pcap = 2, 50, 10, 8, 100
    enough = N * (16 * pcap + 8 * rcap + 8)
    names = ("row_start", "runs", "n_regions", "run_region", "cap", "regions", "rcap", "N", "H", "W", "min_area", "protect", "out_row_start",
             "out_runs", "out_cap", "target", "tcap", "n_absorbed", "pcap", "workspace", "workspace_bytes")
    good = dict(zip(names, (one, one, one, one, cap, one, rcap, N, H, 24, 4, null, one, one, cap, one, rcap, one, pcap, one, enough)))

    def call(**changed):
        return lib.arseg_rle_absorb_fwd(*[dict(good, **changed)[k] for k in names], null)

    for name in ("row_start", "runs", "n_regions", "run_region", "regions", "out_row_start", "out_runs", "n_absorbed"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer
        for address in (65, 66, 67):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte (regions: 8-byte) aligned
    for address in (65, 66, 67):
        assert call(target=ctypes.c_void_p(address)) == EINVAL
    for name in ("regions", "workspace"):                                                       # 8 bytes
        assert call(**{name: ctypes.c_void_p(68)}) == EINVAL and call(**{name: ctypes.c_void_p(65)}) == EINVAL
    for name in ("N", "H", "W", "cap", "pcap", "out_cap"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(min_area=0) == EINVAL and call(min_area=-5) == EINVAL
    assert call(rcap=-1) == EINVAL and call(tcap=-1) == EINVAL
    assert call(target=null, tcap=1) == EINVAL                                                  # targets wanted, nowhere to put them
    assert call(H=1, W=(1 << 24) + 1) == EINVAL                                                 # x_first has 24 bits
    assert call(H=1 << 16, W=1 << 15) == EINVAL and call(H=46341, W=46341) == EINVAL            # H * W > INT32_MAX
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == _lib.ARSEG_EWORKSPACE and call(workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(target=null, tcap=0, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE                # target is optional
    assert call(workspace_bytes=0, min_area=0) == EINVAL and call(workspace_bytes=0, pcap=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    assert lib.arseg_rle_absorb_workspace_bytes(N, cap, rcap, H, pcap) == enough


def test_documented():
    """The header points from the regions' "Not covered" list to the new entry point; DESIGN.md, README.md and INTEGRATION.md describe it."""
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    assert "Removing or merging small regions:\n *   arseg_rle_absorb_fwd" in header and "pcap = 3 x cap can never give -2" in header
    assert "### 6.11" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("README.md", "INTEGRATION.md"):
        assert "absorb" in open(os.path.join(ROOT, name)).read(), name
