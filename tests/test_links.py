"""CPU checks of the links between the regions of two frames (include/arseg_hip.h, arseg_region_links_fwd; arseg_amd.egress.links): the oracle
against answers written out by hand, the pure-numpy host form against the oracle, the invariants of the records, LinkFrames' host side,
TrackIds on a scripted sequence, the wrappers' refusals, every ARSEG_EINVAL / ARSEG_EWORKSPACE case through ctypes (the library loads
without a GPU), and the spread of the inputs the GPU tests use.  Everything is an integer: every comparison is np.array_equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import links_oracle as oracle
import regions_oracle
import rle_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(rec, fields):
    return np.stack([rec[f] for f in fields], axis=1) if len(rec) else np.zeros((0, len(fields)), np.int64)


@pytest.mark.parametrize("name", oracle.HAND_IDS)
def test_oracle_against_the_literals(name):
    cur, ref, mv_q, answers = oracle.HAND[name]
    got = oracle.link_planes(cur, ref, mv_q)
    assert len(got) == len(answers) == cur.shape[0]
    for (n_pairs, links, back), (want_pairs, want_links, want_back) in zip(got, answers):
        assert n_pairs == want_pairs and links.tolist() == [list(r) for r in want_links] and back.tolist() == [list(r) for r in want_back]


def test_the_literals_say_what_they_should():
    by = oracle.HAND
    assert by["identity"][2] is None and np.array_equal(by["identity"][0], by["identity"][1])
    assert by["translation"][2][0, 0, 0].tolist() == [12, -8]                                   # (+3, -2) pixels
    split, merge = by["split"][3][0], by["merge"][3][0]
    assert split[1][1][0] == split[1][3][0] == 1 and split[2][1][0] == 1                        # both halves link to k = 1, which keeps r = 1
    assert [row[4] for row in split[1]] == [1, 1, 0, 0]                                         # exactly one half is mutual
    assert merge[1][1][5] == 2 and merge[1][1][0] == 1                                          # n_ref == 2, the smaller k
    assert by["class-change"][3][0][1][1][0] == -1 and by["class-change"][3][0][1][1][2] == 0
    assert by["reference-tie"][3][0][1][0][:2] == (0, 2)
    assert by["rounding"][2][0, 0, :5, 0].tolist() == [2, 6, -2, -6, 10]
    wide = by["wave-boundary"][0][0, 0]
    assert wide[63] == wide[64] == 2 and wide[59] == 1 and wide[70] == 1 and wide[127] == wide[128] == 1
    assert by["shared-reference"][1].shape[0] == 1 and by["per-frame-references"][1].shape[0] == 2
    assert not np.array_equal(by["per-frame-references"][1][0], by["per-frame-references"][1][1])


def _numpy_form(cur, ref, mv_q):
    """egress.links_numpy per frame on the oracle's run codes, with buffers longer than needed -> [(links rows, back rows)]."""
    from arseg_amd import egress

    N, H, W = cur.shape
    a, b = oracle.device_inputs(cur), oracle.device_inputs(ref)
    out = []
    for n in range(N):
        m = n if ref.shape[0] > 1 else 0
        links, back = egress.links_numpy(a[0][n], a[1][n].view(np.int32), a[3][n], b[0][m], b[1][m], b[3][m], H, W, None if mv_q is None else mv_q[n])
        assert links.dtype.names == oracle.LINK_FIELDS and back.dtype.names == oracle.BACK_FIELDS
        out.append((_rows(links, oracle.LINK_FIELDS), _rows(back, oracle.BACK_FIELDS)))
    return out


def _inputs():
    """(cur, ref, mv_q) triples: the hand-made cases, blob planes with block motion (shared and per-frame references), the edge shapes and
    the dense noise of the GPU tests."""
    for name in oracle.HAND_IDS:
        yield oracle.HAND[name][:3]
    for case in rle_oracle.CASES:
        planes = rle_oracle.build(case)
        N, H, W = planes.shape
        yield planes, np.roll(planes, 1, axis=0), oracle.block_motion(case[1], N, H, W, amp=5)
        yield planes, planes[:1], oracle.block_motion(case[1] + 1, N, H, W, amp=2)
        yield planes, planes[:1], None
    for H, W in oracle.EDGE_SHAPES:
        cur, ref = regions_oracle.noise_planes(700 + H * W, 2, H, W), regions_oracle.noise_planes(750 + H * W, 2, H, W)
        yield cur, ref, oracle.block_motion(700 + W, 2, H, W, block=4)
    seed, N, H, W = oracle.DENSE
    yield regions_oracle.dense_noise(seed, N, H, W), regions_oracle.dense_noise(seed + 1, N, H, W), oracle.block_motion(seed + 2, N, H, W, amp=3)


def test_links_numpy_against_the_oracle_and_invariants():
    from arseg_amd import egress

    linked = 0
    for cur, ref, mv_q in _inputs():
        want = oracle.link_planes(cur, ref, mv_q)
        sides = oracle.region_planes(cur)
        for n, ((links, back), (n_pairs, want_links, want_back)) in enumerate(zip(_numpy_form(cur, ref, mv_q), want)):
            assert np.array_equal(links, want_links) and np.array_equal(back, want_back)
            area = np.bincount(sides[n]["reg"].ravel(), minlength=len(links))
            assert links[:, 2].sum() == back[:, 2].sum()                                        # sum(same) == sum(covered)
            assert (links[:, 2] + links[:, 3] <= area).all()                                    # same + outside <= area
            assert links[:, 5].sum() == back[:, 3].sum() == n_pairs
            mutual = np.flatnonzero(links[:, 4] == 1)
            assert np.array_equal(back[links[mutual, 0], 0], mutual)                            # mutual is symmetric
            ks = np.flatnonzero(back[:, 0] >= 0)
            assert np.array_equal(np.sort(links[mutual, 0]), ks[links[back[ks, 0], 0] == ks])           # ... from the reference's side too
            linked += len(mutual)
    assert linked > 100
    a = oracle.device_inputs(oracle.HAND["split"][0])
    with pytest.raises(ValueError):
        egress.links_numpy(a[0][0], a[1][0], a[3][0], a[0][0], a[1][0], a[3][0], 3, 8, np.zeros((3, 8, 2), np.float32))
    with pytest.raises(ValueError):
        egress.links_numpy(a[0][0], a[1][0], a[3][0][:2], a[0][0], a[1][0], a[3][0], 3, 8)
    with pytest.raises(ValueError):
        egress.links_numpy(a[0][0][:-1], a[1][0], a[3][0], a[0][0], a[1][0], a[3][0], 3, 8)


def test_inputs_are_spread():
    """So that the GPU tests cannot pass vacuously: the dense noise has more than 256 distinct pairs in both frames, in different numbers,
    with regions that are mutual, regions with several reference regions and pixels off the frame; the edge shapes have blocks whose
    targets all leave the frame; the blob planes of the unlinkable-frame test need different numbers of runs."""
    seed, N, H, W = oracle.DENSE
    want = oracle.link_planes(regions_oracle.dense_noise(seed, N, H, W), regions_oracle.dense_noise(seed + 1, N, H, W),
                              oracle.block_motion(seed + 2, N, H, W, amp=3))
    assert min(w[0] for w in want) > 256 and want[0][0] != want[1][0]
    for n_pairs, links, back in want:
        assert (links[:, 4] == 1).sum() > 10 and (links[:, 5] > 1).sum() > 10 and links[:, 3].sum() > 0 and (links[:, 0] < 0).sum() > 0
    mv_q = oracle.block_motion(700 + 129, 2, 3, 129, block=4)
    gone = np.abs(mv_q[..., 1].astype(np.int64)) >= 4 * 3
    assert gone.all(axis=1).any() and not gone.all()                                           # whole block columns, not every one
    need = [len(r) for r in rle_oracle.encode(rle_oracle.build(rle_oracle.CASES[1]))[1]]
    assert len(set(need)) == 3


def _cpu_link_frames(cur, ref, mv_q, capacity=None, ref_capacity=None, pair_capacity=4096, run_cap=None):
    """LinkFrames on CPU tensors, filled by the oracle as the device would fill them."""
    from arseg_amd import egress

    N, H, W = cur.shape
    want = oracle.link_planes(cur, ref, mv_q)
    sides = []
    for planes, rec_cap, cap in ((cur, capacity, run_cap), (ref, ref_capacity, None)):
        row_start, runs, n_regions, run_region = oracle.device_inputs(planes, cap)
        rec_cap = int(n_regions.max()) + 2 if rec_cap is None else rec_cap
        frames = egress.RleFrames(torch.from_numpy(row_start), torch.from_numpy(runs.view(np.int32)), H, W)
        sides.append(egress.RegionFrames(torch.from_numpy(n_regions), torch.from_numpy(run_region),
                                         torch.zeros((planes.shape[0], rec_cap, 8), dtype=torch.int64), frames))
    a, b = sides
    n_pairs = np.zeros(N, np.int32)
    links, back = np.full((N, a.capacity, 6), -9, np.int64), np.full((N, b.capacity, 4), -9, np.int64)
    for n in range(N):
        m = n if b.N > 1 else 0
        linkable = int(a.n_regions[n]) >= 0 and int(b.n_regions[m]) >= 0
        n_pairs[n], links[n], back[n] = oracle.expected(want[n], linkable, a.capacity, b.capacity, pair_capacity, links[n], back[n])
    return egress.LinkFrames(torch.from_numpy(n_pairs), torch.from_numpy(links), torch.from_numpy(back), a, b, pair_capacity), want


def test_link_frames_to_host_on_cpu_tensors():
    from arseg_amd import _lib, egress

    planes = rle_oracle.build(rle_oracle.CASES[1])
    N, H, W = planes.shape
    ref, mv_q = planes[:1], oracle.block_motion(3, N, H, W, amp=3)
    found, want = _cpu_link_frames(planes, ref, mv_q)
    assert found.N == 3 and found.needed().tolist() == [w[0] for w in want] and min(w[0] for w in want) > 0
    host = found.to_host()
    assert len(host) == 3
    for (links, back), (n_pairs, want_links, want_back) in zip(host, want):
        assert links.dtype.names == oracle.LINK_FIELDS and back.dtype.names == oracle.BACK_FIELDS and links["overlap"].dtype == np.int64
        assert np.array_equal(_rows(links, oracle.LINK_FIELDS), want_links) and np.array_equal(_rows(back, oracle.BACK_FIELDS), want_back)
    # a frame whose run code overflowed: -1, the frame is named
    need = [len(r) for r in rle_oracle.encode(planes)[1]]
    worst = int(np.argmax(need))
    cut, _ = _cpu_link_frames(planes, ref, mv_q, run_cap=max(need) - 1, capacity=20)
    assert cut.needed().tolist()[worst] == -1
    with pytest.raises(_lib.ArsegError) as e:
        cut.to_host()
    assert f"frame {worst}" in str(e.value) and "overflowed" in str(e.value)
    # more pairs than the table holds: -2, the frame and the capacity
    most = int(np.argmax([w[0] for w in want]))
    small = max(w[0] for w in want) - 1
    full, _ = _cpu_link_frames(planes, ref, mv_q, pair_capacity=small)
    assert full.needed().tolist()[most] == -2
    with pytest.raises(_lib.ArsegError) as e:
        full.to_host()
    assert f"frame {most}" in str(e.value) and str(small) in str(e.value) and "pair" in str(e.value)
    # more regions than records, on either side
    R = [len(w[1]) for w in want]
    short, _ = _cpu_link_frames(planes, ref, mv_q, capacity=max(R) - 1)
    with pytest.raises(_lib.ArsegError) as e:
        short.to_host()
    assert f"frame {int(np.argmax(R))}" in str(e.value) and str(max(R)) in str(e.value) and str(max(R) - 1) in str(e.value)
    K = len(want[0][2])
    short, _ = _cpu_link_frames(planes, ref, mv_q, ref_capacity=K - 1)
    with pytest.raises(_lib.ArsegError) as e:
        short.to_host()
    assert "reference" in str(e.value) and str(K) in str(e.value) and str(K - 1) in str(e.value)
    exact, _ = _cpu_link_frames(planes, ref, mv_q, capacity=max(R), ref_capacity=K)             # needed == capacity is no overflow
    assert np.array_equal(_rows(exact.to_host()[1][0], oracle.LINK_FIELDS), want[1][1])
    with pytest.raises(ValueError):
        egress.LinkFrames(found.n_pairs[:2], found.links, found.back, found.cur, found.ref, 16)
    with pytest.raises(ValueError):
        egress.LinkFrames(found.n_pairs, found.links, found.back, found.cur, found.cur.frames, 16)


def _links_of(rows):
    from arseg_amd import egress

    return egress._records_of(np.array(rows, dtype=np.int64).reshape(-1, 6), egress.LINK_DTYPE)


def test_track_ids_on_a_scripted_sequence():
    """keyframe (3 regions) -> a split of region 1 -> a merge of regions 0 and 1 -> the next keyframe, whose links (made against the frame
    before it with zero motion) carry the ids over the GOP boundary.  Only ref_region and mutual matter."""
    from arseg_amd import egress

    t = egress.TrackIds()
    with pytest.raises(ValueError):
        t.frame(_links_of([(0, 1, 1, 0, 1, 1)]))
    assert t.keyframe(3).tolist() == [0, 1, 2]
    # split: keyframe region 1 falls into regions 1 and 2; the larger one keeps the id, the other is new with parent 1; region 4 is new
    ids, parents = t.frame(_links_of([(0, 9, 9, 0, 1, 1), (1, 5, 5, 0, 1, 1), (1, 3, 3, 0, 0, 1), (2, 7, 7, 0, 1, 1), (-1, 0, 0, 0, 0, 0)]))
    assert ids.tolist() == [0, 1, 3, 2, 4] and parents.tolist() == [-1, -1, 1, -1, -1]
    # merge: keyframe regions 0 and 1 under one region, which came mostly from 0 and is its largest part; 2 goes on
    ids, parents = t.frame(_links_of([(0, 9, 14, 0, 1, 2), (2, 7, 7, 0, 1, 1)]))
    assert ids.tolist() == [0, 2] and parents.tolist() == [-1, -1]
    # the next keyframe against that last frame (ids 0 and 2): two regions go on, one is born from id 2, one from nothing
    assert t.keyframe(4, _links_of([(1, 6, 6, 0, 1, 1), (0, 9, 9, 0, 1, 1), (1, 2, 2, 0, 0, 1), (-1, 0, 0, 0, 0, 0)])).tolist() == [2, 0, 5, 6]
    ids, parents = t.frame(_links_of([(3, 4, 4, 0, 1, 1), (2, 1, 1, 0, 0, 1)]))
    assert ids.tolist() == [6, 7] and parents.tolist() == [-1, 5]
    assert t.keyframe(2).tolist() == [8, 9]                                                     # without links: all fresh
    with pytest.raises(ValueError):
        t.keyframe(3, _links_of([(0, 1, 1, 0, 1, 1)]))
    with pytest.raises(ValueError):
        t.frame(_links_of([(2, 1, 1, 0, 1, 1)]))                                                # the keyframe has two regions
    with pytest.raises(ValueError):
        egress.TrackIds().keyframe(1, _links_of([(0, 1, 1, 0, 1, 1)]))


def test_host_layer_argument_checks():
    """The wrappers refuse CPU tensors (there is no fallback: links_numpy is the host form) and malformed arguments before any ABI call."""
    from arseg_amd import _lib, egress, ops

    row_start, runs = torch.zeros((2, 5), dtype=torch.int32), torch.zeros((2, 16), dtype=torch.int32)
    n_regions, run_region, n_pairs = torch.zeros((2,), dtype=torch.int32), torch.zeros((2, 16), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    side = (row_start, runs, n_regions, run_region)
    with pytest.raises(_lib.ArsegError):
        ops.region_links(*side, *side, 4, 8, n_pairs)
    with pytest.raises(ValueError):
        ops.region_links(*side, *side, 4, (1 << 24) + 1, n_pairs)
    with pytest.raises(ValueError):
        ops.region_links(*side, *side, 0, 8, n_pairs)
    frames = egress.RleFrames(row_start, runs, 4, 8)
    found = egress.RegionFrames(n_regions, run_region, torch.zeros((2, 4, 8), dtype=torch.int64), frames)
    with pytest.raises(_lib.ArsegError):
        egress.links(found, found)
    with pytest.raises(ValueError):
        egress.links(found, found, pair_capacity=0)
    with pytest.raises(ValueError):
        egress.links(found, frames)
    with pytest.raises(ValueError):
        egress.links(found, found, out=found)
    other = egress.RegionFrames(torch.zeros((3,), dtype=torch.int32), torch.zeros((3, 16), dtype=torch.int32),
                                torch.zeros((3, 4, 8), dtype=torch.int64),
                                egress.RleFrames(torch.zeros((3, 5), dtype=torch.int32), torch.zeros((3, 16), dtype=torch.int32), 4, 8))
    with pytest.raises(ValueError):
        egress.links(found, other)                                                              # one reference frame or N
    taller = egress.RegionFrames(n_regions, run_region, torch.zeros((2, 4, 8), dtype=torch.int64),
                                 egress.RleFrames(torch.zeros((2, 6), dtype=torch.int32), runs, 5, 8))
    with pytest.raises(ValueError):
        egress.links(found, taller)


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, egress, evaluation, ops

    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arseg_hip.h")).read(), flags=re.S)
    for name in ("arseg_region_links_fwd", "arseg_region_links_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
    declared = re.search(r"arseg_region_links_fwd\s*\((.*?)\)", text, flags=re.S).group(1)
    assert len(declared.split(",")) == len(_lib.PROTOTYPES["arseg_region_links_fwd"][1]) == 24
    assert lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.region_links) and callable(evaluation.alter_res_batch_links) and callable(egress.links) and callable(egress.links_numpy)
    assert egress.LINK_DTYPE.names == oracle.LINK_FIELDS and egress.BACK_DTYPE.names == oracle.BACK_FIELDS


def test_workspace_bytes():
    """Two tables of pcap slots of 16 bytes and 8 bytes of flags per frame; nothing for sizes the entry point refuses; rising in both."""
    from arseg_amd import _lib

    f = _lib.load().arseg_region_links_workspace_bytes
    assert f(1, 1) == 40 and f(11, 40000) == 11 * (32 * 40000 + 8)
    assert f(3, 1 << 31) == 3 * (32 * (1 << 31) + 8)                                            # beyond 32 bits
    assert f(0, 100) == 0 and f(2, 0) == 0 and f(-1, 100) == 0 and f(2, -5) == 0
    sizes = [f(2, p) for p in (1, 2, 3, 64, 65, 1000)]
    assert sizes == sorted(set(sizes)) and all(s % 8 == 0 for s in sizes)
    assert [f(n, 10) for n in (1, 2, 3)] == [328, 656, 984]


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract and ARSEG_EWORKSPACE come back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    EINVAL = _lib.ARSEG_EINVAL
    N, pcap = 2, 100
    enough = N * (32 * pcap + 8)
    names = ("row_start", "runs", "n_regions", "run_region", "cap", "ref_row_start", "ref_runs", "ref_n_regions", "ref_run_region", "ref_cap",
             "ref_shared", "mv_q", "N", "H", "W", "n_pairs", "links", "rcap", "back", "kcap", "pcap", "workspace", "workspace_bytes")
    good = dict(zip(names, (one, one, one, one, 50, one, one, one, one, 60, 1, one, N, 8, 24, one, one, 10, one, 12, pcap, one, enough)))

    def call(**changed):
        return lib.arseg_region_links_fwd(*[dict(good, **changed)[k] for k in names], null)

    for name in ("row_start", "runs", "n_regions", "run_region", "ref_row_start", "ref_runs", "ref_n_regions", "ref_run_region", "n_pairs"):
        assert call(**{name: null}) == EINVAL                                                   # a null pointer
        for address in (65, 66, 67):
            assert call(**{name: ctypes.c_void_p(address)}) == EINVAL                           # not 4-byte aligned
    assert call(mv_q=ctypes.c_void_p(66)) == EINVAL
    for name in ("links", "back", "workspace"):                                                 # 8 bytes
        assert call(**{name: ctypes.c_void_p(68)}) == EINVAL and call(**{name: ctypes.c_void_p(65)}) == EINVAL
    for name in ("N", "H", "W", "cap", "ref_cap", "pcap"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(rcap=-1) == EINVAL and call(kcap=-1) == EINVAL
    assert call(links=null, rcap=1) == EINVAL and call(back=null, kcap=1) == EINVAL             # records wanted, nowhere to put them
    for shared in (-1, 2, 7):
        assert call(ref_shared=shared) == EINVAL
    assert call(H=1, W=(1 << 24) + 1) == EINVAL                                                 # x_first has 24 bits
    assert call(H=1 << 16, W=1 << 15) == EINVAL and call(H=46341, W=46341) == EINVAL            # H * W > INT32_MAX
    # the workspace: too small, by one byte and altogether; EINVAL wins over it
    assert call(workspace_bytes=enough - 1) == _lib.ARSEG_EWORKSPACE and call(workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace=null, workspace_bytes=0) == _lib.ARSEG_EWORKSPACE
    assert call(workspace_bytes=0, ref_shared=3) == EINVAL and call(workspace_bytes=0, pcap=0) == EINVAL
    assert call(workspace=null) == EINVAL                                                       # enough bytes claimed, no buffer
    assert lib.arseg_region_links_workspace_bytes(N, pcap) == enough
