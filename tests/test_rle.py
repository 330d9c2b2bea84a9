"""CPU checks of the run-length codes (include/arseg_hip.h, arseg_labels_rle_fwd / arseg_rle_decode_fwd; arseg_amd.egress.rle): the numpy
oracle's invariants, hand-made rows with their words written out, the pure-numpy receiving side, RleFrames' overflow logic, every
ARSEG_EINVAL case of both entry points through ctypes (the library loads without a GPU), and the spread of the seeded planes the GPU tests use."""
import ctypes

import numpy as np
import pytest
import torch

import rle_oracle as oracle


def _starts(runs):
    return (runs >> 8).astype(np.int64)


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_oracle_invariants(case):
    """decode(encode(p)) == p over any prefill; row_start is monotone from 0; a row's run count is 1 + its number of changes."""
    planes = oracle.build(case)
    N, H, W = planes.shape
    assert (N, H, W) == case[2:5] and planes.dtype == np.uint8
    row_start, runs = oracle.encode(planes)
    assert row_start.shape == (N, H + 1) and row_start.dtype == np.int32
    for n in range(N):
        assert row_start[n, 0] == 0 and (np.diff(row_start[n]) >= 1).all() and row_start[n, H] == len(runs[n]) and runs[n].dtype == np.uint32
        changes = (planes[n, :, 1:] != planes[n, :, :-1]).sum(axis=1)
        assert np.array_equal(np.diff(row_start[n]), 1 + changes)
        for fill in (0, 0xA5):
            assert np.array_equal(oracle.decode(row_start[n], runs[n], H, W, np.full((H, W), fill, np.uint8)), planes[n])
        assert (_starts(runs[n])[row_start[n, :-1]] == 0).all()                                  # every row begins with a run at x = 0


@pytest.mark.parametrize("hand", oracle.HAND, ids=oracle.HAND_IDS)
def test_hand_made_rows(hand):
    """The oracle gives the words written out by hand, and they decode to the plane."""
    _, rows, want_start, want_words = hand
    plane = oracle.hand_plane(hand)
    row_start, runs = oracle.encode(plane)
    assert row_start[0].tolist() == want_start and runs[0].tolist() == want_words
    H, W = plane.shape[1:]
    assert np.array_equal(oracle.decode(np.array(want_start), np.array(want_words, dtype=np.uint32), H, W, np.full((H, W), 0xA5, np.uint8)), plane[0])


def test_hand_made_rows_say_what_they_should():
    """The hand-made set holds what the contract's corner cases need (the literal words, not the oracle, are the reference here)."""
    by = {h[0]: h for h in oracle.HAND}
    assert len(by["constant"][3]) == 1
    alt = by["alternating-0-255"]
    assert len(alt[3]) == len(alt[1][0]) and {w & 0xFF for w in alt[3]} == {0, 255}              # W runs; the values 0 and 255
    for x in (15, 16, 17, 1024):
        assert by[f"boundary-at-{x}"][3][1] >> 8 == x
    nxt = by["row-ends-as-the-next-begins"]
    assert nxt[1][0][-1] == nxt[1][1][0] and nxt[3][2] == (0 << 8 | 8) and nxt[2] == [0, 2, 4, 5]  # a new run although the value goes on


def test_overflowed_decode_in_the_oracle():
    """cap below needed: the stored runs are decoded, a stored run whose successor in the row is cut off gives its first pixel, the rest
    keeps the prefill."""
    plane = np.array([[1, 1, 2, 2, 2, 3], [4, 4, 4, 4, 5, 5]], dtype=np.uint8)
    row_start, runs = oracle.encode(plane[None])
    assert row_start[0].tolist() == [0, 3, 5]
    pre = np.full((2, 6), 0xA5, np.uint8)
    A = 0xA5
    assert oracle.decode(row_start[0], runs[0][:5], 2, 6, pre).tolist() == plane.tolist()
    assert oracle.decode(row_start[0], runs[0][:4], 2, 6, pre).tolist() == [[1, 1, 2, 2, 2, 3], [4, A, A, A, A, A]]
    assert oracle.decode(row_start[0], runs[0][:3], 2, 6, pre).tolist() == [[1, 1, 2, 2, 2, 3], [A] * 6]
    assert oracle.decode(row_start[0], runs[0][:2], 2, 6, pre).tolist() == [[1, 1, 2, A, A, A], [A] * 6]
    assert oracle.decode(row_start[0], runs[0][:0], 2, 6, pre).tolist() == pre.tolist()


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_seeded_planes_are_spread(case):
    """So that the GPU tests cannot pass vacuously: per case the mean number of runs per row lies between 2 and W / 4, at least one row is
    a single run, at least one start lies on a multiple of 16 (beyond x = 0) and one on a multiple of 16 +- 1."""
    planes = oracle.build(case)
    N, H, W = planes.shape
    row_start, runs = oracle.encode(planes)
    per_row = np.concatenate([np.diff(r) for r in row_start])
    x = np.concatenate([_starts(r) for r in runs])
    print(f"\n{case[0]}: runs per row mean {per_row.mean():.2f} (min {per_row.min()}, max {per_row.max()}), single-run rows "
          f"{int((per_row == 1).sum())}, starts on 16k {int(((x > 0) & (x % 16 == 0)).sum())}, on 16k-1 {int((x % 16 == 15).sum())}, "
          f"on 16k+1 {int(((x > 1) & (x % 16 == 1)).sum())}, values {len(np.unique(planes))}")
    assert 2.0 <= per_row.mean() <= W / 4
    assert (per_row == 1).any()
    assert ((x > 0) & (x % 16 == 0)).any()
    assert (x % 16 == 15).any() or ((x > 1) & (x % 16 == 1)).any()
    assert 0 in planes and 255 in planes


def test_rle_decode_numpy_against_the_oracle():
    from arseg_amd import egress

    for planes in [oracle.build(c) for c in oracle.CASES] + [oracle.hand_plane(h) for h in oracle.HAND]:
        N, H, W = planes.shape
        row_start, runs = oracle.encode(planes)
        for n in range(N):
            assert np.array_equal(egress.rle_decode_numpy(row_start[n], runs[n], H, W), planes[n])
            padded = np.concatenate([runs[n], np.full(5, oracle.GUARD_WORD, np.uint32)])        # a buffer longer than needed
            assert np.array_equal(egress.rle_decode_numpy(row_start[n], padded.view(np.int32), H, W), planes[n])
    row_start, runs = oracle.encode(oracle.build(oracle.CASES[0]))
    H, W = oracle.CASES[0][3:5]
    with pytest.raises(ValueError):
        egress.rle_decode_numpy(row_start[0], runs[0][:-1], H, W)                                # fewer words than the frame needs
    with pytest.raises(ValueError):
        egress.rle_decode_numpy(row_start[0][:-1], runs[0], H, W)
    bad = runs[0].copy()
    bad[0] |= 3 << 8                                                                            # a row that does not begin at x = 0
    with pytest.raises(ValueError):
        egress.rle_decode_numpy(row_start[0], bad, H, W)


def test_rle_frames_to_host_and_overflow_on_cpu_tensors():
    """RleFrames' host side needs no GPU: two frames with different run counts come back cut to what each needs; a capacity below a
    frame's need raises ArsegError naming the frame and both numbers."""
    from arseg_amd import _lib, egress

    planes = oracle.build(oracle.CASES[0])
    N, H, W = planes.shape
    row_start, runs = oracle.encode(planes)
    need = [len(r) for r in runs]
    assert need[0] != need[1]
    cap = max(need) + 3
    buf = np.full((N, cap), oracle.GUARD_WORD, dtype=np.uint32)
    for n in range(N):
        buf[n, :need[n]] = runs[n]
    frames = egress.RleFrames(torch.from_numpy(row_start), torch.from_numpy(buf.view(np.int32)), H, W)
    assert (frames.N, frames.capacity, frames.H, frames.W) == (N, cap, H, W) and frames.needed().tolist() == need
    host = frames.to_host()
    assert len(host) == N
    for n, (rs, words) in enumerate(host):
        assert words.dtype == np.uint32 and np.array_equal(rs, row_start[n]) and np.array_equal(words, runs[n])
        assert np.array_equal(egress.rle_decode_numpy(rs, words, H, W), planes[n])
    worst = int(np.argmax(need))
    short = egress.RleFrames(torch.from_numpy(row_start), torch.from_numpy(buf.view(np.int32)[:, :max(need) - 1].copy()), H, W)
    with pytest.raises(_lib.ArsegError) as e:
        short.to_host()
    assert f"frame {worst}" in str(e.value) and str(max(need)) in str(e.value) and str(max(need) - 1) in str(e.value)
    exact = egress.RleFrames(torch.from_numpy(row_start), torch.from_numpy(buf.view(np.int32)[:, :max(need)].copy()), H, W)
    assert np.array_equal(exact.to_host()[worst][1], runs[worst])                               # needed == capacity is no overflow
    with pytest.raises(ValueError):
        egress.RleFrames(torch.from_numpy(row_start[:, :-1].copy()), torch.from_numpy(buf.view(np.int32)), H, W)


def test_host_layer_argument_checks():
    """The wrappers refuse CPU tensors (there is no fallback) and malformed capacities before any ABI call."""
    from arseg_amd import _lib, egress, ops

    plane = torch.zeros((2, 4, 8), dtype=torch.uint8)
    row_start = torch.zeros((2, 5), dtype=torch.int32)
    runs = torch.zeros((2, 16), dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):
        ops.labels_rle(plane, row_start, runs)
    with pytest.raises(_lib.ArsegError):
        ops.rle_decode(row_start, runs, plane)
    with pytest.raises(_lib.ArsegError):
        egress.rle_of_planes(plane, 16)
    with pytest.raises(ValueError):
        egress.rle_of_planes(plane, -1)
    with pytest.raises(ValueError):
        egress.rle_of_planes(plane[0], 16)


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib

    lib = _lib.load()
    for name in ("arseg_labels_rle_fwd", "arseg_rle_decode_fwd"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract, for both entry points, comes back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(66)
    EINVAL = _lib.ARSEG_EINVAL
    N, H, W = 2, 8, 24

    def enc(labels=one, pitch=W, ns=H * W, N=N, H=H, W=W, row_start=one, runs=one, cap=100):
        return lib.arseg_labels_rle_fwd(labels, pitch, ns, N, H, W, row_start, runs, cap, null)

    def dec(row_start=one, runs=one, cap=100, N=N, H=H, W=W, labels=one, pitch=W, ns=H * W):
        return lib.arseg_rle_decode_fwd(row_start, runs, cap, N, H, W, labels, pitch, ns, null)

    for fn in (enc, dec):
        assert fn(labels=null) == EINVAL and fn(row_start=null) == EINVAL                      # null plane / row_start
        assert fn(row_start=odd) == EINVAL and fn(runs=odd) == EINVAL                          # not 4-byte aligned
        assert fn(row_start=ctypes.c_void_p(65)) == EINVAL and fn(runs=ctypes.c_void_p(67)) == EINVAL
        assert fn(cap=-1) == EINVAL                                                            # cap < 0 with non-null runs
        for name in ("N", "H", "W"):
            assert fn(**{name: 0}) == EINVAL and fn(**{name: -3}) == EINVAL                    # a non-positive size
        assert fn(pitch=W - 1) == EINVAL and fn(ns=-1) == EINVAL                               # pitch < W, a negative stride
        big = (1 << 24) + 1
        assert fn(H=1, W=big, pitch=big) == EINVAL                                             # x_first has 24 bits
        assert fn(H=1 << 16, W=1 << 15, pitch=1 << 15) == EINVAL                               # H * W = 2^31 > INT32_MAX
        assert fn(H=46341, W=46341, pitch=46341) == EINVAL                                     # 46341^2 = 2^31 + 4633
    assert dec(runs=null) == EINVAL                                                            # the decoder needs runs
    assert enc(runs=null, cap=-1, labels=null) == EINVAL                                       # (the sizing pass ignores cap, not the rest)
    assert enc(runs=null, cap=-1, pitch=W - 1) == EINVAL
