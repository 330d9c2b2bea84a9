"""CPU-side checks of the two-list (B-frame) record chain: the oracle (tests/mv_brecords_oracle.py) against its hand-written literals,
ingest.chain_records_numpy against the oracle, the P-frame equivalence against oracle.cpu_ref.merge_motion, ingest.motion_vectors_to_records,
and the argument validation of the arseg_mv_records_bi_* entry points, which happens before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import mv_brecords_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = oracle.hand_cases()
SHAPES = [(24, 40), (37, 53), (8, 8)]


@pytest.mark.parametrize("case", HAND, ids=lambda c: c[0])
def test_oracle_equals_its_literals(case):
    _, max_ref, pushes, expected = case
    for policy in oracle.POLICIES:
        assert np.array_equal(oracle.chain(pushes, 8, 8, 4, max_ref, policy), oracle.hand_expected(expected[policy])), policy


def test_hand_cases_exercise_what_their_names_say():
    cases = {name: (pushes, exp) for name, _, pushes, exp in HAND}
    for name in ("bi block, list 0 back, list 1 forward, NEAR tie", "bi block, list 0 forward, list 1 back"):
        st = {}
        oracle.chain(cases[name][0], 8, 8, 4, 3, "near", st)
        assert st["both"] == 16 and st["near_tie"] == 16
        assert cases[name][1]["list0"] != cases[name][1]["mean"]
    assert cases["bi block, list 0 back, list 1 forward, NEAR tie"][1]["list0"] != cases["bi block, list 0 forward, list 1 back"][1]["list0"]
    exp = cases["two past references, NEAR takes list 1"][1]
    assert exp["list0"] != exp["near"] and exp["near"] != exp["mean"]
    st = {}
    oracle.chain(cases["MEAN with odd sums in both signs"][0], 8, 8, 4, 3, "mean", st)
    assert st["mean_half"] == 32                                       # both blocks of frame 3
    st = {}
    oracle.chain(cases["intra with a gap in D"][0], 8, 8, 4, 3, "list0", st)
    assert st["intra_gap"] == 48                                       # frame 3 outside its block, with p = 1; frame 2 has p = f - 1
    st = {}
    oracle.chain(cases["unusable winner over a usable lower index reads intra"][0], 8, 8, 4, 3, "list0", st)
    assert st["neither_under_winner"] == 10


@pytest.mark.parametrize("case", HAND, ids=lambda c: c[0])
def test_chain_records_numpy_on_the_hand_cases(case):
    from arseg_amd import ingest

    _, max_ref, pushes, expected = case
    for policy in oracle.POLICIES:
        got = ingest.chain_records_numpy(pushes, 8, 8, 4, max_ref, policy)
        assert got.dtype == np.int16 and got.shape == (4, 8, 8, 2)
        assert np.array_equal(got, oracle.hand_expected(expected[policy])), policy


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("order", oracle.ORDERS, ids=lambda o: "".join(map(str, o)))
@pytest.mark.parametrize("H,W", SHAPES)
def test_chain_records_numpy_on_generated_gops(H, W, order, max_ref):
    from arseg_amd import ingest

    for policy in oracle.POLICIES:
        pushes, want, _ = oracle.generated(H, W, order, max_ref, policy)
        assert np.array_equal(ingest.chain_records_numpy(pushes, H, W, oracle.GOP, max_ref, policy), want), policy


@pytest.mark.parametrize("max_ref", [3, 8])
@pytest.mark.parametrize("order", oracle.ORDERS, ids=lambda o: "".join(map(str, o)))
def test_generated_gops_exercise_the_rules(order, max_ref):
    """Per decode order (and max_ref, at both multi-block shapes) the oracle alone meets: pixels with both lists usable, with only list 1
    usable, with neither usable under a present winner, intra with p != f - 1, a NEAR tie, a MEAN half.  In-order pushes always have
    p = f - 1, so that count is asserted zero there.  The policies see different fields, yet differ from each other."""
    for H, W in ((24, 40), (37, 53)):
        pushes, mean, st = oracle.generated(H, W, order, max_ref, "mean")
        for key in oracle.STAT_KEYS:
            if key == "intra_gap" and order == oracle.ORDERS[0]:
                assert st[key] == 0
            else:
                assert st[key] > 0, (H, W, key, st)
        list0, near = (oracle.generated(H, W, order, max_ref, pol)[1] for pol in ("list0", "near"))
        assert not np.array_equal(list0, near) and not np.array_equal(list0, mean) and not np.array_equal(near, mean)
        rec = np.concatenate([r for _, r in pushes])
        assert (rec[:, 6] < 0).any() and (rec[:, 7] & 1).any() and ((rec[:, 2] <= 0) & (rec[:, 3] <= 0)).any()
        x, y, w, h = (rec[:, i].astype(np.int64) for i in range(4))
        assert ((w > 0) & ((x + w <= 0) | (x >= W) | (y + h <= 0) | (y >= H))).any()          # off-frame records


@pytest.mark.parametrize("H,W,F_", [(37, 53, 11), (64, 96, 3)])
def test_p_only_records_in_order_equal_merge_motion(H, W, F_):
    """The anchor: P-only records pushed in order 1, 2, ... give cpu_ref.merge_motion bit for bit, under every policy."""
    from arseg_amd import ingest, synth
    from oracle import cpu_ref

    flows = synth.make_mv_chain(21 + F_, H, W, F_)
    want = cpu_ref.merge_motion(flows).transpose(2, 0, 1, 3).astype(np.int16)
    pushes = [(f, ingest.mv_to_records(flows[f])) for f in range(1, F_ + 1)]
    assert all(not (r[:, 7] & 1).any() for _, r in pushes)
    for policy in oracle.POLICIES:
        assert np.array_equal(ingest.chain_records_numpy(pushes, H, W, F_ + 1, 3, policy), want), policy
    assert np.array_equal(oracle.chain(pushes, H, W, F_ + 1, 3, "near"), want)


def test_chain_records_numpy_refusals():
    from arseg_amd import ingest

    r = np.zeros((1, 8), np.int16)
    for bad in (dict(gop=65), dict(gop=1), dict(max_ref=0), dict(max_ref=17), dict(bipred="nearest"), dict(H=0), dict(W=8193)):
        kw = dict(H=8, W=8, gop=4, max_ref=3, bipred="list0")
        kw.update(bad)
        with pytest.raises(ValueError):
            ingest.chain_records_numpy([(1, r)], **kw)
    for pushes in ([(0, r)], [(4, r)], [(1, r), (1, r)], [(1, r.astype(np.int32))], [(1, np.zeros((3, 7), np.int16))]):
        with pytest.raises(ValueError):
            ingest.chain_records_numpy(pushes, 8, 8, 4)


def test_motion_vectors_to_records():
    from arseg_amd import ingest

    mv = ingest.motion_vectors_to_records
    # centre (12, 20) of a 16x8 block; motion in 1/4, 1/2 and 1/8 pel; past 1, past 3, future 1, future 2
    got = mv([12, 12, 12, 12], [20, 20, 20, 20], [16, 16, 8, 7], [8, 8, 16, 5], [5, -3, 5, -12], [-7, 1, 3, 20], [4, 2, 8, 8], [-1, -3, 1, 2], [0, 1, 1, 0])
    want = np.array([[4, 16, 16, 8, 5, -7, 0, 0],
                     [4, 16, 16, 8, -6, 2, 2, 1],
                     [8, 12, 8, 16, 2, 2, -1, 1],        # 5/8 pel = 2.5 quarter-pel -> 2, 3/8 = 1.5 -> 2: half to even
                     [9, 18, 7, 5, -6, 10, -2, 0]], dtype=np.int16)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    # half to even in both signs: 4 m / 8 = m / 2
    got = mv([0] * 8, [0] * 8, [2] * 8, [2] * 8, [1, 3, 5, 7, -1, -3, -5, -7], [0] * 8, 8, -1)
    assert got[:, 4].tolist() == [0, 2, 2, 4, 0, -2, -2, -4] and not got[:, 6:].any()
    assert mv([], [], [], [], [], [], 4, -1).shape == (0, 8)
    ok = ([5], [5], [8], [8], [1], [1], 4, -1, 0)
    assert mv(*ok).shape == (1, 8)
    for i, bad in ((7, 0), (6, 0), (6, -4), (8, 2), (8, -1), (0, [40000]), (4, [40000]), (7, 40000), (7, -40000), (0, [1.5]), (1, [5, 5])):
        args = list(ok)
        args[i] = bad
        with pytest.raises(ValueError):
            mv(*args)
    # what it returns is what the chain takes: a bi-predicted block between frames 1 and 3, pushed as frame 2
    bi = mv([4, 4], [4, 4], [4, 4], [4, 4], [4, -4], [0, 4], 4, [-1, 1], [0, 1])
    assert np.array_equal(bi, np.array([oracle.rec(2, 2, 4, 4, 4, 0, 0, 0), oracle.rec(2, 2, 4, 4, -4, 4, -1, 1)], dtype=np.int16))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """ARSEG_EINVAL / ARSEG_EWORKSPACE come back before any launch: everything the P-frame step refuses, gop > 64, bit 0 of done_mask
    clear, bit f set, a bit >= gop set, policy outside 0..2, a workspace below two index maps."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)        # non-null pointers are never dereferenced
    EINVAL, EWS = _lib.ARSEG_EINVAL, _lib.ARSEG_EWORKSPACE
    H, W = 10, 12
    need = H * W * 8
    ws = lib.arseg_mv_records_bi_workspace_bytes
    assert ws(H, W) == need == 2 * lib.arseg_mv_records_workspace_bytes(H, W)
    assert ws(8192, 8192) == 8 * 8192 * 8192
    assert ws(8193, 8) == 0 and ws(8, 0) == 0 and ws(-1, 8) == 0
    step = lib.arseg_mv_records_bi_step_fwd
    # (records, n_records, merged, f, gop, done_mask, policy, workspace, workspace_bytes, H, W, max_ref, stream)
    assert step(null, 4, one, 1, 12, 1, 0, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, null, 1, 12, 1, 0, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, 1, 0, null, need, H, W, 3, null) == EINVAL
    assert step(one, -1, one, 1, 12, 1, 0, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, 1, 0, one, 1 << 40, 8193, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, 1, 0, one, 1 << 40, H, 8193, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, 1, 0, one, need, 0, W, 3, null) == EINVAL
    for max_ref in (0, -1, 17):
        assert step(one, 4, one, 1, 12, 1, 0, one, need, H, W, max_ref, null) == EINVAL
    for f, gop in ((0, 12), (12, 12), (-1, 12), (1, 1), (13, 12)):
        assert step(one, 4, one, f, gop, 1, 0, one, need, H, W, 3, null) == EINVAL
    assert step(one, 4, one, 1, 12, 1, 0, one, need - 1, H, W, 3, null) == EWS
    assert step(one, 4, one, 1, 12, 1, 0, one, need // 2, H, W, 3, null) == EWS           # one map is not enough
    assert step(one, 4, one, 1, 12, 1, 0, one, 0, H, W, 3, null) == EWS
    assert step(one, 4, one, 1, 12, 1, 0, odd, need, H, W, 3, null) == EINVAL             # workspace not 16-byte aligned
    assert step(odd, 4, one, 1, 12, 1, 0, one, need, H, W, 3, null) == EINVAL             # records not 16-byte aligned
    assert step(one, 4, ctypes.c_void_p(18), 1, 12, 1, 0, one, need, H, W, 3, null) == EINVAL      # merged not 4-byte aligned
    assert step(one, 4, one, 1, 65, 1, 0, one, need, H, W, 3, null) == EINVAL             # gop > 64
    assert step(one, 4, one, 64, 65, 1, 0, one, need, H, W, 3, null) == EINVAL
    for done in (0, 0b10, 0b1000):                                                         # bit 0 clear
        assert step(one, 4, one, 2, 12, done, 0, one, need, H, W, 3, null) == EINVAL
    for f, done in ((1, 0b11), (5, 0b100101), (11, 1 | 1 << 11)):                          # bit f set
        assert step(one, 4, one, f, 12, done, 0, one, need, H, W, 3, null) == EINVAL
    for done in (1 | 1 << 12, 1 | 1 << 40, 1 | 1 << 63):                                   # a bit >= gop set
        assert step(one, 4, one, 1, 12, done, 0, one, need, H, W, 3, null) == EINVAL
    for policy in (-1, 3, 100):
        assert step(one, 4, one, 1, 12, 1, policy, one, need, H, W, 3, null) == EINVAL
    reset = lib.arseg_mv_records_bi_reset                                                  # (merged, workspace, workspace_bytes, H, W, stream)
    assert reset(null, one, need, H, W, null) == EINVAL
    assert reset(one, null, need, H, W, null) == EINVAL
    assert reset(one, one, need, 8193, W, null) == EINVAL
    assert reset(one, one, need, H, 0, null) == EINVAL
    assert reset(one, odd, need, H, W, null) == EINVAL
    assert reset(ctypes.c_void_p(18), one, need, H, W, null) == EINVAL
    assert reset(one, one, need - 4, H, W, null) == EWS
    assert reset(one, one, need // 2, H, W, null) == EWS


def test_host_layer_refusals_without_a_gpu():
    import torch

    from arseg_amd import _lib, ingest, ops

    rec = torch.zeros((4, 8), dtype=torch.int16)
    merged, idx = torch.zeros((3, 8, 8, 2), dtype=torch.int16), torch.zeros(128, dtype=torch.int32)
    with pytest.raises(_lib.ArsegError):                                   # no CPU fallback
        ops.mv_records_bi_step(rec, merged, 1, 1, idx)
    with pytest.raises(_lib.ArsegError):
        ops.mv_records_bi_reset(merged, idx)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8, 8, device="cpu", bidirectional=True)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8, 8, gop=65, device="cuda", bidirectional=True)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8, 8, gop=8, device="cuda", bidirectional=True, bipred="nearest")
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8193, 8, device="cuda", bidirectional=True)
    with pytest.raises(_lib.ArsegError):
        ingest.MotionChain(8, 8, max_ref=17, device="cuda", bidirectional=True)
    assert ingest.BIPRED == oracle.POLICIES and ops.MV_BI_POLICIES == {"list0": 0, "near": 1, "mean": 2}


def test_entry_points_are_declared_and_abi_version_stays_5():
    from arseg_amd import _lib, ingest, ops

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("arseg_mv_records_bi_workspace_bytes", 2), ("arseg_mv_records_bi_reset", 6), ("arseg_mv_records_bi_step_fwd", 13)):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text)
        declared = re.search(r"%s\s*\((.*?)\)" % name, text, flags=re.S).group(1)
        assert len(declared.split(",")) == len(_lib.PROTOTYPES[name][1]) == n_args
    assert _lib.PROTOTYPES["arseg_mv_records_bi_step_fwd"][1][5] is ctypes.c_uint64
    m = re.search(r"enum arseg_mvr_bi_policy \{ ARSEG_MVR_BI_LIST0 = (\d), ARSEG_MVR_BI_NEAR = (\d), ARSEG_MVR_BI_MEAN = (\d) \}", text)
    assert m and tuple(int(v) for v in m.groups()) == (_lib.MVR_BI_LIST0, _lib.MVR_BI_NEAR, _lib.MVR_BI_MEAN) == (0, 1, 2)
    assert re.search(r"#define ARSEG_ABI_VERSION 5\b", header) and lib.arseg_version() == _lib.ABI_VERSION == 5
    assert callable(ops.mv_records_bi_reset) and callable(ops.mv_records_bi_step) and callable(ingest.chain_records_numpy)
    assert callable(ingest.motion_vectors_to_records)
