"""CPU-side checks of the temporal consistency: the numpy oracle's own invariants and hand-made rounding cases
(tests/consistency_oracle.py), that every seeded input of tests/test_gpu_consistency.py exercises all four outcomes and every class,
egress.tc_table against hand-computed rows, egress.ConsistencyMonitor's decisions, the host layer's argument checks and the argument
validation of arseg_segment_consistency_fwd / arseg_labels_consistency_fwd, which happens before any launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import consistency_oracle as oracle


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_seeded_inputs_are_spread_over_all_outcomes(case):
    """Per frame of every case the GPU file compares on, with the labels of the float64 argmax: agreeing pixels are 20 % .. 90 % of the
    compared ones; differing, outside and void pixels are each at least 1 % of the frame; with up to 19 classes every class has a non-zero
    cur, ref and inter -- so the GPU tests cannot pass on degenerate inputs."""
    n_cls = case[3]
    for n, (agree, differ, outside, void, least) in enumerate(oracle.spread(case)):
        print(f"\n{case[0]} frame {n}: agree {100 * agree:.1f} % of compared; of the frame: differ {100 * differ:.1f} %, outside "
              f"{100 * outside:.1f} %, void {100 * void:.1f} %; smallest class counter {least}")
        assert 0.20 <= agree <= 0.90
        assert differ >= 0.01 and outside >= 0.01 and void >= 0.01
        if n_cls <= 19:
            assert least > 0


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_oracle_invariants(case):
    """compared + outside + void == H W; sum cur == sum ref == compared; inter_k <= min(cur_k, ref_k); change == 0 exactly where the pixel
    is counted in inter; 255 / 128 partition the rest as differ / not compared; the entries from n_cls on stay zero."""
    b = oracle.build(case)
    n_cls, H, W = case[3], case[6], case[7]
    change, stats, labels8 = oracle.consistency(b["labels"], b["ref"], b["mv"], n_cls)
    assert change.dtype == np.uint8 and stats.dtype == np.int64 and stats.shape == (case[2], oracle.TC_NSTATS) and oracle.TC_NSTATS == 99
    cur, ref, inter = (stats[:, o:o + 32] for o in (oracle.CUR, oracle.REF, oracle.INTER))
    assert (stats[:, 0] + stats[:, 1] + stats[:, 2] == H * W).all()
    assert (cur.sum(axis=1) == stats[:, 0]).all() and (ref.sum(axis=1) == stats[:, 0]).all()
    assert (inter <= np.minimum(cur, ref)).all()
    assert not cur[:, n_cls:].any() and not ref[:, n_cls:].any() and not inter[:, n_cls:].any()
    assert ((change == 0).sum(axis=(1, 2)) == inter.sum(axis=1)).all()
    assert ((change == 255).sum(axis=(1, 2)) == stats[:, 0] - inter.sum(axis=1)).all()
    assert ((change == 128).sum(axis=(1, 2)) == stats[:, 1] + stats[:, 2]).all()
    assert set(np.unique(change)) <= {0, 128, 255}
    for n in range(case[2]):
        for k in range(n_cls):
            assert int(((change[n] == 0) & (b["labels"][n] == k)).sum()) == int(inter[n, k])
    assert np.array_equal(labels8, b["labels"])
    lut = np.arange(100, 100 + n_cls, dtype=np.uint8)
    c2, s2, l2 = oracle.consistency(b["labels"], b["ref"], b["mv"], n_cls, lut=lut)
    assert np.array_equal(c2, change) and np.array_equal(s2, stats) and np.array_equal(l2, b["labels"] + 100)


def test_rounding_hand_made():
    """round_half_even_div4 on the halves (-6, -2, 2, 6, 10: to the even neighbour) and on +-3, +-5, against np.round on exact quarters;
    then the same vectors through the oracle on a one-row frame whose reference holds its own column index."""
    v = np.array([-6, -2, 2, 6, 10, -3, 3, -5, 5, 0, 1, -1, 4, -4, 32767, -32768])
    want = [-2, 0, 0, 2, 2, -1, 1, -1, 1, 0, 0, 0, 1, -1, 8192, -8192]
    assert oracle.round_half_even_div4(v).tolist() == want
    assert oracle.round_half_even_div4(np.arange(-64, 65)).tolist() == np.round(np.arange(-64, 65) / 4.0).astype(int).tolist()
    W, x0 = 16, 8
    ref = np.arange(W, dtype=np.uint8)[None, None, :]                        # ref[0, 0, x] = x
    for mvx, d in zip(v[:9].tolist(), want[:9]):
        mv = np.zeros((1, 1, W, 2), dtype=np.int16)
        mv[0, 0, :, 0] = mvx
        labels = np.full((1, 1, W), x0 + d)                                 # agrees exactly at x = x0
        change, stats, _ = oracle.consistency(labels, ref, mv, 32)
        inside = [(0 <= x + d < W) for x in range(W)]
        assert change[0, 0, x0] == 0 and int((change == 0).sum()) == 1
        assert stats[0, 1] == W - sum(inside) and stats[0, 0] == sum(inside) and stats[0, 2] == 0
        assert stats[0, oracle.INTER + x0 + d] == 1 and stats[0, oracle.CUR + x0 + d] == sum(inside)
    mv = np.zeros((1, 2, 2, 2), dtype=np.int16)                             # the vertical component and the order of (mvx, mvy)
    mv[0, 0, 0] = (0, 6)                                                    # (0, 0) -> row 0 + 2: outside a 2-row frame
    mv[0, 0, 1] = (-2, 2)                                                   # (1, 0) -> (1, 0): both halves go to 0
    mv[0, 1, 0] = (3, -3)                                                   # (0, 1) -> (1, 0)
    mv[0, 1, 1] = (-5, -5)                                                  # (1, 1) -> (0, 0)
    ref = np.array([[[7, 9], [255, 255]]], dtype=np.uint8)
    change, stats, _ = oracle.consistency(np.array([[[7, 9], [9, 9]]]), ref, mv, 19)
    assert change.tolist() == [[[128, 0], [0, 255]]] and stats[0, :3].tolist() == [3, 1, 0]
    assert stats[0, oracle.CUR + 9] == 3 and stats[0, oracle.REF + 9] == 2 and stats[0, oracle.REF + 7] == 1 and stats[0, oracle.INTER + 9] == 2
    # void on either side, and outside before void
    change, stats, _ = oracle.consistency(np.array([[[7, 255], [9, 19]]]), ref, mv, 19)
    assert change.tolist() == [[[128, 128], [0, 128]]] and stats[0, :3].tolist() == [1, 1, 2]


def test_tc_table_against_hand_computed_rows():
    from arseg_amd import _lib, egress

    rows = np.zeros((4, _lib.TC_NSTATS), dtype=np.int64)
    # frame 0: 3 classes; cur = (50, 30, 20), ref = (40, 40, 20), inter = (35, 25, 20): agreement 0.8; IoU 35/55, 25/45, 20/20
    rows[0, :3] = (100, 20, 5)
    rows[0, 3:6], rows[0, 35:38], rows[0, 67:70] = (50, 30, 20), (40, 40, 20), (35, 25, 20)
    # frame 1: class 1 absent on both sides (no union: left out of the mean), class 2 only in the frame (IoU 0)
    rows[1, :3] = (10, 0, 0)
    rows[1, 3:6], rows[1, 35:38], rows[1, 67:70] = (6, 0, 4), (10, 0, 0), (6, 0, 0)
    # frame 2: nothing compared
    rows[2, :3] = (0, 60, 40)
    # frame 3: perfect
    rows[3, :3] = (8, 0, 0)
    rows[3, 3:6], rows[3, 35:38], rows[3, 67:70] = (8, 0, 0), (8, 0, 0), (8, 0, 0)
    t = egress.tc_table(rows, 3)
    assert set(t) == {"agreement", "tc_miou", "compared_share"} and all(v.shape == (4,) and v.dtype == np.float64 for v in t.values())
    assert t["agreement"][0] == pytest.approx(0.8) and t["tc_miou"][0] == pytest.approx((35 / 55 + 25 / 45 + 1.0) / 3)
    assert t["compared_share"][0] == pytest.approx(100 / 125)
    assert t["agreement"][1] == pytest.approx(0.6) and t["tc_miou"][1] == pytest.approx((6 / 10 + 0.0) / 2) and t["compared_share"][1] == 1.0
    assert math.isnan(t["agreement"][2]) and math.isnan(t["tc_miou"][2]) and t["compared_share"][2] == 0.0
    assert t["agreement"][3] == 1.0 and t["tc_miou"][3] == 1.0
    for got, want in zip(zip(t["agreement"], t["tc_miou"], t["compared_share"]), oracle.tc_rows(rows, 3)):
        assert all((math.isnan(g) and math.isnan(w)) or g == pytest.approx(w) for g, w in zip(got, want))
    import torch

    one = egress.tc_table(torch.from_numpy(rows[0]), 3)                   # one row, as a tensor
    assert one["agreement"].shape == (1,) and one["agreement"][0] == pytest.approx(0.8)
    with pytest.raises(ValueError):
        egress.tc_table(rows[:, :50], 3)
    with pytest.raises(ValueError):
        egress.tc_table(rows, 33)


def test_consistency_monitor_decisions():
    """Hand-made rows: the agreement trigger, the compared-share trigger, no trigger, the exact thresholds, a frame of which nothing could
    be compared; both thresholds are required."""
    from arseg_amd import _lib, egress

    def row(compared, agree):
        r = [0] * _lib.TC_NSTATS
        r[0] = compared
        r[67 + 3], r[67 + 31] = agree // 2, agree - agree // 2          # spread over two classes: the monitor sums all 32
        return r

    n = 1000
    mon = egress.ConsistencyMonitor(min_agreement=0.7, min_compared_share=0.5)
    assert mon.update(row(800, 700), n) is False                       # 87.5 % agree, 80 % compared
    assert mon.update(row(800, 560), n) is False                       # exactly 70 %: not below
    assert mon.update(row(800, 559), n) is True                        # agreement below the threshold
    assert mon.update(row(500, 500), n) is False                       # exactly half compared: not below
    assert mon.update(row(499, 499), n) is True                        # the chain has left the picture
    assert mon.update(row(0, 0), n) is True                            # nothing compared
    assert egress.ConsistencyMonitor(0.7, 0.0).update(row(0, 0), n) is False          # ... and no undefined agreement is reported
    assert egress.ConsistencyMonitor(0.0, 0.0).update(row(10, 0), n) is False
    assert egress.ConsistencyMonitor(1.0, 1.0).update(row(n, n), n) is False and egress.ConsistencyMonitor(1.0, 1.0).update(row(n, n - 1), n) is True
    assert mon.update(np.array(row(900, 100), dtype=np.int64), n) is True             # a row of the statistics tensor
    with pytest.raises(TypeError):
        egress.ConsistencyMonitor()
    with pytest.raises(TypeError):
        egress.ConsistencyMonitor(0.7)
    for bad in ((-0.1, 0.5), (1.5, 0.5), (0.7, -0.1), (0.7, 1.1)):
        with pytest.raises(ValueError):
            egress.ConsistencyMonitor(*bad)
    with pytest.raises(ValueError):
        mon.update(row(1, 1), 0)
    assert "calibrate" in egress.ConsistencyMonitor.__doc__
    assert not hasattr(egress.DriftMonitor, "min_agreement")           # the sibling is its own class


def test_host_layer_argument_checks():
    """ArsegError for CPU tensors (no CPU fallback), ValueError for malformed tensors, before anything touches a GPU."""
    import torch

    from arseg_amd import _lib, egress, evaluation, ops

    logits = torch.zeros((1, 12, 4, 6))
    ref, mv = torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((1, 4, 6, 2), dtype=torch.int16)
    with pytest.raises(_lib.ArsegError):
        egress.consistency(logits, ref, mv, 4, 6)
    with pytest.raises(_lib.ArsegError):
        ops.segment_consistency(logits, ref[None], mv, 4, 6, stats=torch.zeros((1, _lib.TC_NSTATS), dtype=torch.int64))
    with pytest.raises(_lib.ArsegError):
        egress.consistency_of_planes(torch.zeros((1, 4, 6), dtype=torch.uint8), ref, mv, 12)
    with pytest.raises(_lib.ArsegError):
        ops.labels_consistency(torch.zeros((1, 4, 6), dtype=torch.uint8), ref[None], mv, 12, stats=torch.zeros((1, _lib.TC_NSTATS), dtype=torch.int64))
    with pytest.raises(ValueError):
        egress.consistency(torch.zeros((12, 4, 6)), ref, mv, 4, 6)
    with pytest.raises(ValueError):
        egress.consistency(logits, torch.zeros((1, 1, 4, 6), dtype=torch.uint8), mv, 4, 6)
    with pytest.raises(ValueError):
        egress.consistency_of_planes(torch.zeros((4, 6), dtype=torch.uint8), ref, mv, 12)
    assert _lib.TC_NSTATS == 99 == oracle.TC_NSTATS
    assert callable(evaluation.alter_res_batch_consistency)


def test_entry_points_are_declared_and_abi_version_stays_5():
    from conftest import ROOT

    from arseg_amd import _lib

    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    for name in ("arseg_segment_consistency_fwd", "arseg_labels_consistency_fwd"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.PROTOTYPES
    assert re.search(r"#define ARSEG_TC_NSTATS \(3 \+ 3 \* 32\)", header) and re.search(r"#define ARSEG_ABI_VERSION 5\b", header)
    lib = _lib.load()
    assert lib.arseg_version() == _lib.ABI_VERSION == 5


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract, for both entry points, comes back before any launch (device pointers are dummies and never
    dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(66)
    EINVAL = _lib.ARSEG_EINVAL
    H, W = 32, 48
    lut = (ctypes.c_uint8 * 32)(*range(32))

    def seg(logits=one, N=2, n_cls=19, h=4, w=6, H=H, W=W, align=0, ref=one, ref_pitch=W, ref_ns=0, mv=one, lut=lut, lab=one, lab_pitch=W,
            lab_ns=H * W, chg=one, chg_pitch=W, chg_ns=H * W, stats=one):
        return lib.arseg_segment_consistency_fwd(logits, N, n_cls, h, w, H, W, align, ref, ref_pitch, ref_ns, mv, lut, lab, lab_pitch, lab_ns, chg,
                                                 chg_pitch, chg_ns, stats, null)

    def pln(src=one, in_pitch=W, in_ns=H * W, N=2, n_cls=19, H=H, W=W, ref=one, ref_pitch=W, ref_ns=0, mv=one, chg=one, chg_pitch=W,
            chg_ns=H * W, stats=one):
        return lib.arseg_labels_consistency_fwd(src, in_pitch, in_ns, N, n_cls, H, W, ref, ref_pitch, ref_ns, mv, chg, chg_pitch, chg_ns, stats, null)

    assert seg(logits=null) == EINVAL and pln(src=null) == EINVAL                          # null logits / source plane
    for fn in (seg, pln):
        assert fn(ref=null) == EINVAL and fn(mv=null) == EINVAL                            # null ref_labels / mv_q
        assert fn(mv=odd) == EINVAL                                                        # mv_q not 4-byte aligned
        for bad in (0, -1, 33):
            assert fn(n_cls=bad) == EINVAL and fn(n_cls=bad, chg=null) == EINVAL           # n_cls outside 1 .. 32
        for name in ("N", "H", "W"):
            assert fn(**{name: 0}) == EINVAL and fn(**{name: -3}) == EINVAL                # a non-positive size
        assert fn(ref_pitch=W - 1) == EINVAL and fn(chg_pitch=W - 1) == EINVAL             # a pitch below W
        assert fn(chg_pitch=W - 1, stats=null) == EINVAL
        assert fn(ref_ns=-1) == EINVAL and fn(chg_ns=-1) == EINVAL                         # a negative stride
    for name in ("h", "w"):
        assert seg(**{name: 0}) == EINVAL and seg(**{name: -3}) == EINVAL
    assert seg(lab=null, chg=null, stats=null) == EINVAL and pln(chg=null, stats=null) == EINVAL          # no output at all
    assert seg(lab_pitch=W - 1) == EINVAL and seg(lab_pitch=W - 1, chg=null, stats=null) == EINVAL and seg(lab_ns=-1) == EINVAL
    assert pln(in_pitch=W - 1) == EINVAL and pln(in_ns=-1) == EINVAL
    for align in (0, 1):                                                                   # the run route (x8 here) and the per-pixel route alike
        assert seg(align=align, ref_pitch=W - 1) == EINVAL and seg(align=align, lab=null, chg=null, stats=null) == EINVAL
