"""CPU-side checks of the segmentation confidence: the float64 oracle's own invariants (tests/confidence_oracle.py), that every seeded input
of tests/test_gpu_confidence.py leaves the reference inside the comparison rule's caps, egress.DriftMonitor's decisions, the host layer's
argument checks and the argument validation of arseg_segment_confidence_fwd, which happens before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import confidence_oracle as oracle


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
@pytest.mark.parametrize("kind", oracle.KINDS)
def test_seeded_inputs_leave_the_reference_inside_the_caps(case, kind):
    """At most 10 % of a case's pixels lie within 0.025 codes of a rounding boundary, and the reference takes at least 64 distinct codes --
    for every input the GPU file compares on, so a failure of those caps there is the kernel's."""
    _, _, _, _, _, _, H, W, align = case
    x = oracle.exact(oracle.case_logits(case), H, W, align, kind)
    share, distinct = oracle.reference_figures(x)
    print(f"\n{case[0]} {kind}: boundary share {100 * share:.2f} %, {distinct} distinct codes")
    assert not np.isnan(x).any() and np.abs(oracle.case_logits(case)).max() <= 8.0
    assert share <= oracle.MAX_BOUNDARY_SHARE and distinct >= oracle.MIN_DISTINCT


@pytest.mark.parametrize("case", [c for c in oracle.CASES if c[3] < 32], ids=lambda c: c[0])
def test_special_value_inputs_stay_inside_the_boundary_cap(case):
    """The planted-ties / NaN / inf inputs of the GPU file: the boundary share of the reference stays below the cap with the plants in."""
    _, _, _, _, _, _, H, W, align = case
    logits = oracle.case_logits(case)
    oracle.plant_specials(logits)
    for kind in oracle.KINDS:
        x = oracle.exact(logits, H, W, align, kind)
        share, distinct = oracle.reference_figures(x)
        assert share <= oracle.MAX_BOUNDARY_SHARE and distinct >= oracle.MIN_DISTINCT and np.isnan(x).any()


def test_oracle_invariants():
    """The margin code never exceeds the top-1 code; one class: both are 255 everywhere; NaN rule: a NaN logit, a +inf maximum and an
    all -inf pixel code to 0 and leave every other pixel of a same-size frame alone; log-softmax input gives the same exact values; a hand
    example."""
    case = oracle.CASES[0]
    logits = oracle.case_logits(case)
    H, W = case[6:8]
    top1, margin = oracle.exact(logits, H, W, True, "top1"), oracle.exact(logits, H, W, True, "margin")
    assert (oracle.codes(margin) <= oracle.codes(top1)).all() and (margin <= top1).all() and (margin >= 0).all()
    one = oracle.make_logits(1, 2, 1, 9, 11)
    for kind in oracle.KINDS:
        assert (oracle.codes(oracle.exact(one, 72, 88, False, kind)) == 255).all()
    planted = logits.copy()
    where = oracle.plant_specials(planted)
    for kind, clean in (("top1", top1), ("margin", margin)):
        x = oracle.exact(planted, H, W, True, kind)
        q = oracle.codes(x)
        for n, yy, xx in where:
            assert np.isnan(x[n, yy, xx]) and q[n, yy, xx] == 0
        assert int(np.isnan(x).sum()) == len(where)
        untouched = np.ones_like(q, dtype=bool)
        untouched[:, 4, :] = False
        untouched[:, 6, 2::3] = False
        for n, yy, xx in where:
            untouched[n, yy, xx] = False
        assert np.array_equal(q[untouched], oracle.codes(clean)[untouched])
        assert (oracle.codes(oracle.exact(planted, H, W, True, "margin"))[:, 4, :] == 0).all()          # an exact tie of the top two: margin 0
    import torch

    logp = torch.log_softmax(torch.from_numpy(logits).double(), dim=1).float().numpy()
    assert np.abs(oracle.exact(logp, H, W, True, "top1") - top1).max() < 1e-3
    hand = np.log(np.array([0.6, 0.25, 0.15], dtype=np.float64)).astype(np.float32).reshape(1, 3, 1, 1)
    assert oracle.codes(oracle.exact(hand, 1, 1, True, "top1"))[0, 0, 0] == 153 and oracle.codes(oracle.exact(hand, 1, 1, True, "margin"))[0, 0, 0] == 89
    assert oracle.codes(np.array([0.49, 0.5, 254.5, 255.0, np.nan])).tolist() == [0, 1, 255, 255, 0]
    assert oracle.boundary_mask(np.array([10.5, 10.52, 10.53, 10.47, 10.0, np.nan])).tolist() == [True, True, False, False, False, False]


def test_drift_monitor_decisions():
    """Hand-made rows [sum of codes, low pixels, ...]: a keyframe resets the baseline, the relative-drop trigger, the low-share trigger, no
    trigger; both thresholds are required."""
    from arseg_amd import egress

    n = 1000
    mon = egress.DriftMonitor(rel_drop=0.8, low_share=0.25)
    assert mon.update([100 * n, 400], n, False) is True                # before any keyframe: only the low share applies (40 % > 25 %)
    assert mon.update([100 * n, 100], n, False) is False
    assert mon.update([200 * n, 10], n, True) is False and mon.key_mean == 200.0          # keyframe: baseline 200
    assert mon.update([170 * n, 10], n, False) is False                # 170 >= 0.8 * 200, 1 % low: no trigger
    assert mon.update([160 * n, 10], n, False) is False                # exactly at the threshold: not below it
    assert mon.update([159 * n, 10], n, False) is True                 # relative drop
    assert mon.update([190 * n, 251], n, False) is True                # low share 25.1 % > 25 %
    assert mon.update([190 * n, 250], n, False) is False               # exactly at the share: not above it
    assert mon.update([120 * n, 0], n, True) is False and mon.key_mean == 120.0           # a new keyframe resets the baseline ...
    assert mon.update([100 * n, 0], n, False) is False                 # ... 100 >= 0.8 * 120 now
    assert mon.update([95 * n, 0], n, False) is True
    assert mon.update([10 * n, 900], n, True) is True                  # a keyframe is still held to the low share
    assert mon.update(np.array([150 * n, 0] + [0] * 32, dtype=np.int64), n, True) is False          # a row of the statistics tensor
    with pytest.raises(TypeError):
        egress.DriftMonitor()
    with pytest.raises(TypeError):
        egress.DriftMonitor(0.8)
    for bad in ((0.0, 0.5), (1.5, 0.5), (0.8, -0.1), (0.8, 1.1)):
        with pytest.raises(ValueError):
            egress.DriftMonitor(*bad)
    with pytest.raises(ValueError):
        mon.update([0, 0], 0, False)
    assert "calibrate" in egress.DriftMonitor.__doc__


def test_host_layer_argument_checks():
    """ArsegError for CPU tensors (no CPU fallback), ValueError for a malformed logits tensor, before anything touches a GPU."""
    import torch

    from arseg_amd import _lib, egress, ops

    logits = torch.zeros((1, 12, 4, 6))
    with pytest.raises(_lib.ArsegError):
        egress.confidence(logits, 4, 6)
    with pytest.raises(_lib.ArsegError):
        ops.segment_confidence(logits, 4, 6, stats=torch.zeros((1, _lib.CONF_NSTATS), dtype=torch.int64))
    with pytest.raises(ValueError):
        egress.confidence(torch.zeros((12, 4, 6)), 4, 6)
    assert _lib.CONF_NSTATS == 34 and (_lib.CONF_TOP1, _lib.CONF_MARGIN) == (0, 1)


def test_entry_point_is_declared_and_abi_version_stays_5():
    from conftest import ROOT

    from arseg_amd import _lib

    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    assert re.search(r"\bint arseg_segment_confidence_fwd\(", header) and "arseg_segment_confidence_fwd" in _lib.PROTOTYPES
    assert re.search(r"#define ARSEG_CONF_NSTATS \(2 \+ 32\)", header) and re.search(r"#define ARSEG_ABI_VERSION 5\b", header)
    lib = _lib.load()
    assert lib.arseg_version() == _lib.ABI_VERSION == 5


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract comes back before any launch (device pointers are dummies and never dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    fn = lib.arseg_segment_confidence_fwd
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    EINVAL = _lib.ARSEG_EINVAL
    H, W = 32, 48
    lut = (ctypes.c_uint8 * 32)(*range(32))

    def call(logits=one, N=2, n_cls=19, h=4, w=6, H=H, W=W, align=0, kind=_lib.CONF_TOP1, low=128, lut=lut, conf=one, conf_pitch=W, conf_ns=H * W,
             lab=one, lab_pitch=W, lab_ns=H * W, stats=one):
        return fn(logits, N, n_cls, h, w, H, W, align, kind, low, lut, conf, conf_pitch, conf_ns, lab, lab_pitch, lab_ns, stats, null)

    assert call(logits=null) == EINVAL                                            # null logits
    assert call(conf=null, lab=null, stats=null) == EINVAL                        # no output requested
    for bad in (0, -1, 33):
        assert call(n_cls=bad) == EINVAL                                          # n_cls outside 1 .. 32
        assert call(n_cls=bad, conf=null, lab=null) == EINVAL
    for name in ("N", "h", "w", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL       # a non-positive size
    assert call(conf_pitch=W - 1) == EINVAL and call(lab_pitch=W - 1) == EINVAL   # a pitch below W
    assert call(conf_pitch=W - 1, lab=null) == EINVAL and call(lab_pitch=W - 1, conf=null, stats=null) == EINVAL
    assert call(conf_ns=-1) == EINVAL and call(lab_ns=-1) == EINVAL               # a negative stride
    for bad in (-1, 2, 7):
        assert call(kind=bad) == EINVAL                                           # an unknown kind
    for bad in (-1, 257, 1000):
        assert call(low=bad) == EINVAL                                            # low outside 0 .. 256
    assert call(low=bad, conf=null, lab=null) == EINVAL
