"""CPU-side checks of the calibration counts (include/arseg_hip.h, arseg_calibration_fwd): the hand cases' literal tables, the host form
evaluation.calibration_numpy against the oracle's pixel loop on them and on the seeded cases, the conditions the seeded inputs must meet
for the GPU comparison to mean something, CalibrationTable's arithmetic on a literal table, every argument the entry point refuses before a
launch, and header, binding, exports and documents in step.  All comparisons of counts are exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import calibration_oracle as co
import confidence_oracle as oracle
from conftest import ROOT


@pytest.mark.parametrize("name,logits,label,groups,n_groups,kind,want", co.HAND, ids=co.HAND_IDS)
def test_hand_cases_have_the_written_tables(name, logits, label, groups, n_groups, kind, want):
    from arseg_amd import evaluation as ev

    label = np.array(label, dtype=np.int64)
    n_cls, W = logits.shape[1], label.shape[-1]
    table = co.sparse(want, n_groups, n_cls)
    assert np.array_equal(co.table(logits, label, 1, W, n_cls, groups, n_groups, kind=kind), table)
    host = ev.calibration_numpy(logits, label, 1, W, n_cls, groups=groups, n_groups=n_groups, kind=kind)
    assert host.dtype == np.int64 and host.shape == (n_groups, n_cls, 256, 2) and np.array_equal(host, table)


def test_hand_cases_cover_what_they_are_there_for():
    by = {h[0]: h for h in co.HAND}
    assert len(co.HAND) >= 8
    assert 255 in np.array(by["ignored-pixel"][2]) and {-1, 2} <= set(np.array(by["labels-below-and-above"][2]).ravel().tolist())
    assert by["labels-below-and-above"][1].shape[1] == 2                                          # 2 == n_cls
    assert any(n != r for n, r in by["wrong-pixel"][6].values())
    assert by["two-groups"][4] == 2 and {g for g, _, _ in by["two-groups"][6]} == {0, 1}
    assert by["group-out-of-range"][3] == [2, -1, 1] and sum(n for n, _ in by["group-out-of-range"][6].values()) == 1
    assert np.isnan(by["nan-pixel"][1]).any() and by["nan-pixel"][6][(0, 1, 0)] == (1, 1)       # the NaN pixel: its class, code 0
    assert by["one-class"][1].shape[1] == 1 and set(by["one-class"][6]) == {(0, 0, 255)}
    assert np.array_equal(by["margin-vs-top1/top1"][1], by["margin-vs-top1/margin"][1]) and by["margin-vs-top1/top1"][6] != by["margin-vs-top1/margin"][6]


@pytest.fixture(scope="module")
def seeded():
    """(case name, kind) -> (logits, labels, groups, the oracle's table), computed once per module."""
    cache = {}

    def get(case, kind):
        if case[0] not in cache:
            cache[case[0]] = (oracle.case_logits(case), co.case_labels(case), {})
        logits, label, tables = cache[case[0]]
        if kind not in tables:
            _, _, N, n_cls, h, w, H, W, align = case
            tables[kind] = co.table(logits, label, H, W, n_cls, co.case_groups(case), 2, kind=kind, align_corners=align)
        return logits, label, co.case_groups(case), tables[kind]
    return get


@pytest.mark.parametrize("kind", oracle.KINDS)
@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_numpy_form_equals_the_definition_on_the_seeded_cases(seeded, case, kind):
    from arseg_amd import evaluation as ev

    name, _, N, n_cls, h, w, H, W, align = case
    logits, label, groups, want = seeded(case, kind)
    got = ev.calibration_numpy(logits, label, H, W, n_cls, groups=groups, n_groups=2, kind=kind, align_corners=align)
    assert np.array_equal(got, want)
    # the conditions on the inputs: a table with few codes, or whose codes are all right or all wrong, would compare little
    per_code = want.sum(axis=(0, 1))
    filled = int((per_code[:, 0] > 0).sum())
    mixed = int(((per_code[:, 1] > 0) & (per_code[:, 1] < per_code[:, 0])).sum())
    print(f"\n{name} {kind}: {filled} non-empty codes, {mixed} with right and wrong pixels, {int(want[..., 0].sum())} counting pixels of {N * H * W}")
    assert filled >= 128 and mixed >= 64
    assert (want[..., 0].sum(axis=(0, 2)) > 0).all()                                             # every class is predicted
    assert (want[..., 0].sum(axis=(1, 2)) > 0).all()                                             # both groups count
    counting = (label >= 0) & (label < n_cls) & (label != 255)
    assert int(want[..., 0].sum()) == int(counting.sum()) < N * H * W
    assert (label == -1).any() and (label == n_cls + 3).any() and (label == 255).any()
    # the link to the tail, on the host: columns and diagonal of the confusion matrix of the same predictions
    k = co.classes(logits, H, W, align)
    for g in range(2):
        frames = [n for n in range(N) if groups[n] == g]
        hist = np.zeros((n_cls, n_cls), np.int64)
        np.add.at(hist, (label[frames][counting[frames]], k[frames][counting[frames]]), 1)
        assert np.array_equal(want[g, :, :, 0].sum(axis=1), hist.sum(axis=0)) and np.array_equal(want[g, :, :, 1].sum(axis=1), np.diag(hist))


def test_numpy_form_refuses_bad_arguments():
    from arseg_amd import evaluation as ev

    logits, label = np.zeros((2, 3, 4, 4), np.float32), np.zeros((2, 4, 4), np.int64)
    assert ev.calibration_numpy(logits, label, 4, 4, 3)[0, 0, 85, 0] == 32                       # p = 1/3: floor(85 + 0.5)
    for bad in (dict(kind="entropy"), dict(n_groups=2), dict(n_groups=0), dict(groups=[0], n_groups=1), dict(n_cls=4)):
        with pytest.raises(ValueError):
            ev.calibration_numpy(logits, label, 4, 4, **{"n_cls": 3, **bad})
    with pytest.raises(ValueError):
        ev.calibration_numpy(logits, label.astype(np.float32), 4, 4, 3)
    with pytest.raises(ValueError):
        ev.calibration_numpy(logits, label[:1], 4, 4, 3)
    with pytest.raises(ValueError):
        ev.calibration_numpy(logits[0], label, 4, 4, 3)


def _literal():
    """One group, two classes: class 0 has 6 pixels at code 255 (all right) and 2 at 128 (1 right); class 1 has 2 at code 64 (none right)."""
    c = np.zeros((1, 2, 256, 2), np.int64)
    c[0, 0, 255], c[0, 0, 128], c[0, 1, 64] = (6, 6), (2, 1), (2, 0)
    return c


def test_calibration_table_arithmetic_on_a_literal_table():
    from arseg_amd import evaluation as ev

    t = ev.CalibrationTable(torch.from_numpy(_literal()))
    assert t.kind == "top1" and tuple(t.counts().shape) == (1, 256, 2) and tuple(t.counts(per_class=True).shape) == (1, 2, 256, 2)
    assert t.counts()[0, 128].tolist() == [2, 1] and int(t.counts()[..., 0].sum()) == 10
    f = np.float32
    assert t.accuracy().dtype == torch.float32 and t.accuracy().tolist() == [f(7) / f(10)]
    assert t.confidence().tolist() == [f(6 * 255 + 2 * 128 + 2 * 64) / f(2550)]
    for n_bins, bins in ((4, (1, 2, 3)), (15, (3, 7, 14)), (256, (64, 128, 255)), (1, None)):
        conf, acc, weight = t.reliability(n_bins)
        assert tuple(conf.shape) == tuple(acc.shape) == tuple(weight.shape) == (1, n_bins)
        if bins is None:                                                            # one bin: the whole table
            assert conf[0, 0].item() == t.confidence()[0].item() and acc[0, 0].item() == t.accuracy()[0].item() and weight[0, 0].item() == 1.0
            assert t.ece(1)[0].item() == pytest.approx(1914 / 2550 - 0.7, abs=1e-6) and t.mce(1)[0].item() == t.ece(1)[0].item()
            continue
        lo, mid, hi = bins
        assert weight[0, [lo, mid, hi]].tolist() == [f(2) / f(10), f(2) / f(10), f(6) / f(10)] and float(weight.sum()) == pytest.approx(1.0, abs=1e-6)
        assert acc[0, [lo, mid, hi]].tolist() == [0.0, 0.5, 1.0]
        assert conf[0, [lo, mid, hi]].tolist() == [f(128) / f(510), f(256) / f(510), 1.0]
        empty = [b for b in range(n_bins) if b not in bins]
        assert conf[0, empty].isnan().all() and acc[0, empty].isnan().all() and (weight[0, empty] == 0).all()
        assert t.ece(n_bins)[0].item() == pytest.approx(0.2 * 64 / 255 + 0.2 * abs(0.5 - 128 / 255), abs=1e-6)
        assert t.mce(n_bins)[0].item() == pytest.approx(64 / 255, abs=1e-6)
        assert t.classwise_ece(n_bins)[0].item() == pytest.approx((0.25 * abs(0.5 - 128 / 255) + 64 / 255) / 2, abs=1e-6)
    assert t.ece().item() == t.ece(15).item()
    coverage, selective = t.risk_coverage()
    assert tuple(coverage.shape) == tuple(selective.shape) == (1, 256)
    assert (coverage[0, :65] == 1.0).all() and (coverage[0, 65:129] == f(8) / f(10)).all() and (coverage[0, 129:] == f(6) / f(10)).all()
    assert (selective[0, :65] == f(7) / f(10)).all() and (selective[0, 65:129] == f(7) / f(8)).all() and (selective[0, 129:] == 1.0).all()
    assert t.accuracy_below(128).tolist() == [0.0] and t.accuracy_below(129).tolist() == [0.25] and t.accuracy_below(256).tolist() == [f(7) / f(10)]
    assert np.isnan(t.accuracy_below(0).item()) and np.isnan(t.accuracy_below(64).item())
    thr = t.threshold_for(0.8)
    assert thr.dtype == torch.int64 and thr.tolist() == [65]
    assert t.threshold_for(0.5).tolist() == [0] and t.threshold_for(0.9).tolist() == [129] and t.threshold_for(1.0).tolist() == [129]
    assert t.threshold_for(1.01).tolist() == [256]
    for bad in (0, 257):
        with pytest.raises(ValueError):
            t.reliability(bad)
        with pytest.raises(ValueError):
            t.ece(bad)
    with pytest.raises(ValueError):
        t.accuracy_below(257)


def test_calibration_table_groups_pooling_and_files(tmp_path):
    from arseg_amd import evaluation as ev

    c = np.zeros((3, 2, 256, 2), np.int64)
    c[0] = _literal()[0]
    c[2, 1, 200] = (4, 3)                                                            # group 1 has no pixels
    t = ev.CalibrationTable(c, kind="margin")
    assert t.accuracy()[0].item() == np.float32(0.7) and np.isnan(t.accuracy()[1].item()) and t.accuracy()[2].item() == 0.75
    for v in (t.confidence(), t.ece(), t.mce(), t.classwise_ece(), t.accuracy_below(256)):
        assert tuple(v.shape) == (3,) and np.isnan(v[1].item()) and not np.isnan(v[0].item()) and not np.isnan(v[2].item())
    assert t.ece()[2].item() == pytest.approx(abs(0.75 - 200 / 255), abs=1e-6) and t.classwise_ece()[2].item() == t.ece()[2].item()
    assert t.threshold_for(0.75).tolist() == [65, 256, 0] and t.threshold_for(0.7).tolist() == [0, 256, 0]
    pooled = t.pooled()
    assert isinstance(pooled, ev.CalibrationTable) and pooled.kind == "margin" and tuple(pooled.cal.shape) == (1, 2, 256, 2)
    assert torch.equal(pooled.cal[0], t.cal.sum(dim=0)) and pooled.accuracy().tolist() == [np.float32(10) / np.float32(14)]
    path = tmp_path / "cal.npz"
    t.save(path)
    back = ev.CalibrationTable.load(path)
    assert back.kind == "margin" and back.cal.dtype == torch.int64 and torch.equal(back.cal, t.cal)
    other = tmp_path / "other.npz"
    np.savez(other, counts=c)
    with pytest.raises(ValueError):
        ev.CalibrationTable.load(other)
    for bad in (c[0], c[:, :, :255], c[..., :1], c.astype(np.float32)):
        with pytest.raises(ValueError):
            ev.CalibrationTable(bad)
    with pytest.raises(ValueError):
        ev.CalibrationTable(c, kind="entropy")


def test_a_perfectly_calibrated_table_has_no_calibration_error():
    """Of the pixels with code q exactly q / 255 are right: what is left is float32 rounding, far inside the 0.5 / 255 the 8-bit code costs.
    And the quantisation itself: pixels whose true confidences fill a code's interval evenly move a bin's mean by less than 0.5 / 255."""
    from arseg_amd import evaluation as ev

    c = np.zeros((2, 3, 256, 2), np.int64)
    q = np.arange(256)
    for k in range(3):
        c[0, k, :, 0], c[0, k, :, 1] = 255 * (k + 1), q * (k + 1)
    c[1, 0, :, 0], c[1, 0, :, 1] = 255 * (1 + q % 7), q * (1 + q % 7)
    t = ev.CalibrationTable(c)
    for n_bins in (1, 10, 15, 256):
        assert float(t.ece(n_bins).max()) <= 0.5 / 255 and float(t.mce(n_bins).max()) <= 0.5 / 255 and float(t.classwise_ece(n_bins).max()) <= 0.5 / 255
        assert float(t.ece(n_bins).max()) <= 1e-6
    assert t.threshold_for(0.5).tolist() == [0, 0]
    g = np.random.Generator(np.random.PCG64(7))
    true = g.random(200000)
    codes = np.floor(255 * true + 0.5).astype(np.int64)
    conf, _, weight = ev.CalibrationTable(np.stack([np.bincount(codes, minlength=256)] * 2, axis=-1)[None, None]).reliability(15)
    index = codes * 15 // 256
    fp = np.array([true[index == b].mean() for b in range(15)])
    assert float(np.abs(conf[0].numpy() - fp).max()) <= 0.5 / 255 and float(weight.sum()) == pytest.approx(1.0, abs=1e-6)


def test_eval_by_calibration_keeps_the_distance_evaluator():
    from arseg_amd import evaluation as ev

    e = ev.EvalByCalibration(scale=0.5, gop=12)
    assert isinstance(e, ev.EvalByDistance) and e.kind == "top1" and e.gop == 12 and e.ignore_label == 255 and e.hr_forwards == 0
    assert ev.EvalByCalibration(kind="margin", gop=4, cache_keyframe=True).kind == "margin"
    with pytest.raises(ValueError):
        ev.EvalByCalibration(kind="entropy")
    with pytest.raises(ValueError):
        ev.EvalByCalibration(gop=0)
    assert e._groups(torch.tensor([3, 11]), 2) == [3, 11]
    with pytest.raises(ValueError):
        e._groups(12, 1)


def _call(lib, logits, label, group, cal, N, n_groups, n_cls, h, w, H, W, align, kind):
    return lib.arseg_calibration_fwd(logits, label, group, cal, N, n_groups, n_cls, h, w, H, W, 255, align, kind, ctypes.c_void_p(0))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Never-dereferenced pointers: every refusal comes before a launch, so none of these touches a GPU."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    good = dict(logits=one, label=one, group=one, cal=one, N=2, n_groups=3, n_cls=19, h=8, w=10, H=64, W=80, align=0, kind=_lib.CONF_TOP1)
    bad = [dict(logits=null), dict(label=null), dict(cal=null), dict(group=null), dict(group=null, n_groups=2), dict(n_groups=0), dict(n_groups=-1),
           dict(group=null, n_groups=0), dict(n_cls=0), dict(n_cls=33), dict(n_cls=-1), dict(N=0), dict(N=-1), dict(h=0), dict(w=0), dict(H=0),
           dict(W=0), dict(h=-8), dict(W=-80), dict(kind=2), dict(kind=-1), dict(label=ctypes.c_void_p(68)), dict(cal=ctypes.c_void_p(68)),
           dict(label=ctypes.c_void_p(65)), dict(group=ctypes.c_void_p(66)), dict(group=ctypes.c_void_p(65))]
    for change in bad:
        assert _call(lib, **{**good, **change}) == _lib.ARSEG_EINVAL, change
    for route in (dict(h=64, w=80), dict(align=1), dict(H=16, W=20), dict(kind=_lib.CONF_MARGIN)):      # on every route, either kind
        assert _call(lib, **{**good, **route, "n_cls": 33}) == _lib.ARSEG_EINVAL, route
        assert _call(lib, **{**good, **route, "cal": null}) == _lib.ARSEG_EINVAL, route


def test_header_binding_and_exports_in_step():
    from arseg_amd import _lib, evaluation, ops

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\barseg_calibration_fwd\s*\(([^)]*)\)\s*;", code)
    assert m, "arseg_calibration_fwd is not declared in arseg_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert hasattr(lib, "arseg_calibration_fwd") and len(args) == len(_lib.PROTOTYPES["arseg_calibration_fwd"][1]) == 15
    assert args[:4] == ["const float *logits", "const int64_t *label", "const int32_t *group", "int64_t *cal"] and args[-1] == "arseg_stream_t stream"
    assert [a.split()[-1] for a in args[4:14]] == ["N", "n_groups", "n_cls", "h", "w", "H", "W", "ignore_label", "align_corners", "kind"]
    res, argtypes = _lib.PROTOTYPES["arseg_calibration_fwd"]
    assert res is ctypes.c_int and argtypes[:4] == [ctypes.c_void_p] * 4 and argtypes[4:14] == [ctypes.c_int] * 10
    assert sorted(set(re.findall(r"\b(arseg_\w+)\s*\(", code))) == sorted(_lib.PROTOTYPES)
    assert lib.arseg_version() == _lib.ABI_VERSION == 5 and "#define ARSEG_ABI_VERSION 5" in text
    block = text[text.index("Calibration counts (csrc/calibration.hip)"):text.index("int arseg_calibration_fwd")]
    for phrase in ("Not covered", "NLL / Brier", "entropy", "temperature fitting", "Link to the tail", "sum_q cal[g][k][q][0] == sum_l hist[g][l][k]",
                   "sum_q cal[g][k][q][1] == hist[g][k][k]", "q = 0", "ACCUMULATED", "no workspace"):
        assert phrase in block, phrase
    assert "calibration.hip" in open(os.path.join(ROOT, "ar-seg_amd", "csrc", "Makefile")).read()
    assert callable(ops.calibration)
    for n in ("calibration_numpy", "alter_res_batch_calibration", "EvalByCalibration", "CalibrationTable"):
        assert callable(getattr(evaluation, n)), n


def test_the_kernels_call_the_one_label_rule_and_its_softmax():
    """Class and code come from arseg_device.h: the kernels hand ArsegSoftmaxAcc to the label rule and ask it for the code; no exponential,
    reciprocal or rounding of their own, and no inline assembly."""
    src = open(os.path.join(ROOT, "ar-seg_amd", "csrc", "calibration.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert code.count("arseg_label_pixel(") == 1 and code.count("arseg_label_run<S>(") == 1
    assert "ArsegSoftmaxAcc<1> acc" in code and "ArsegSoftmaxAcc<S> acc" in code and code.count(".code(") == 2
    for word in ("expf", "rcpf", "floorf", "asm", "softmax("):
        assert word not in code, word
    assert code.count("hipLaunchKernelGGL(") == 4 and "hipMalloc" not in code and "Synchronize" not in code


def test_no_cpu_fallback_and_python_side_checks():
    from arseg_amd import _lib, ops

    logits, label = torch.zeros((2, 3, 4, 4)), torch.zeros((2, 4, 4), dtype=torch.int64)
    with pytest.raises(_lib.ArsegError):
        ops.calibration(logits, label, 4, 4)
    with pytest.raises(_lib.ArsegError):
        ops.calibration(logits, label, 4, 4, groups=[0, 1], n_groups=2, kind="margin")
    with pytest.raises(ValueError):
        ops.calibration(logits, label, 4, 4, kind="entropy")
    with pytest.raises(ValueError):
        ops.calibration(logits, label, 4, 4, n_groups=2)                            # no groups for two tables
    with pytest.raises(ValueError):
        ops.calibration(logits, label, 4, 4, groups=[0, 5], n_groups=2)             # a group id outside the range
    with pytest.raises(ValueError):
        ops.calibration(logits, label, 4, 4, groups=[0, 0], n_groups=0)


def test_documents_describe_the_calibration_table():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.19" in design and design.index("### 6.19") > design.index("### 6.18")
    section = design[design.index("### 6.19"):]
    for heading in ("Why", "Contract", "Kernels", "Host layers", "Tests", "Measured", "Not covered"):
        assert f"**{heading}" in section, heading
    for word in ("hot bin", "flush", "VGPRs", "Occupancy", "NLL", "temperature"):
        assert word in section, word
    assert "EvalByCalibration" in open(os.path.join(ROOT, "README.md")).read()
    assert "EvalByCalibration" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
