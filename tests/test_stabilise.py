"""CPU-side checks of the keyframe prior (arseg_segment_stabilise_fwd, egress.stabilise): that every seeded input of
tests/test_gpu_stabilise.py exercises all seven outcomes and stays under the band cap of the comparison rule, the oracle's own invariants
and hand-made edge cases (tests/stabilise_oracle.py), egress.hold_bonus and egress.hold_table against hand-computed values, the host layer's
argument checks and the argument validation of the entry point, which happens before any launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import stabilise_oracle as oracle


@pytest.fixture(scope="module")
def solved():
    cache = {}

    def get(case):
        if case[0] not in cache:
            cache[case[0]] = oracle.solve(case)
        return cache[case[0]]
    return get


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_seeded_inputs_are_spread_over_all_outcomes_and_stay_under_the_band_cap(solved, case):
    """Per frame of every case the GPU file compares on, with both gates on and the median thresholds: HELD, OWN and AGREE are each at least
    2 % of the pixels and each of the four no-prior outcomes at least 1 %; at most 0.5 % of a case's pixels lie within BAND of beta."""
    b, o = solved(case)
    H, W = case[6], case[7]
    share = o["stats"][:, :7] / float(H * W)
    print(f"\n{case[0]}: beta {b['beta'].tolist()}, band {100 * o['band'].mean():.4f} %; shares per frame (%) "
          f"{[dict(zip(oracle.OUTCOMES, np.round(100 * s, 1).tolist())) for s in share]}")
    assert o["band"].mean() <= oracle.BAND_CAP
    assert (share[:, [oracle.HELD, oracle.OWN, oracle.AGREE]] >= 0.02).all()
    assert (share[:, [oracle.UNLINKED, oracle.OUTSIDE, oracle.VOID, oracle.WEAK]] >= 0.01).all()
    assert np.isfinite(b["beta"]).all() and (b["beta"] > 0).all()


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.CASE_IDS)
def test_oracle_invariants(solved, case):
    """The seven counts sum to H W; sum into == sum from == held; the planes and the counters say the same; beta = 0 gives the plain labels;
    beta = +inf holds every differing pixel with a prior, without a NaN anywhere; the gates switched off move their pixels elsewhere."""
    b, o = solved(case)
    N, n_cls, H, W = case[2], case[3], case[6], case[7]
    s = o["stats"]
    assert s.dtype == np.int64 and s.shape == (N, oracle.ST_NSTATS) and oracle.ST_NSTATS == 72
    assert (s[:, :7].sum(axis=1) == H * W).all() and not s[:, 7].any()
    assert (s[:, oracle.INTO:oracle.INTO + 32].sum(axis=1) == s[:, oracle.HELD]).all()
    assert (s[:, oracle.FROM:oracle.FROM + 32].sum(axis=1) == s[:, oracle.HELD]).all()
    assert not s[:, oracle.INTO + n_cls:oracle.FROM].any() and not s[:, oracle.FROM + n_cls:].any()
    for code, which in ((0, [oracle.AGREE]), (255, [oracle.HELD]), (192, [oracle.OWN]), (128, [0, 1, 2, 3])):
        assert ((o["hold"] == code).sum(axis=(1, 2)) == s[:, which].sum(axis=1)).all()
    assert set(np.unique(o["hold"])) == {0, 128, 192, 255}
    held = o["outcome"] == oracle.HELD
    assert np.array_equal(o["labels"][held], o["pre"][held]) and np.array_equal(o["labels"][~held], o["kstar"][~held])
    assert (o["pre"][held] != o["kstar"][held]).all()
    gates = (b["link"], oracle.LINK_MASK, b["conf"], oracle.REF_LOW)
    zero = oracle.stabilise(b["values"], b["ref"], b["mv"], np.zeros(N, dtype=np.float32), *gates)
    assert np.array_equal(zero["labels"], zero["kstar"]) and not zero["stats"][:, oracle.HELD].any() and not zero["stats"][:, oracle.INTO:].any()
    assert np.array_equal(zero["stats"][:, :5], s[:, :5]) and (zero["stats"][:, oracle.OWN] == s[:, oracle.HELD] + s[:, oracle.OWN]).all()
    inf = oracle.stabilise(b["values"], b["ref"], b["mv"], np.full(N, np.inf, dtype=np.float32), *gates)
    assert not inf["stats"][:, oracle.OWN].any() and (inf["stats"][:, oracle.HELD] == s[:, oracle.HELD] + s[:, oracle.OWN]).all()
    assert not np.isnan(inf["d"]).any() and np.array_equal(inf["labels"][inf["pre"] >= 0], inf["pre"][inf["pre"] >= 0])
    lut = np.arange(100, 100 + n_cls, dtype=np.uint8)
    assert np.array_equal(oracle.stabilise(b["values"], b["ref"], b["mv"], b["beta"], *gates, lut=lut)["labels"], o["labels"] + 100)
    off = oracle.stabilise(b["values"], b["ref"], b["mv"], b["beta"])
    assert not off["stats"][:, oracle.UNLINKED].any() and not off["stats"][:, oracle.WEAK].any()
    assert np.array_equal(off["stats"], oracle.stabilise(b["values"], b["ref"], b["mv"], b["beta"], b["link"], 0, b["conf"], 0)["stats"])
    clamped = oracle.stabilise(b["values"], b["ref"], b["mv"], b["beta"], b["link"], oracle.LINK_CLAMPED)
    assert (clamped["stats"][:, oracle.UNLINKED] > 0).all()


def _one_pixel(v, ref_class, beta, n_cls=None):
    """One frame of one pixel with the class values ``v``, a zero vector and a reference pixel of class ``ref_class`` -> its outcome."""
    v = np.asarray(v, dtype=np.float32).reshape(1, -1, 1, 1)
    ref = np.full((1, 1, 1), ref_class, dtype=np.uint8)
    o = oracle.stabilise(v, ref, np.zeros((1, 1, 1, 2), dtype=np.int16), np.array([beta], dtype=np.float32))
    return int(o["outcome"][0, 0, 0]), int(o["labels"][0, 0, 0])


def test_hand_made_cases():
    """d == beta exactly is OWN (the comparison is strict), just below it HELD; a NaN logit, all -inf pixels and a NaN beta never hold; the
    first maximum is k* and a later equal value is held by any positive beta; n_cls == 1 never holds; the order of the no-prior outcomes."""
    inf, nan = float("inf"), float("nan")
    assert _one_pixel([3.0, 1.5, 0.0], 1, 1.5) == (oracle.OWN, 0)                      # d = 1.5 == beta
    assert _one_pixel([3.0, 1.5, 0.0], 1, float(np.nextafter(np.float32(1.5), np.float32(2)))) == (oracle.HELD, 1)
    assert _one_pixel([3.0, 1.5, 0.0], 2, 2.9) == (oracle.OWN, 0) and _one_pixel([3.0, 1.5, 0.0], 2, 3.1) == (oracle.HELD, 2)
    assert _one_pixel([3.0, 1.5, 0.0], 0, 100.0) == (oracle.AGREE, 0)
    assert _one_pixel([3.0, 1.5, 0.0], 1, 0.0) == (oracle.OWN, 0) and _one_pixel([3.0, 1.5, 0.0], 1, -1.0) == (oracle.OWN, 0)
    assert _one_pixel([2.0, 2.0, 0.0], 1, 1e-30) == (oracle.HELD, 1)                   # a tie: the first maximum is k*, d = 0 < beta
    assert _one_pixel([2.0, 2.0, 0.0], 1, 0.0) == (oracle.OWN, 0)
    assert _one_pixel([1.0, nan, 5.0], 0, inf) == (oracle.OWN, 1)                      # k* is the NaN's class; NaN - 1 is NaN: not held
    assert _one_pixel([1.0, nan, 5.0], 1, inf) == (oracle.AGREE, 1)
    assert _one_pixel([nan, 1.0, 5.0], 2, inf) == (oracle.OWN, 0)
    assert _one_pixel([-inf, -inf, -inf], 2, inf) == (oracle.OWN, 0)                   # -inf - -inf is NaN; k* of an all -inf pixel is 0
    assert _one_pixel([-inf, -inf, -inf], 0, inf) == (oracle.AGREE, 0)
    assert _one_pixel([inf, inf, 0.0], 1, inf) == (oracle.OWN, 0)                      # +inf - +inf
    assert _one_pixel([inf, 1.0, 0.0], 1, inf) == (oracle.OWN, 0)                      # d = +inf is not below +inf
    assert _one_pixel([3.0, 1.5, 0.0], 1, nan) == (oracle.OWN, 0)                      # a NaN beta holds nothing
    assert _one_pixel([3.0, 1.5, 0.0], 3, inf) == (oracle.VOID, 0) and _one_pixel([3.0, 1.5, 0.0], 255, inf) == (oracle.VOID, 0)
    assert _one_pixel([0.7], 0, inf) == (oracle.AGREE, 0) and _one_pixel([0.7], 1, inf) == (oracle.VOID, 0)        # n_cls == 1
    assert _one_pixel([nan], 0, inf) == (oracle.AGREE, 0)
    # the order: unlinked before outside before void before weak
    ref, conf = np.array([[[1, 255]]], dtype=np.uint8), np.array([[[10, 10]]], dtype=np.uint8)
    v = np.zeros((1, 3, 1, 2), dtype=np.float32)
    v[0, 0] = 1.0
    beta = np.array([5.0], dtype=np.float32)
    for mvx, link, want in ((0, 0, oracle.WEAK), (4, 0, oracle.VOID), (8, 0, oracle.OUTSIDE), (8, 1, oracle.UNLINKED), (4, 2, oracle.UNLINKED)):
        mv = np.zeros((1, 1, 2, 2), dtype=np.int16)
        mv[0, 0, 0, 0] = mvx
        o = oracle.stabilise(v, ref, mv, beta, np.full((1, 1, 2), link, dtype=np.uint8), 3, conf, 11)
        assert o["outcome"][0, 0, 0] == want
    o = oracle.stabilise(v, ref, np.zeros((1, 1, 2, 2), dtype=np.int16), beta, None, 0, conf, 10)          # code 10 is not below 10
    assert o["outcome"][0, 0].tolist() == [oracle.HELD, oracle.VOID] and o["labels"][0, 0].tolist() == [1, 0]
    assert oracle.label_rule(np.array([1.0, nan, nan, 9.0]).reshape(1, 4, 1, 1))[0, 0, 0] == 1


def test_hold_bonus_against_hand_computed_values():
    import torch

    from arseg_amd import egress

    b = egress.hold_bonus([0, 1, 2, 4, 11], 2.0, 2.0)
    assert b.dtype == torch.float32 and tuple(b.shape) == (5,)
    assert b.tolist() == [2.0, np.float32(2.0 ** 0.5), 1.0, 0.5, np.float32(2.0 * 2.0 ** -5.5)]
    assert egress.hold_bonus(3, 1.5, 3.0).tolist() == [0.75] and egress.hold_bonus([], 1.0, 1.0).numel() == 0
    assert egress.hold_bonus([0, 7], 0.0, 1.0).tolist() == [0.0, 0.0]
    assert egress.hold_bonus(np.arange(3), 1.0, 1.0).tolist() == [1.0, 0.5, 0.25]
    for bad in (([-1], 1.0, 1.0), ([0], -0.5, 1.0), ([0], 1.0, 0.0), ([0], 1.0, -2.0), ([0], float("nan"), 1.0), ([0], 1.0, float("inf")),
                ([float("nan")], 1.0, 1.0), ([[0, 1]], 1.0, 1.0)):
        with pytest.raises(ValueError):
            egress.hold_bonus(*bad)


def test_hold_table_against_hand_computed_rows():
    from arseg_amd import _lib, egress

    rows = np.zeros((3, _lib.ST_NSTATS), dtype=np.int64)
    rows[0, :7] = (10, 20, 5, 5, 100, 45, 15)                               # 200 pixels; 60 differ, 45 of them held
    rows[0, 8:11], rows[0, 40:43] = (30, 15, 0), (5, 0, 40)
    rows[1, :7] = (0, 0, 0, 0, 50, 0, 0)                                    # nothing differs
    t = egress.hold_table(rows, 3)
    assert set(t) == {"shares", "held_of_differing", "into", "from"} and tuple(t["shares"]) == egress.HOLD_OUTCOMES == oracle.OUTCOMES
    got = [t["shares"][k][0] for k in egress.HOLD_OUTCOMES]
    assert got == pytest.approx([0.05, 0.1, 0.025, 0.025, 0.5, 0.225, 0.075])
    assert t["held_of_differing"][0] == pytest.approx(0.75) and math.isnan(t["held_of_differing"][1]) and t["shares"]["agree"][1] == 1.0
    assert math.isnan(t["held_of_differing"][2]) and all(math.isnan(t["shares"][k][2]) for k in egress.HOLD_OUTCOMES)          # an empty row
    assert t["into"].tolist() == [[30, 15, 0], [0, 0, 0], [0, 0, 0]] and t["from"].tolist() == [[5, 0, 40], [0, 0, 0], [0, 0, 0]]
    assert t["into"].dtype == np.int64 and t["into"].shape == (3, 3)
    import torch

    one = egress.hold_table(torch.from_numpy(rows[0]), 3)
    assert one["held_of_differing"].shape == (1,) and one["held_of_differing"][0] == pytest.approx(0.75)
    with pytest.raises(ValueError):
        egress.hold_table(rows[:, :50], 3)
    with pytest.raises(ValueError):
        egress.hold_table(rows, 33)


def test_host_layer_argument_checks():
    """ArsegError for CPU tensors (no CPU fallback), ValueError for malformed arguments, before anything touches a GPU."""
    import torch

    from arseg_amd import _lib, egress, evaluation, ops

    logits = torch.zeros((1, 12, 4, 6))
    ref, mv = torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((1, 4, 6, 2), dtype=torch.int16)
    with pytest.raises(_lib.ArsegError):
        egress.stabilise(logits, ref, mv, 4, 6, 1.0)
    with pytest.raises(_lib.ArsegError):
        ops.segment_stabilise(logits, ref[None], mv, 4, 6, torch.zeros(1), stats=torch.zeros((1, _lib.ST_NSTATS), dtype=torch.int64))
    with pytest.raises(ValueError):
        egress.stabilise(torch.zeros((12, 4, 6)), ref, mv, 4, 6, 1.0)
    with pytest.raises(ValueError):
        egress.stabilise(logits, torch.zeros((1, 1, 4, 6), dtype=torch.uint8), mv, 4, 6, 1.0)
    with pytest.raises(ValueError):
        egress.stabilise(logits, ref, mv, 4, 6, 1.0, ref_conf=torch.zeros((1, 1, 4, 6), dtype=torch.uint8))
    assert _lib.ST_NSTATS == 72 == oracle.ST_NSTATS and (_lib.LINK_INTRA | _lib.LINK_UNCOVERED) == oracle.LINK_MASK
    assert callable(evaluation.alter_res_batch_stabilised)


def test_entry_point_is_declared_and_abi_version_stays_5():
    from conftest import ROOT

    from arseg_amd import _lib

    header = open(os.path.join(ROOT, "include", "arseg_hip.h")).read()
    m = re.search(r"\bint arseg_segment_stabilise_fwd\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == len(_lib.PROTOTYPES["arseg_segment_stabilise_fwd"][1]) == 30
    assert _lib.PROTOTYPES["arseg_segment_stabilise_fwd"][1][:12] == _lib.PROTOTYPES["arseg_segment_consistency_fwd"][1][:12]
    assert re.search(r"#define ARSEG_ST_NSTATS \(8 \+ 2 \* 32\)", header) and re.search(r"#define ARSEG_ABI_VERSION 5\b", header)
    lib = _lib.load()
    assert hasattr(lib, "arseg_segment_stabilise_fwd") and lib.arseg_version() == _lib.ABI_VERSION == 5


def test_documents_describe_the_pass():
    """DESIGN.md section 6.24 (with its resource table: no scratch), README.md and INTEGRATION.md describe the pass; the benchmark tool is there."""
    from conftest import ROOT

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 6.24"):design.index("## 7. Multi-GPU")]
    for kernel in ("stabilise_pixel_kernel", "stabilise_run_kernel<2>", "stabilise_run_kernel<4>", "stabilise_run_kernel<8>"):
        assert re.search(r"\| `" + re.escape(kernel) + r"`[^|]*\| \d+ \| \d+ \| \d+ \| \d+ \| 0 \|", section), kernel
    assert "arseg_segment_stabilise_fwd" in section and "Measured" in section and "byte-identical" in section
    assert "egress.stabilise" in open(os.path.join(ROOT, "README.md")).read()
    assert "alter_res_batch_stabilised" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_stabilise.py"))


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every ARSEG_EINVAL case of the contract comes back before any launch (device pointers are dummies and never dereferenced)."""
    from arseg_amd import _lib

    lib = _lib.load()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(66)
    EINVAL = _lib.ARSEG_EINVAL
    H, W = 32, 48
    lut = (ctypes.c_uint8 * 32)(*range(32))

    def st(logits=one, N=2, n_cls=19, h=4, w=6, H=H, W=W, align=0, ref=one, ref_pitch=W, ref_ns=0, mv=one, bonus=one, link=one, link_pitch=W,
           link_ns=H * W, link_mask=3, conf=one, conf_pitch=W, conf_ns=0, ref_low=128, lut=lut, lab=one, lab_pitch=W, lab_ns=H * W, hold=one,
           hold_pitch=W, hold_ns=H * W, stats=one):
        return lib.arseg_segment_stabilise_fwd(logits, N, n_cls, h, w, H, W, align, ref, ref_pitch, ref_ns, mv, bonus, link, link_pitch, link_ns,
                                               link_mask, conf, conf_pitch, conf_ns, ref_low, lut, lab, lab_pitch, lab_ns, hold, hold_pitch,
                                               hold_ns, stats, null)

    assert st(logits=null) == EINVAL and st(ref=null) == EINVAL and st(mv=null) == EINVAL          # null logits / ref_labels / mv_q
    assert st(mv=odd) == EINVAL                                                                    # mv_q not 4-byte aligned
    assert st(bonus=null) == EINVAL and st(bonus=odd) == EINVAL                                    # a null (or misaligned) bonus
    for bad in (0, -1, 33):
        assert st(n_cls=bad) == EINVAL and st(n_cls=bad, hold=null) == EINVAL                      # n_cls outside 1 .. 32
    for name in ("N", "H", "W", "h", "w"):
        assert st(**{name: 0}) == EINVAL and st(**{name: -3}) == EINVAL                            # a non-positive size
    for name in ("ref_pitch", "lab_pitch", "hold_pitch", "link_pitch", "conf_pitch"):
        assert st(**{name: W - 1}) == EINVAL                                                       # a pitch below W
    assert st(hold_pitch=W - 1, stats=null) == EINVAL and st(lab_pitch=W - 1, hold=null, stats=null) == EINVAL
    for name in ("ref_ns", "lab_ns", "hold_ns", "link_ns", "conf_ns"):
        assert st(**{name: -1}) == EINVAL                                                          # a negative stride
    for bad in (-1, 257):
        assert st(ref_low=bad) == EINVAL and st(ref_low=bad, conf=null) == EINVAL                  # ref_low outside 0 .. 256
    assert st(lab=null, hold=null, stats=null) == EINVAL                                           # no output at all
    for align in (0, 1):                                                                           # the run route (x8 here) and the per-pixel route alike
        assert st(align=align, conf_pitch=W - 1) == EINVAL and st(align=align, bonus=null) == EINVAL
        assert st(align=align, lab=null, hold=null, stats=null) == EINVAL
