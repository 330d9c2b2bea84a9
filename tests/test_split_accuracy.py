"""The accuracy bound of tests/split_accuracy.py, proven on the CPU: on every case of the GPU table the emulation of the correct split-fp16
arithmetic passes it with room, each seeded defect fails it by a factor of three or more, torch's float32 passes, the Winograd emulation
passes its own bound and a seeded GEMM of it fails -- and the older absolute tolerance lets a seeded defect through.  Nothing here launches."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import split_accuracy as sa

ALL = [(c.id, d) for c in sa.CASES for d in sa.DISTS]
WINO = [(c.id, d) for c in sa.CASES if sa.has_wino(c) for d in sa.DISTS]


@functools.lru_cache(maxsize=None)
def emulated(case_id, dist, defect=None):
    return sa.stat(sa.emulate(case_id, sa.inputs(case_id, dist), defect), sa.yardstick(case_id, dist)[0])


@functools.lru_cache(maxsize=None)
def wino_emulated(case_id, dist, defect=None):
    return sa.stat(sa.wino(case_id, sa.inputs(case_id, dist), True, defect), sa.yardstick(case_id, dist)[0])


def test_rtz_split_is_the_kernels():
    """hi = the 11 leading bits, never rounded up and never infinite; hi + lo holds 22 bits; fp16-subnormal lo halves degrade to 2^-24 absolute."""
    x = np.array([1.0 + 2.0 ** -11 + 2.0 ** -12, -(1.0 + 2.0 ** -11 + 2.0 ** -12), 65519.0, 1e5, 3.0e-6, 0.0, 2049.0, -2049.0], dtype=np.float32)
    hi, lo = sa.split_f16(x)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    assert list(hi[:4].astype(np.float64)) == [1.0, -1.0, 65504.0, 65504.0]          # round to nearest would give 1 + 2^-10 and inf
    assert float(hi[6]) == 2048.0 and float(hi[7]) == -2048.0 and float(lo[6]) == 1.0 and float(lo[7]) == -1.0
    g = np.random.Generator(np.random.PCG64(5))
    v = (g.standard_normal(4096) * np.exp(g.uniform(-7, 4.6, 4096))).astype(np.float32)
    hi, lo = sa.split_f16(v)
    assert bool((np.abs(hi.astype(np.float32)) <= np.abs(v)).all())
    rest = v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert bool((np.abs(rest) <= np.maximum(2.0 ** -21 * np.abs(v), 2.0 ** -24)).all()) and bool((rest * v >= 0).all())      # one-sided


@pytest.mark.parametrize("case_id", ["c", "e", "p"])
def test_weight_split_is_the_host_packers(case_id):
    """The emulation's weight halves are, bit for bit, what arseg_split_weight_f16x3_host writes (per 32 k: 32 hi halves, then 32 lo), and its
    per-channel power of two the one that function folds into the scale."""
    from arseg_amd import _lib

    B = np.ascontiguousarray(sa.pack_weight(sa.inputs(case_id, "normal")["w"]), dtype=np.float32)
    cout, kpad = B.shape
    out, mul_inv = np.empty((cout, kpad), dtype=np.float32), np.empty(cout, dtype=np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    _lib.check(_lib.load().arseg_split_weight_f16x3_host(P(B), cout, kpad, P(out), P(mul_inv)), "split_weight_f16x3")
    exps = sa.weight_exponents(B)
    assert np.array_equal(mul_inv, np.ldexp(np.float32(1.0), -exps))
    hi, lo = sa.split_f16(np.ldexp(B, exps[:, None]))
    halves = out.view(np.uint16).reshape(cout, kpad // 32, 2, 32)
    assert np.array_equal(halves[:, :, 0], hi.view(np.uint16).reshape(cout, kpad // 32, 32))
    assert np.array_equal(halves[:, :, 1], lo.view(np.uint16).reshape(cout, kpad // 32, 32))


@pytest.mark.parametrize("case_id,dist", ALL)
def test_correct_emulation_passes_with_room_and_fp32_passes(case_id, dist):
    want, e32 = sa.yardstick(case_id, dist)
    ins = sa.inputs(case_id, dist)
    assert 5e-8 <= e32 <= 1e-5, e32                                     # float32 arithmetic, not something coarser or an exact copy
    sa.check(sa.reference32(case_id, ins), want, e32, "the float32 loop", 1.0)
    sa.check(sa.reference(case_id, ins, torch.float32), want, e32, "torch float32", sa.MARGIN)
    e = emulated(case_id, dist)
    assert e <= 0.5 * sa.max_margin(case_id) * e32, f"correct emulation: e = {e:.3g} = {e / e32:.2f} x e32, margin {sa.max_margin(case_id):g}"
    sa.check(sa.emulate(case_id, ins), want, e32, "correct emulation", sa.margin(case_id, "tile"))


@pytest.mark.parametrize("case_id,dist", ALL)
def test_seeded_defects_fail_by_three(case_id, dist):
    """... which is also the condition on every margin: the bound stays at or below a third of the smallest error D1, D2, D3 give."""
    want, e32 = sa.yardstick(case_id, dist)
    bound = sa.max_margin(case_id) * e32
    errs = {d: emulated(case_id, dist, d) for d in sa.DEFECTS}
    assert bound <= min(errs[d] for d in ("D1", "D2", "D3")) / 3.0, (bound, errs)
    for d, e in errs.items():
        assert e >= 3.0 * bound, f"{d}: e = {e:.3g} < 3 x bound = {3 * bound:.3g}"
    with pytest.raises(AssertionError, match=r"D1: e = .* x e32"):
        sa.check(sa.emulate(case_id, sa.inputs(case_id, dist), "D1"), want, e32, "D1", sa.max_margin(case_id))


@pytest.mark.parametrize("case_id,dist", WINO)
def test_winograd_emulation_passes_its_own_bound_and_its_seeded_gemm_fails(case_id, dist):
    want, _ = sa.yardstick(case_id, dist)
    e32w = sa.wino_yardstick(case_id, dist)
    assert e32w <= 2e-5, e32w                                          # the float32 Winograd computes the same conv
    bound = sa.max_margin(case_id, wino=True) * e32w
    e = wino_emulated(case_id, dist)
    assert e <= bound, f"Winograd emulation: e = {e:.3g} = {e / e32w:.2f} x e32"
    seeded = wino_emulated(case_id, dist, "D1")
    assert bound <= seeded / 3.0, f"one seeded GEMM of 36: e = {seeded:.3g} < 3 x bound = {3 * bound:.3g}"


def test_every_margin_above_the_default_states_its_reason():
    for key, (m, reason) in list(sa.CASE_MARGINS.items()) + list(sa.ROUTE_MARGINS.items()):
        assert m > sa.MARGIN and len(reason) > 20, key
        assert (key if isinstance(key, str) else key[0]) in list(sa.BY_ID) + ["*"], key


def test_old_absolute_tolerance_cannot_tell_a_seeded_defect_from_a_correct_result():
    """Why 2e-4 absolute was not enough.  The K = 2304 case drawn as the older tests draw (unit normal activations, He-scaled weights without
    a channel gain): a correct result is at 6e-6, 30 times below that tolerance, and the activations' low half lost in a whole K step lands
    at 4.0e-4 -- the old tolerance stands within a factor of two of it, so that one draw of the inputs, a BN scale of 1 in place of 2, or
    the same loss in half a K step decides whether it is seen.  (With low halves rounded to nearest the loss would be half as large and pass;
    the kernels' split rounds toward zero, which makes the lost half one-sided and twice as large.)  The new bound sees it by a factor of ten."""
    ins = sa.inputs(sa.K2304, "normal", gain=False)
    want = sa.reference(sa.K2304, ins, torch.float64)
    e32 = sa.stat(sa.reference32(sa.K2304, ins), want)
    absmax = lambda got: float((got.double() - want).abs().max())      # noqa: E731
    ok, bad = sa.emulate(sa.K2304, ins), sa.emulate(sa.K2304, ins, "D1")
    assert absmax(ok) <= sa.OLD_TOL / 25
    assert absmax(bad) <= 2.5 * sa.OLD_TOL, absmax(bad)
    plain = dict(ins, bn=None, res=None)                               # the conv alone, without the epilogue's BN scale: 2.9e-4
    want_plain = sa.reference(sa.K2304, plain, torch.float64)
    assert float((sa.emulate(sa.K2304, plain, "D1").double() - want_plain).abs().max()) <= 1.5 * sa.OLD_TOL
    assert sa.stat(bad, want) >= 5 * sa.margin(sa.K2304, "tile") * e32            # (9.7 x the bound)
    sa.check(ok, want, e32, "correct emulation", sa.margin(sa.K2304, "tile"))


def test_the_table_reaches_every_plan():
    """The device-free plan query on the table's shapes: every id 1..23 and every split-K pair of test_conv2d is accepted on at least one
    conv case under f16x3, every id 0..12 under f32 (both distributions share the shapes)."""
    from arseg_amd import _lib

    cases = [c.id for c in sa.conv_cases()]
    for cfg in range(1, 24):
        assert any(sa.accepted(cid, cfg, 1, _lib.MATH_F16X3) for cid in cases), cfg
    for cfg, sk in sa.SPLIT_K_PAIRS:
        assert any(sa.accepted(cid, cfg, sk, _lib.MATH_F16X3) for cid in cases), (cfg, sk)
        assert sa.accepted(sa.K2304, cfg, sk, _lib.MATH_F16X3), (cfg, sk)
    for cid in cases:
        for cfg in range(0, 13):
            assert sa.accepted(cid, cfg, 0 if cfg == 0 else 1, _lib.MATH_F32), (cid, cfg)
    assert sa.accepted("i64", 23, 1, _lib.MATH_F16X3) and not sa.accepted("i96", 23, 1, _lib.MATH_F16X3)
    assert sa.accepted("h", 20, 1, _lib.MATH_F16X3) and not sa.accepted("b", 20, 1, _lib.MATH_F16X3)
    assert any(sa.has_wino(c) and c.up2 for c in sa.CASES) and any(sa.has_wino(c) and c.dil > 1 for c in sa.CASES)
    for c in sa.CASES:
        M = c.N * sa.out_hw(c)[0] * sa.out_hw(c)[1]
        assert M % 64, c.id                          # every case ends in a ragged pixel tile
