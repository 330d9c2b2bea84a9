"""The accuracy bounds of tests/creff_accuracy.py, proven on the CPU: on every (case, distribution, gain, head) of the GPU table the emulation
of the correct split-fp16 CReFF arithmetic passes its bound and the plain float32 loop is float32 arithmetic; every seeded defect (the low
half of K, V, P, Q or Wf lost, a cross term of the scores dropped) fails the bound where this file says it does, by at least twice the
largest margin; beyond the range ("over") and on the fp16 floor ("low") the correct emulation is inside the bound the format gives and a lost
low half of V is outside it.  Nothing here launches.  ``pytest -s`` shows the figures."""
import functools

import pytest
import torch

import creff_accuracy as ca

ALL = [(c.id, d, g) for c in ca.CASES for d in ca.DISTS for g in ca.GAINS]

# Where each defect has to fail: (case, distribution, gain, head).  DK, DQ and DX on every in-range distribution of w64, both gains, every output.
_W64_IN_RANGE = [("w64", d, g, n) for d in ca.IN_RANGE for g in ca.GAINS for n in ca.HEADS]
FAILS = {
    "DK": _W64_IN_RANGE + [("w128", "normal", 0.35, 0), ("f64", "high", 1.0, 19)],
    "DQ": _W64_IN_RANGE + [("w128", "high", 0.35, 12), ("f64", "normal", 0.35, 0)],
    "DX": _W64_IN_RANGE + [("f64", "high", 0.35, 0)],
    # "low": DV and DP on p and on the raw 19-class logits of every case and gain, DV also behind log_softmax at gain 1.0
    "DV": [("w64", d, g, n) for d in ("normal", "high") for g in ca.GAINS for n in ca.HEADS] + [("w128", "wide", 1.0, 0), ("f64", "normal", 1.0, 12)]
          + [(c.id, d, g, 0) for c in ca.CASES for d in ("low", "over") for g in ca.GAINS]
          + [(c.id, "low", g, 19) for c in ca.CASES for g in ca.GAINS] + [(c.id, "low", 1.0, 12) for c in ca.CASES],
    "DP": [("w64", d, g, n) for d in ("normal", "high") for g in ca.GAINS for n in ca.HEADS] + [("w128", "normal", 1.0, 0), ("f64", "high", 1.0, 19)]
          + [(c.id, "low", g, n) for c in ca.CASES for g in ca.GAINS for n in (0, 19)],
    "DW": [(c.id, d, g, n) for c in ca.CASES for d in ("normal", "high", "low") for g in ca.GAINS for n in (12, 19)],
}


@functools.lru_cache(maxsize=None)
def emulated(case_id, dist, gain, defect=None, clamp=False, descending=False):
    return ca.emulate(case_id, dist, gain, defect, clamp, descending)


def judged(case_id, dist, gain, n_cls, defect=None, clamp=False, m=None, descending=False):
    """(e, e32, what is wrong) of an emulated output under the bound of its distribution (m None: see below)"""
    y = ca.yardstick(case_id, dist, gain, clamp)
    floor = ca.low_floor(case_id, gain, n_cls) if dist == "low" else 0.0
    if m is None:          # in range: the largest margin of the case (a defect has to beat it twice over); "low", "over": the output's own
        m = ca.max_margin(case_id) if dist in ca.IN_RANGE else ca.margin(case_id, dist, gain, "", n_cls)
    e, prob = ca.problem(dist, emulated(case_id, dist, gain, defect, clamp, descending)[n_cls], y.want[n_cls], y.e32[n_cls], m, floor, clamp)
    return e, y.e32[n_cls], prob


@pytest.mark.parametrize("case_id,dist,gain", ALL)
def test_correct_emulation_passes_every_bound(case_id, dist, gain):
    """... with the channel chunks of the scores in either order: a correct kernel may use any."""
    y = ca.yardstick(case_id, dist, gain)
    for n in ca.HEADS:
        m = ca.margin(case_id, dist, gain, "", n)
        assert 2e-8 <= y.e32[n] <= 3e-4, (n, y.e32[n])                   # float32 arithmetic, not something coarser or an exact copy
        for desc in (False, True):
            e, e32, prob = judged(case_id, dist, gain, n, m=m, descending=desc)
            print(f"{case_id:5s} {dist:6s} {gain:4g} head {n:2d}: e32 = {e32:.3g}, correct emulation{' (descending)' if desc else ''} e = {e:.3g} = {e / e32:5.2f} x e32 {prob}")
            assert not prob, (n, desc, prob)
    if dist == "over":                                                   # the same call on the feature clamped to +-65504: the in-range bound
        for n in ca.HEADS:
            m = ca.margin(case_id, dist, gain, "", n)
            e, e32, prob = judged(case_id, dist, gain, n, clamp=True, m=m)
            print(f"{case_id:5s} clamped {gain:4g} head {n:2d}: e = {e:.3g} = {e / e32:5.2f} x e32 {prob}")
            assert not prob and e <= m * e32, (n, prob)


@pytest.mark.parametrize("defect", ca.DEFECTS)
def test_seeded_defect_fails_where_named(defect):
    """... by at least twice the largest margin of the case on the in-range distributions: no margin may be raised to half a defect's ratio."""
    assert set(FAILS) == set(ca.DEFECTS)
    for case_id, dist, gain, n in FAILS[defect]:
        e, e32, prob = judged(case_id, dist, gain, n, defect)
        print(f"{defect} {case_id:5s} {dist:6s} {gain:4g} head {n:2d}: e = {e:.3g} = {e / e32:7.1f} x e32  {prob}")
        assert prob, (defect, case_id, dist, gain, n, e / e32)
        if dist in ca.IN_RANGE:
            assert e >= 2.0 * ca.max_margin(case_id) * e32, (defect, case_id, dist, gain, n, e / e32)
        assert not judged(case_id, dist, gain, n)[2]                    # ... where the correct arithmetic passes


def test_low_floor_is_the_formats():
    """p and the logits behind log_softmax: 2^-24 (1 + 49 max|v|) and nothing else.  Raw logits: that plus 2^-24 times the larger one-signed
    part of the head's gain (between 0.5 and 0.85 of sum |wf|) and 2^-24 sum |p|; the correct emulation needs the addition (it is outside the
    bare term) and uses less than half of the bound with it."""
    for c in ca.CASES:
        for g in ca.GAINS:
            y = ca.yardstick(c.id, "low", g)
            assert 2e-3 <= y.vmax <= 5e-2, y.vmax
            fp = ca.FLOOR * (1.0 + 49.0 * y.vmax)
            assert ca.low_floor(c.id, g, 0) == fp and ca.low_floor(c.id, g, 12) == fp and fp <= 3 * ca.FLOOR
            l1 = float(ca.inputs(c.id, "low", g)["heads"][19][0].double().abs().sum(dim=1).max())
            psum = float(y.want[0].abs().sum(dim=1).max())
            assert fp + ca.FLOOR * (0.5 * l1 + psum) <= ca.low_floor(c.id, g, 19) <= fp + ca.FLOOR * (0.85 * l1 + psum)
            want, got = y.want[19], emulated(c.id, "low", g)[19]
            err, base = float((got.double() - want).abs().max()), ca.MARGIN * y.e32[19] * float(want.abs().max())
            assert base + fp < err <= 0.5 * (base + ca.low_floor(c.id, g, 19)), (err, base, fp)


def test_over_is_finite_clamps_and_needs_its_term():
    """Beyond 131008 the split clamps (never an infinity); the 2^-10 term is needed -- the in-range bound alone fails the correct arithmetic
    there -- and is not what lets a defect through: DV is outside by a factor of hundreds (test_seeded_defect_fails_where_named)."""
    hi, lo = ca.split_f16([2.0e5, -2.0e5, 98304.0 + 31.0])
    assert [float(hi[i]) + float(lo[i]) for i in range(3)] == [ca.LO_MAX, -ca.LO_MAX, 98304.0]
    for c in ca.CASES:
        y = ca.yardstick(c.id, "over", 0.35)
        got = emulated(c.id, "over", 0.35)
        assert all(bool(torch.isfinite(got[n]).all()) for n in ca.HEADS)
        assert ca.stat(got[0], y.want[0]) > ca.max_margin(c.id) * y.e32[0]


def test_every_margin_above_the_default_states_its_reason_and_is_needed_by_the_correct_arithmetic():
    """A larger margin has a written reason, the CPU emulation of the correct arithmetic exceeds the default on that case (in one of the two
    chunk orders: the excess is inherent, no kernel is involved), and it stays below half the smallest ratio a seeded defect gives where
    this file says the defect fails on that case."""
    assert ca.MARGIN == 4.0
    for key, (m, reason) in list(ca.CASE_MARGINS.items()) + list(ca.ROUTE_MARGINS.items()):
        assert m > ca.MARGIN and len(reason) > 20, key
        assert key[0] in list(ca.BY_ID) + ["*"], key
    for (case_id, dist, gain), (m, _) in ca.CASE_MARGINS.items():
        assert dist in ca.IN_RANGE and gain in ca.GAINS
        ratios = [judged(case_id, dist, gain, n, descending=desc)[0] / ca.yardstick(case_id, dist, gain).e32[n] for n in ca.HEADS for desc in (False, True)]
        assert ca.MARGIN < max(ratios) <= m, ratios
        named = [judged(c, d, g, n, defect)[:2] for defect, where in FAILS.items() for c, d, g, n in where if c == case_id and d in ca.IN_RANGE]
        assert named and m <= 0.5 * min(e / e32 for e, e32 in named), (m, min(e / e32 for e, e32 in named))
