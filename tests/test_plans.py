"""The plan tuner (arseg_amd.ops._plans.tuned): cache, re-tuning, skipped candidates, untuned forms, plan-file round trip.
CPU only -- a fake launcher and timer stand in for the device."""
import pytest


@pytest.fixture
def plans(monkeypatch):
    """ops._plans with an empty cache, no plan file, the tuner on and no capture running; everything restored afterwards."""
    from arseg_amd import ops
    from arseg_amd.ops import _plans

    saved = dict(_plans._conv_plans)
    prev = ops.configure(conv_plan_file=None, conv_autotune=True)
    dict.clear(_plans._conv_plans)
    monkeypatch.setattr(_plans, "_capturing", lambda: False)
    yield _plans
    dict.clear(_plans._conv_plans)
    ops.configure(**prev)
    dict.clear(_plans._conv_plans)
    dict.update(_plans._conv_plans, saved)


def fake(times, raises=()):
    """(run, timer, launched): run(plan) records the plan, raises ArsegError for those in ``raises``; timer(f) calls f and returns times[plan]."""
    from arseg_amd import _lib

    launched = []

    def run(plan):
        if plan in raises:
            raise _lib.ArsegError(f"plan {plan} refused")
        launched.append(plan)

    def timer(f):
        f()
        return times[launched[-1]]

    return run, timer, launched


def test_cache_hit_times_nothing(plans):
    plans._conv_plans[("k", 1)] = (3, 1)
    run, timer, launched = fake({})
    assert plans.tuned(("k", 1), [(0, 0), (3, 1)], run, timer=timer) == (3, 1)
    assert launched == []


def test_rejected_plan_is_retuned(plans):
    plans._conv_plans[("k", 2)] = "rows"            # a route that no longer exists
    run, timer, launched = fake({(0, 0): 2.0, (5, 1): 1.0})
    assert plans.tuned(("k", 2), [(0, 0), (5, 1)], run, timer=timer, valid=lambda p: isinstance(p, tuple)) == (5, 1)
    assert launched == [(0, 0), (5, 1)] and plans._conv_plans[("k", 2)] == (5, 1)


def test_raising_candidates_are_skipped(plans):
    run, timer, _ = fake({1: 3.0, 3: 2.0}, raises=(0, 2))
    assert plans.tuned(("k", 3), range(4), run, timer=timer) == 3
    assert plans._conv_plans[("k", 3)] == 3


def test_nothing_launched_returns_none_uncached(plans):
    run, timer, _ = fake({}, raises=(0, 1, 2))
    assert plans.tuned(("k", 4), range(3), run, timer=timer) is None
    assert ("k", 4) not in plans._conv_plans


def test_first_of_equal_times_wins(plans):
    run, timer, _ = fake({"a": 1.0, "b": 1.0, "c": 2.0})
    assert plans.tuned(("k", 5), ["c", "a", "b"], run, timer=timer) == "a"


def test_margin_scales_one_candidate(plans):
    run, timer, _ = fake({(0, 0): 1.0, "wino": 0.9})
    assert plans.tuned(("k", 6), [(0, 0), "wino"], run, timer=timer, margin={"wino": 1.2}) == (0, 0)
    assert plans.tuned(("k", 7), [(0, 0), "wino"], run, timer=timer, margin={"wino": 1.0}) == "wino"


@pytest.mark.parametrize("why", ["autotune off", "capturing"])
def test_untuned_form_is_not_cached(plans, monkeypatch, why):
    from arseg_amd import ops

    if why == "autotune off":
        ops.configure(conv_autotune=False)
    else:
        monkeypatch.setattr(plans, "_capturing", lambda: True)
    run, timer, launched = fake({0: 1.0})
    assert plans.tuned(("k", 8), [0], run, timer=timer, untuned=9) == 9
    assert launched == [] and ("k", 8) not in plans._conv_plans
    # a site without an untuned form tunes regardless
    assert plans.tuned(("k", 9), [0], run, timer=timer) == 0


def test_plan_file_round_trip(plans, tmp_path):
    from arseg_amd import ops

    path = tmp_path / "plans.json"
    ops.configure(conv_plan_file=str(path))
    run, timer, _ = fake({(13, 1): 1.0, "wino": 2.0, 7: 1.0})
    assert plans.tuned((0, 1, 64, 64, "up2"), [(13, 1), "wino"], run, timer=timer) == (13, 1)
    plans._conv_plans[(0, 2, 32)] = "wino"
    assert plans.tuned(("wino_gemm", 0, 512), [7], run, timer=timer) == 7
    assert path.exists()
    dict.clear(plans._conv_plans)
    reloaded = plans._PlanCache()
    assert reloaded == {(0, 1, 64, 64, "up2"): (13, 1), (0, 2, 32): "wino", ("wino_gemm", 0, 512): 7}
    assert isinstance(reloaded[(0, 1, 64, 64, "up2")], tuple)
