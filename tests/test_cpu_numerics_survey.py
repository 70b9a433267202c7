"""CPU tier: a test of the test.  tests/numerics_survey.own_step_errors judges a traced fan on its own recorded steps
with the oracle's one-step entry; the GPU tier relies on it to find a trace loop that lost a step's accuracy, recorded a
point the reference would not have, or skipped / doubled a commit.  Here the traced fan comes from the host build of the
kernel sources (emul_lib.trace, which runs the hand-over and the resume kernel): on it every number is exactly 0; then
faults are planted in a COPY of the result (plain array edits on the host) and each must be found, and only where
it was planted."""
import numpy as np
import pytest

from tests import emul_lib
from tests.common import host_libm_is_the_variant_the_fixtures_were_cut_with, load_golden
from tests.numerics_survey import OUTSIDE_THE_STEP, own_step_errors

CASES = ["cfg2_solovev1024_rk4", "gold_solovev64_damp_rk4"]


@pytest.fixture(scope="module", params=CASES)
def traced(request):
    g, nml, p = load_golden(request.param)
    return p, emul_lib.trace(p, g["rvec0"], g["rindex_vec0"])


def _own(p, out):
    return own_step_errors(p, out["ray_vec"], out["npoints"], out["stop_code"], out["residual"])


def _copy(out):
    return {k: np.array(v, copy=True) for k, v in out.items()}


def _a_ray(out, min_points=6):
    """a ray that ends inside a step and has room for the plants"""
    ok = np.flatnonzero(~np.isin(out["stop_code"], OUTSIDE_THE_STEP) & (out["npoints"] >= min_points))
    assert len(ok), "the fixture has no ray that ends inside a step"
    return int(ok[len(ok) // 2])


def test_own_steps_of_the_emulated_trace_are_the_oracles(traced):
    p, out = traced
    o = _own(p, out)
    assert o["steps"] == int((out["npoints"] - 1).sum()) > 0
    assert o["midray_stops"] == 0 and o["terminal_disagree"] == 0
    assert o["terminal_judged"] == int((~np.isin(out["stop_code"], OUTSIDE_THE_STEP) & (out["npoints"] >= 2)).sum()) > 0
    if host_libm_is_the_variant_the_fixtures_were_cut_with():
        assert o["max_per_step"] == 0.0 and not o["err"].any()
        assert o["max_other_rows"] == 0.0 and o["max_damping_row"] == 0.0 and o["max_resid_diff"] == 0.0
    else:   # the oracle calls this host's libm, the kernel sources carry their own: the documented bars
        assert o["max_per_step"] <= 1e-10 and o["max_other_rows"] <= 1e-10 and o["max_damping_row"] <= 1e-6


def test_a_point_moved_by_1e9_is_found_on_the_two_steps_touching_it(traced):
    p, out = traced
    base = _own(p, out)["err"]
    bad = _copy(out)
    r = _a_ray(out)
    k = int(out["npoints"][r]) // 2
    bad["ray_vec"][r, k, 3:6] *= 1.0 + 1e-9
    o = _own(p, bad)
    hit = (o["ray"] == r) & ((o["point"] == k - 1) | (o["point"] == k))
    assert hit.sum() == 2
    assert (o["err"][hit] > 1e-10).all() and (o["err"][hit] < 1e-8).all(), o["err"][hit]
    np.testing.assert_array_equal(o["err"][~hit], base[~hit])      # every other step: untouched (0 on the fixtures' libm)
    assert int((o["err"] > 1e-10).sum()) == 2 + int((base > 1e-10).sum())
    assert o["midray_stops"] == 0 and o["terminal_disagree"] == 0
    # the landing step alone carries the relative move on k; r is not moved there
    land = hit & (o["point"] == k - 1)
    assert o["err"][land][0] == pytest.approx(1e-9, rel=1e-3)


def test_a_dropped_last_point_is_a_terminal_disagreement(traced):
    p, out = traced
    bad = _copy(out)
    r = _a_ray(out)
    bad["npoints"][r] -= 1
    o = _own(p, bad)
    assert o["terminal_disagree"] == 1 and o["terminal_disagreements"][0][0] == r
    assert o["terminal_disagreements"][0][4] is False          # the reference goes on from there: it does not stop
    assert o["midray_stops"] == 0 and o["steps"] == int((out["npoints"] - 1).sum()) - 1
    assert int((o["err"] > 1e-10).sum()) == 0


def test_a_doubled_last_point_is_a_midray_stop(traced):
    """the other direction: one point more than the reference records (the step that ends the ray, committed)"""
    p, out = traced
    bad = _copy(out)
    r = _a_ray(out)
    n = int(out["npoints"][r])
    assert n < bad["ray_vec"].shape[1]      # (a ray that ends inside a step ends before nstep_max)
    bad["ray_vec"][r, n] = bad["ray_vec"][r, n - 1]
    bad["npoints"][r] = n + 1
    o = _own(p, bad)
    assert o["midray_stops"] == 1 and o["midray_stop_steps"][0][:2] == (r, n - 1)
    assert o["midray_stop_steps"][0][2] == int(out["stop_code"][r])
    assert np.isinf(o["err"][(o["ray"] == r) & (o["point"] == n - 1)]).all()


def test_a_skipped_commit_is_found_at_its_step(traced):
    p, out = traced
    base = _own(p, out)["err"]
    bad = _copy(out)
    r = _a_ray(out)
    k = int(out["npoints"][r]) // 2
    bad["ray_vec"][r, k + 1] = out["ray_vec"][r, k + 2]         # point k + 1 holds the state two steps after point k
    bad["residual"][r, k + 1] = out["residual"][r, k + 2]
    o = _own(p, bad)
    at = (o["ray"] == r) & (o["point"] == k)
    assert at.sum() == 1 and o["err"][at][0] > 1e-6, o["err"][at]   # a whole step's displacement, not a rounding
    # the recorded step from the overwritten point (the state at k + 2) to the untouched point k + 2 is no step at all,
    # where the reference moves on by one: found as well; nothing else is
    after = (o["ray"] == r) & (o["point"] == k + 1)
    assert o["err"][after][0] > 1e-6
    np.testing.assert_array_equal(o["err"][~(at | after)], base[~(at | after)])
    assert o["terminal_disagree"] == 0


def test_rays_that_end_between_steps_or_never_start_are_not_judged():
    g, nml, p = load_golden("cfg1_slab16_rk4")
    out = emul_lib.trace(p, g["rvec0"], g["rindex_vec0"])
    o = _own(p, out)
    assert o["terminal_judged"] == int((~np.isin(out["stop_code"], OUTSIDE_THE_STEP) & (out["npoints"] >= 2)).sum())
    assert o["terminal_disagree"] == 0 and o["midray_stops"] == 0
    # an empty fan and a fan of rays without a step
    e = own_step_errors(p, out["ray_vec"][:0], out["npoints"][:0], out["stop_code"][:0])
    assert e["steps"] == 0 and e["terminal_judged"] == 0
    one = np.ones(2, dtype=np.int32)
    e = own_step_errors(p, out["ray_vec"][:2], one, np.array([40, 1], dtype=np.int32))
    assert e["steps"] == 0 and e["terminal_judged"] == 0 and e["err"].shape == (0,)
