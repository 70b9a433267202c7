"""GPU tier: what the numerics of the kernels bench.py runs ARE on the BASELINE fans at full size, measured against the
oracle (tests/numerics_survey.py) -- not on 30 rays of a fixture:

  * cfg 3b, the headline fan: all 65 536 rays, every one of its 12.87 M recorded steps restarted from the oracle's point;
  * cfg 5b (eqdsk + damping): all 262 144 rays;
  * cfg 4 (slab, 1 M rays, two-waves build): every 16th ray;
  * the headline fan refined four times in launch angle (262 144 rays, what `bench.py --fan-scale 4` runs): all rays --
    a Solovev fan of two waves per SIMD worth of rays and more, for which the dispatcher must pick a kernel that meets
    the bar (the two-waves build has no hand-over of the ill-conditioned last steps).

Each fan is judged twice per step: `restart` (the step kernel restarted from the oracle's points) and `own` (the
oracle's one step from the TRACED fan's own point k against its point k + 1: what the benchmarked persistent loop did,
tests/numerics_survey.own_step_errors).

For the tolerance flavour the test records and bounds: steps above 1e-10 / 1e-11 (north_star's per-step bar), the
largest per-step error, the largest POINTWISE deviation of the traced fan from the oracle and the share of points
above 1e-10; ray counts and stop codes of every surveyed ray must be the oracle's.  For the exact flavour (headline fan and cfg 5b) everything
must be zero.  The numbers go to gpurun_out/numerics_evidence.json (copied to profiles/numerics_evidence.json, which
bench.py quotes in its line as `numerics_evidence`, labelled as replayed and keyed by the kernel sources' hash)."""
import json
import os

import pytest

import bench
from rays_amd import hip
from tests import oracle_lib
from tests.common import ROOT
from tests.numerics_survey import survey

pytestmark = pytest.mark.gpu

# config, ray stride, states per restart call (below / from 131072: the one-wave / two-waves build, as the fan dispatches)
FANS = [("cfg3b_solovev64k_rk4.in", 1, 65536), ("cfg5b_axisym256k_rk4_damp.in", 1, 65536), ("cfg4_slab1M_rk4.in", 16, 262144)]

# Bounds of the tolerance flavour, per config: steps above 1e-10 (north_star's bar: none), max per step, max pointwise.
# Measured (profiles/numerics_evidence.json): per step 5.1e-15 | 2.2e-16 | 3.5e-14, pointwise 1.1e-8 | 4.2e-15 | 2.3e-9.
# On the traced fans' own steps (own_max_per_step): 4.4e-15 | 2.2e-16 | 2.4e-13; held to the same per-step bounds.
# Before the ill-conditioned steps were handed over to the reference's arithmetic (rays_rk4_body.inc: kStopResumeExact)
# the headline fan had 13 steps above 1e-10, max 4.5e-10.  The per-step bounds leave two decades for another compiler's
# instruction selection; the pointwise ones are regression alarms (accumulated deviation is not part of the per-step bar).
BOUNDS = {
    "cfg3b_solovev64k_rk4.in": dict(n_above=0, max_per_step=1e-12, max_pointwise=5e-8),
    "cfg5b_axisym256k_rk4_damp.in": dict(n_above=0, max_per_step=1e-13, max_pointwise=1e-9),
    "cfg4_slab1M_rk4.in": dict(n_above=0, max_per_step=1e-11, max_pointwise=1e-6),
}


def _record(cfg, flavour, res):
    d = os.path.join(ROOT, "gpurun_out")
    if not os.path.isdir(d):
        return
    path = os.path.join(d, "numerics_evidence.json")
    db = json.load(open(path)) if os.path.exists(path) else {}
    res = dict(res, source_hash=bench.kernel_source_hash())
    db[f"{cfg}::{flavour}"] = res
    json.dump(db, open(path, "w"), indent=1, sort_keys=True)


def _fan(cfg, scale=1):
    nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", cfg), 1, scale, None)
    if bench.build_fan.tables is not None:
        oracle_lib.set_axisym_tables(bench.build_fan.tables)
    return p, r0, n0


def _survey_tolerance(cfg, stride, batch, scale=1):
    prev = hip.set_numerics("tolerance")
    try:
        p, r0, n0 = _fan(cfg, scale)
        eq = int(hip.kernel_name(p, len(r0)).split("<")[1].split(",")[0])
        assert eq & 16, hip.kernel_name(p, len(r0))
        assert hip.kernel_name(p, batch) == hip.kernel_name(p, len(r0)), "restarts must run the build the fan dispatches"
        res = survey(p, r0, n0, ray_stride=stride, restart_batch=batch, progress=print, own_step=True)
    finally:
        hip.set_numerics(prev)
    _record(cfg if scale == 1 else f"{cfg}*{scale}", "tolerance", res)
    print(json.dumps(res))
    return res


def _assert_the_contract(res):
    """The tolerance flavour's contract -- conditions, not measurements: counts and stop flags exactly the reference's,
    every step within 1e-10 (restarted from the reference's points AND on the traced fan's own points), no recorded
    point from which the reference would have ended the ray; rows >= 6 by the rule of
    test_gpu_tolerance_flavour.test_per_step_within_1e10_of_the_reference."""
    assert res["rays_with_other_counts"] == 0, "a ray count / stop code differs from the oracle's"
    assert res["restarts_stopped"] == 0
    assert res["n_above_1e-10"] == 0, res["worst_steps"]
    assert res["own_steps"] > 0 and res["own_ray_stride"] == 1
    assert res["own_n_above_1e-10"] == 0, res["own_worst_steps"]
    assert res["own_midray_stops"] == 0, res["own_midray_stop_steps"]
    assert res["own_max_other_rows"] <= 1e-10 and res["own_max_damping_row"] <= 1e-6
    # own_terminal_disagree is recorded, not asserted: from a last point 1e-8 off the reference's trajectory the
    # reference's arithmetic may end the ray a step earlier or later than it does on its own trajectory
    print(f"own steps: {res['own_steps']}, max {res['own_max_per_step']:.3e}, last points judged {res['own_terminal_judged']}, "
          f"where the reference would not end the ray alike: {res['own_terminal_disagree']} {res['own_terminal_disagreements']}")


@pytest.mark.parametrize("cfg,stride,batch", FANS)
def test_tolerance_flavour_on_the_full_fan(cfg, stride, batch):
    res = _survey_tolerance(cfg, stride, batch)
    b = BOUNDS[cfg]
    _assert_the_contract(res)
    assert res["n_above_1e-10"] <= b["n_above"], res["worst_steps"]
    assert res["max_per_step"] <= b["max_per_step"], res["worst_steps"]
    assert res["own_max_per_step"] <= b["max_per_step"], res["own_worst_steps"]
    assert res["max_pointwise"] <= b["max_pointwise"]


def test_tolerance_flavour_on_the_solovev_fan_of_262144_rays():
    """The headline fan refined four times in launch angle (`bench.py --fan-scale 4`): from 131072 rays on the
    dispatcher prefers a two-waves-per-SIMD build where one exists, and that build has no hand-over of the
    ill-conditioned last steps of Solovev rays.  Whatever kernel the tolerance setting dispatches for this fan must be
    a tolerance kernel and meet the bar on all 262144 rays; the restarts run in batches of the fan's size, i.e. on the
    same build.  Bounds: cfg 3b's own per-step bound (same equilibrium, same kernel family, the same fan refined in
    angle); pointwise the project's accumulated bar (test_gpu_tolerance_flavour.ACCUMULATED_TOL; cfg 3b's 5e-8 alarm
    was cut on other rays)."""
    cfg = "cfg3b_solovev64k_rk4.in"
    res = _survey_tolerance(cfg, 1, 262144, scale=4)
    print("kernel surveyed:", res["kernel"], "| restarts on:", res["restart_kernel"])
    assert res["rays_total"] == res["rays_surveyed"] == 262144
    _assert_the_contract(res)
    assert res["max_per_step"] <= BOUNDS[cfg]["max_per_step"], res["worst_steps"]
    assert res["own_max_per_step"] <= BOUNDS[cfg]["max_per_step"], res["own_worst_steps"]
    assert res["max_pointwise"] <= 1e-6


@pytest.mark.parametrize("cfg,stride,batch", FANS[:2])
def test_exact_flavour_on_the_full_fans(cfg, stride, batch):
    """The exact kernels on the same survey (headline fan; the eqdsk fan, whose spline cell search takes its estimate from
    host-computed grid constants): every restarted step and every traced point IS the oracle's -- and so the oracle's
    step from each traced point is the next traced point, and ends the ray where the kernel ended it."""
    prev = hip.set_numerics("exact")
    try:
        p, r0, n0 = _fan(cfg)
        res = survey(p, r0, n0, ray_stride=stride, restart_batch=batch, progress=print, own_step=True)
    finally:
        hip.set_numerics(prev)
    _record(cfg, "exact", res)
    assert res["rays_with_other_counts"] == 0 and res["restarts_stopped"] == 0
    assert res["max_per_step"] == 0.0 and res["max_pointwise"] == 0.0 and res["points_not_identical"] == 0
    assert res["own_steps"] == res["points_compared"] - res["rays_surveyed"] > 0
    assert res["own_max_per_step"] == 0.0 and res["own_n_above_1e-12"] == 0 and res["own_midray_stops"] == 0
    assert res["own_max_other_rows"] == 0.0 and res["own_max_damping_row"] == 0.0 and res["own_max_resid_diff"] == 0.0
    assert res["own_terminal_judged"] > 0 and res["own_terminal_disagree"] == 0, res["own_terminal_disagreements"]


def test_shampine_gordon_eqdsk_fan_is_the_oracles_at_full_size():
    """BASELINE config 5 (eqdsk splines + damping, SG, 262 144 rays) at full size: every recorded point of every ray, the
    counts and the stop codes are the oracle's, bit for bit (the kernel has one numerics flavour; the oracle's share of
    the test is ~20 s of the box's host cores)."""
    cfg = "cfg5_axisym256k_sg_damp.in"
    p, r0, n0 = _fan(cfg)
    assert hip.kernel_name(p, len(r0)).startswith("sg_trace_kernel<6, 2, 0, 8>")
    res = survey(p, r0, n0, per_step=False, progress=print)
    _record(cfg, "exact", res)
    assert res["rays_surveyed"] == len(r0) and res["rays_with_other_counts"] == 0
    assert res["points_compared"] > 7_000_000 and res["max_pointwise"] == 0.0 and res["points_not_identical"] == 0


def test_shampine_gordon_finite_difference_fan_is_the_oracles_at_full_size():
    """BASELINE config 3 (Solovev 64k fan, SG + finite-difference dD: `sg_group_kernel`, one ray per group of four lanes)
    launched at full size: every recorded point of every FOURTH ray (16 384 rays; with fourteen determinants per
    evaluation the oracle's share is ~30 s of the box's host cores: 64 s for every second ray, same result), the counts
    and the stop codes are the oracle's, bit for bit."""
    cfg = "cfg3_solovev64k_sg_num.in"
    p, r0, n0 = _fan(cfg)
    assert hip.kernel_name(p, len(r0)).startswith("sg_group_kernel<5, 2, 4>")
    res = survey(p, r0, n0, ray_stride=4, per_step=False, progress=print)
    _record(cfg, "exact", res)
    assert res["rays_surveyed"] == len(r0) // 4 and res["rays_with_other_counts"] == 0
    assert res["points_compared"] > 3_000_000 and res["max_pointwise"] == 0.0 and res["points_not_identical"] == 0
