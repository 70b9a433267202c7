"""GPU tier: the two step loops of the one-wave-per-SIMD Solovev RK4 kernels (rays_rk4.hpp: the lean step loop).  The
library reads RAYS_HIP_RK4_LOOP at every launch, so one process runs a fan under automatic selection (the lean loop for
these configurations) and with the general loop forced; rays_hip_rk4_loop_for states which one a launch takes -- the
kernel's name is the same.  Exact flavour: both equal the fixtures bit for bit.  Tolerance flavour: both keep the exact
flavour's ray counts and stop codes, and every step they record is within 1e-10 of the reference's step from the same
point."""
import os

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import numerics_survey
from tests.common import load_golden, stop_codes
from tests.test_gpu_baseline_kernels import _fan

pytestmark = pytest.mark.gpu

PER_STEP_TOL = 1e-10   # north_star
LOOPS = {"automatic": None, "forced_general": "general"}


def _select(monkeypatch, loop, p, nray, automatic="lean"):
    """`automatic`: the loop the parameter set takes when nothing is forced"""
    if LOOPS[loop] is None:
        monkeypatch.delenv("RAYS_HIP_RK4_LOOP", raising=False)
    else:
        monkeypatch.setenv("RAYS_HIP_RK4_LOOP", LOOPS[loop])
    assert hip.rk4_loop(p, nray) == (automatic if loop == "automatic" else "general")


@pytest.fixture(scope="module")
def cfg2():
    return load_golden("cfg2_solovev1024_rk4")


@pytest.mark.parametrize("loop", list(LOOPS))
def test_cfg2_exact_equals_the_fixture(cfg2, loop, monkeypatch):
    g, nml, p = cfg2
    assert hip.get_numerics() == "exact" and hip.kernel_name(p, 1024) == "rk4_trace_kernel<5, 2, 0, 7>"
    _select(monkeypatch, loop, p, 1024)
    out = hip.trace_host(p, g["rvec0_full"], g["rindex_vec0_full"], ngpu=1)
    np.testing.assert_array_equal(out["npoints"], g["npoints_full"])
    np.testing.assert_array_equal(out["stop_code"], stop_codes(g["stop_flag_full"]))
    idx, keep = g["ray_index"], g["ray_vec"].shape[1]
    np.testing.assert_array_equal(out["ray_vec"][idx, :keep], g["ray_vec"])
    np.testing.assert_array_equal(out["residual"][idx, :keep], g["residual"])
    np.testing.assert_array_equal(out["end_ray_vec"][idx], g["end_ray_vec"])
    assert not out["ray_vec"][idx, keep:].any()


def _fixture_equals(g, p, out):
    np.testing.assert_array_equal(out["npoints"], g["npoints_full"])
    np.testing.assert_array_equal(out["stop_code"], stop_codes(g["stop_flag_full"]))
    idx, keep = g["ray_index"], g["ray_vec"].shape[1]
    np.testing.assert_array_equal(out["ray_vec"][idx, :keep], g["ray_vec"])
    np.testing.assert_array_equal(out["residual"][idx, :keep], g["residual"])
    np.testing.assert_array_equal(out["end_ray_vec"][idx], g["end_ray_vec"])


@pytest.mark.parametrize("loop", list(LOOPS))
def test_evanescent_fixture_exact_equals_the_fixture(loop, monkeypatch):
    """one ragged wave (31 rays), rays that stop at their launch point next to rays that run to nstep_max"""
    g, nml, p = load_golden("gold_solovev_evanescent_rk4")
    _select(monkeypatch, loop, p, len(g["rvec0_full"]))
    _fixture_equals(g, p, hip.trace_host(p, g["rvec0_full"], g["rindex_vec0_full"], ngpu=1))


@pytest.mark.parametrize("loop", list(LOOPS))
def test_damped_64_ray_fixture_exact_equals_the_fixture(loop, monkeypatch):
    """nv = 8, the absorbed-power row and the Z-function table in LDS next to the point window: a kernel that holds both
    copies; the fixture's own models ('constant' density, parabolic electron temperature) take the general one."""
    g, nml, p = load_golden("gold_solovev64_damp_rk4")
    assert len(g["rvec0_full"]) == 64 and hip.kernel_name(p, 64) == "rk4_trace_kernel<5, 2, 0, 8>"
    _select(monkeypatch, loop, p, 64, automatic="general")
    _fixture_equals(g, p, hip.trace_host(p, g["rvec0_full"], g["rindex_vec0_full"], ngpu=1))


@pytest.mark.parametrize("loop", list(LOOPS))
def test_cfg2_tolerance_keeps_the_counts_and_every_own_step(cfg2, loop, monkeypatch):
    g, nml, p = cfg2
    prev = hip.set_numerics("tolerance")
    try:
        assert hip.kernel_name(p, 1024) == "rk4_trace_kernel<21, 2, 0, 7>"
        _select(monkeypatch, loop, p, 1024)
        out = hip.trace_host(p, g["rvec0_full"], g["rindex_vec0_full"], ngpu=1)
    finally:
        hip.set_numerics(prev)
    # the exact flavour's counts are the fixture's (test_cfg2_exact_equals_the_fixture)
    np.testing.assert_array_equal(out["npoints"], g["npoints_full"])
    np.testing.assert_array_equal(out["stop_code"], stop_codes(g["stop_flag_full"]))
    nmax = int(out["npoints"].max())
    own = numerics_survey.own_step_errors(p, out["ray_vec"][:, :nmax], out["npoints"], out["stop_code"],
                                          residual=out["residual"][:, :nmax], nthreads=min(16, os.cpu_count() or 1))
    print(f"{loop}: {own['steps']} own steps, max per-step error {own['max_per_step']:.3e}, "
          f"mid-ray stops {own['midray_stops']}, rows >= 6 {own['max_other_rows']:.3e}")
    assert own["steps"] == int((out["npoints"].astype(np.int64) - 1).clip(0).sum()) > 100000
    assert own["midray_stops"] == 0
    assert own["max_per_step"] <= PER_STEP_TOL
    assert own["max_other_rows"] <= PER_STEP_TOL
    assert own["terminal_disagree"] == 0


@pytest.mark.parametrize("loop", list(LOOPS))
def test_the_step_entry_takes_the_same_loop_as_the_trace(loop, monkeypatch):
    """cfg 2 widened to 2048 rays (n_rindex_theta = 64): rays_hip_ode_step_device launches the trace kernel itself with
    nstep_max = 1, so it is the same kernel and the same loop, and from a trace's first points it lands on its second."""
    p, r0, n0 = _fan("cfg2_solovev1024_rk4.in", {"solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=64),
                                                 "ray_init_list": dict(nray_max=4096)})
    assert len(r0) == 2048
    q = copy_params(p)   # what the step entry launches with
    q.nstep_max = 1
    q.s_max = 1.7976931348623157e308
    _select(monkeypatch, loop, p, 2048)
    assert hip.kernel_name(q, 2048) == hip.kernel_name(p, 2048) == "rk4_trace_kernel<5, 2, 0, 7>"
    assert hip.rk4_loop(q, 2048) == hip.rk4_loop(p, 2048)
    short = copy_params(p)
    short.nstep_max = 4
    out = hip.trace_host(short, r0, n0, ngpu=1)
    v1, resid, code = hip.ode_step(p, out["ray_vec"][:, 0], np.zeros(len(r0)))
    took = out["npoints"] >= 2
    assert took.sum() > 1500
    assert (code[took] == 0).all()
    np.testing.assert_array_equal(v1[took], out["ray_vec"][took, 1])
    np.testing.assert_array_equal(resid[took], out["residual"][took, 1])
