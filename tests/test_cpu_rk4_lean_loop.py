"""CPU tier: the one-wave-per-SIMD RK4 trace kernel of the Solovev equilibrium holds its step loop twice (rays_rk4.hpp:
the lean step loop) -- a lean copy whose evaluations are compiled with the run's three model switches folded (density
model not 'constant', no parabolic temperature profile, ray_param not 'arcl') and the general copy -- and a launch takes
one of them (rays_trace.hpp: rk4_lean_loop).  The host emulation of the sources runs every case twice: under automatic
selection and with the developer switch RAYS_HIP_RK4_LOOP=general, under which every launch takes the general copy.
Both give the fixtures' arrays bit for bit; the wave emulator (64 lanes as fibers) counts the lanes that entered the lean
copy, and the product library's query (rays_hip_rk4_loop_for) states the same selection for the same parameter sets."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.namelist import read_namelist
from rays_amd.params import params_from_namelist
from rays_amd.ray_init import ray_init_XYZ_k_direction
from tests import emul_lib
from tests import group_emul_lib as ge
from tests import oracle_lib
from tests.common import ROOT, assert_matches_golden, load_golden, stop_codes

CHECK = "-DRAYS_EMUL_CHECK_UNIFORM_STAGE"
LOOPS = {"automatic": None, "forced_general": "general"}
ARRAYS = ("npoints", "stop_code", "ray_vec", "residual", "end_ray_vec", "end_residuals", "max_residuals")
# The Solovev RK4 fixtures with analytic derivatives (gold_solovev64_rk4_num: finite differences, no lean copy) and the
# loop automatic selection takes for each, read off its namelist: the electron temperature of three of them is
# 'parabolic', and two of those also have the 'constant' density model.
FIXTURES = {"gold_solovev64_pow_rk4": "general", "gold_solovev64_damp_rk4": "general",
            "gold_solovev_evanescent_rk4": "lean", "gold_solovev_file_rays_damp_rk4": "general",
            "cfg2_solovev1024_rk4": "lean"}


def _lib():
    # the library tests/test_cpu_rk4_step_loop.py builds (same tag, same switches: one compilation serves both files)
    library = ge.lib_variant("stagecheck", [CHECK])
    for fn in ("rays_emul_uniform_stage_violations", "rays_emul_lean_loop_lanes"):
        getattr(library, fn).restype = C.POINTER(C.c_int)
        getattr(library, fn).argtypes = []
    return library


def _lean_lanes(library):
    return int(library.rays_emul_lean_loop_lanes()[0])


def _select(monkeypatch, loop):
    if LOOPS[loop] is None:
        monkeypatch.delenv("RAYS_HIP_RK4_LOOP", raising=False)
    else:
        monkeypatch.setenv("RAYS_HIP_RK4_LOOP", LOOPS[loop])   # read by the emulated kernel at its start


def _trace(p, r0, n0):
    """One 64-lane wave of the emulator: (result, lanes that entered the lean copy during this trace)"""
    library = _lib()
    before = _lean_lanes(library)
    out = ge.trace_rk4_waves(p, r0, n0, nwaves=1, library=library)
    assert int(library.rays_emul_uniform_stage_violations()[0]) == 0
    return out, _lean_lanes(library) - before


def _statistics_from_the_recorded_residuals(g):
    """end_residuals and max_residuals as trace_rays leaves them (ray_tracing.f90:237-260), from the fixture's residual(:):
    the residual of the second-to-last point, and the largest |residual| before the last point."""
    npts, res = g["npoints"].astype(np.int64), g["residual"]
    end = np.array([res[r, n - 2] if n >= 2 else 0.0 for r, n in enumerate(npts)])
    mx = np.array([np.abs(res[r, :n - 1]).max() if n >= 2 else None for r, n in enumerate(npts)], dtype=object)
    return end, mx


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("name", list(FIXTURES))
def test_both_loops_give_the_fixtures_arrays(name, loop, monkeypatch):
    g, nml, p = load_golden(name)
    assert hip.rk4_loop(p) == FIXTURES[name]
    _select(monkeypatch, loop)
    if p.nv == 7:
        out, lean_lanes = _trace(p, g["rvec0"], g["rindex_vec0"])
        assert (lean_lanes > 0) == (loop == "automatic" and FIXTURES[name] == "lean"), f"{lean_lanes} lanes in the lean copy"
    else:   # the absorbed-power row: the wave emulator holds no nv = 8 kernel; one lane per wave, nothing counted
        assert FIXTURES[name] == "general"
        out = emul_lib.trace(p, g["rvec0"], g["rindex_vec0"])
    assert_matches_golden(out, g, p, exact=True)   # npoints, stop_code, ray_vec, residual, end_ray_vec: assert_array_equal
    end, mx = _statistics_from_the_recorded_residuals(g)
    np.testing.assert_array_equal(out["end_residuals"], end)
    took_a_step = g["npoints"] >= 2
    np.testing.assert_array_equal(out["max_residuals"][took_a_step], mx[took_a_step].astype(np.float64))


def _config_params(cfg):
    return params_from_namelist(read_namelist(os.path.join(ROOT, "configs", cfg)))


def test_the_baseline_solovev_fans_take_the_lean_loop():
    for cfg, nray in (("cfg2_solovev1024_rk4.in", 1024), ("cfg3b_solovev64k_rk4.in", 65536)):
        p = _config_params(cfg)
        assert hip.kernel_name(p, nray) == "rk4_trace_kernel<5, 2, 0, 7>"
        assert hip.rk4_loop(p, nray) == "lean", cfg


def test_the_developer_switch_forces_the_general_loop(monkeypatch):
    p = _config_params("cfg2_solovev1024_rk4.in")
    monkeypatch.setenv("RAYS_HIP_RK4_LOOP", "general")   # read by the library at every launch and every query
    assert hip.rk4_loop(p, 1024) == "general"
    monkeypatch.delenv("RAYS_HIP_RK4_LOOP")
    assert hip.rk4_loop(p, 1024) == "lean"


def test_kernels_without_a_lean_copy_answer_general():
    for name in ("gold_solovev64_rk4_num", "cfg1_slab16_rk4", "gold_axisym64_solmag_damp_rk4"):
        assert hip.rk4_loop(load_golden(name)[2]) == "general", name
    with pytest.raises(hip.RaysHipError):
        hip.rk4_loop(load_golden("gold_solovev64_sg_cold")[2])


# ---- one switch flipped in cfg 2's namelist: each variant takes the general loop ---------------------------------------
# All of them (and the unflipped twin below) move the box's outer wall inside the plasma (outer_bound = 1.4): with the
# parabolic density a ray ends at the plasma edge, where the mode runs into dD/dw -> 0, so it never reaches cfg 2's box.
BOX = dict(box_rmax=1.36)


def _flip(nml, variant):
    nml = copy.deepcopy(nml)
    nml["solovev_eq_list"].update(BOX)
    if variant == "ray_param_arcl":
        nml["rf_list"]["ray_param"] = "arcl"
        nml["ode_list"]["ds"] = 1.5e-2   # arc length in metres instead of time: about the fan's step in space
    elif variant == "parabolic_temperature":
        s = nml["solovev_eq_list"]
        s["t_prof_model"] = ["zero", "parabolic"]
        s["alphat1"], s["alphat2"] = [1.0, 1.0], [1.0, 1.0]
    elif variant == "constant_density":
        nml["solovev_eq_list"]["dens_prof_model"] = "constant"
    elif variant is not None:
        raise KeyError(variant)
    return nml


def _psi_n(p, rv):
    """psiN of solovev_psi (solovev_eq_m.f90:280-322) at trajectory points rv[..., 0:3]"""
    v = p.solovev
    r2 = rv[..., 0] ** 2 + rv[..., 1] ** 2
    psi = 0.5 * v.bphi0 * v.iota0 * (r2 * rv[..., 2] ** 2 / (v.rmaj * v.kappa) ** 2
                                     + (r2 - v.rmaj ** 2) ** 2 / v.rmaj ** 2 * 0.25)
    return psi / v.psiB


# launch points (minor radius, poloidal angle): six inside the plasma, two above and below it (psiN = 1.08, 1.13; inside
# the box), each with eight directions round the poloidal plane
LAUNCH_POINTS = [(0.30, 0.0), (0.36, 0.6), (0.38, 2.5), (0.33, -1.2), (0.34, 0.1), (0.25, 3.0), (0.55, math.pi / 2),
                 (0.57, -1.7)]


def _variant_rays(p, nml):
    """64 single rays, each launched by position and direction in the run's own mode (one_ray_init_XYZ_k_direction)"""
    r0, n0 = [], []
    for rmin, th in LAUNCH_POINTS:
        rvec = [p.solovev.rmaj + rmin * math.cos(th), 0.0, rmin * math.sin(th)]
        for i in range(8):
            a = 2.0 * math.pi * i / 8 + 0.2
            n, err = ray_init_XYZ_k_direction(p, nml["rf_list"], rvec, [math.cos(a), 0.3, math.sin(a)])
            assert not err and np.isfinite(n).all(), (rmin, th, i)
            r0.append(rvec)
            n0.append(n)
    assert len(r0) == 64
    return np.ascontiguousarray(r0, dtype=np.float64), np.ascontiguousarray(n0, dtype=np.float64)


BOX_EXITS = stop_codes(["R out_of_box", "z out_of_box"])


def _both_kinds_of_rays(p, ora):
    """The oracle alone: the 64 rays hold the two kinds the lean loop's removed joins could matter for -- rays with a
    recorded point at psiN >= 1 (no density there: the 0 * 0 / 0 of the density's logarithmic gradient) and rays that
    leave the box (a stage refuses and the lane parks).  Asserted, so that a change of the rays cannot silently empty it."""
    npts = ora["npoints"].astype(np.int64)
    recorded = np.arange(ora["ray_vec"].shape[1])[None, :] < npts[:, None]
    reach_vacuum = ((_psi_n(p, ora["ray_vec"]) >= 1.0) & recorded).any(axis=1)
    leave_box = np.isin(ora["stop_code"], BOX_EXITS)
    assert reach_vacuum.sum() >= 4, f"{reach_vacuum.sum()} rays reach psiN >= 1"
    assert leave_box.sum() >= 4, f"{leave_box.sum()} rays leave the box"
    assert len(set(npts.tolist())) > 8, "the rays of the wave end together"


@pytest.mark.parametrize("variant", ["ray_param_arcl", "parabolic_temperature", "constant_density"])
def test_one_flipped_switch_takes_the_general_loop_and_equals_the_oracle(variant, monkeypatch):
    g, nml0, p0 = load_golden("cfg2_solovev1024_rk4")
    nml = _flip(nml0, variant)
    p = params_from_namelist(nml)
    assert hip.rk4_loop(p0, 64) == "lean" and hip.rk4_loop(p, 64) == "general"
    assert hip.kernel_name(p, 64) == hip.kernel_name(p0, 64)   # the same kernel: only the loop inside it differs
    r0, n0 = _variant_rays(p, nml)
    ora = oracle_lib.trace(p, r0, n0)
    _both_kinds_of_rays(p, ora)
    monkeypatch.delenv("RAYS_HIP_RK4_LOOP", raising=False)
    out, lean_lanes = _trace(p, r0, n0)
    assert lean_lanes == 0
    for k in ARRAYS:
        np.testing.assert_array_equal(out[k], ora[k], err_msg=k)


def test_the_lean_loop_equals_the_oracle_on_rays_that_reach_the_vacuum_and_leave_the_box(monkeypatch):
    """The unflipped twin of the three variants on the same launches: the lean copy, and the forced general copy, against
    the oracle."""
    g, nml0, p0 = load_golden("cfg2_solovev1024_rk4")
    nml = _flip(nml0, None)
    p = params_from_namelist(nml)
    assert hip.rk4_loop(p, 64) == "lean"
    r0, n0 = _variant_rays(p, nml)
    ora = oracle_lib.trace(p, r0, n0)
    _both_kinds_of_rays(p, ora)
    for loop in LOOPS:
        _select(monkeypatch, loop)
        out, lean_lanes = _trace(p, r0, n0)
        assert (lean_lanes > 0) == (loop == "automatic")
        for k in ARRAYS:
            np.testing.assert_array_equal(out[k], ora[k], err_msg=f"{loop}: {k}")
