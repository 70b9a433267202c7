"""CPU tier: fused trace and deposition (rays_hip_trace_deposition*, kernels with kEqNoTraj | kEqDeposit in EQ) -- the
product kernel sources in the variant that records no trajectory point and bins every accepted point, on the host
emulation with TraceArgs::residual NULL and ::ray_vec carrying the binning arguments (a trajectory store the variant
should not have crashes here, on the host); the Python plumbing and its refusals.  Every comparison is on bit
patterns; no tolerance appears anywhere."""
import dataclasses
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from rays_amd.params import STOP_CODE, copy_params
from tests import emul_lib
from tests import fused_deposition_lib as fl
from tests import summary_lib as sl
from tests.common import ROOT, load_golden
from tests.test_cpu_summary_trace import _fake_torch

EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")


def _rho(g):
    grid, fspl = fl.rho_table(g)
    return None if grid is None else (grid, fspl)


def _two_step_emul(p, r0, n0, power, which, n_bins, rho):
    """Emulated trace (the recording kernel) + emulated deposition (deposit_ray and the ray-ordered sum): the two-step
    path on the host."""
    full = emul_lib.trace(p, r0, n0)
    grid, fspl = rho if rho is not None else (np.zeros(2), np.zeros(8))
    work, prof = emul_lib.deposition(p, fl.WHICH[which], n_bins, full["ray_vec"], full["npoints"], power, grid, fspl)
    out = sl.summaries_of(full)
    out["work"], out["profile"] = work, prof
    return out


def _assert_same(out, ref, what=""):
    sl.assert_same(out, ref, what)
    np.testing.assert_array_equal(out["work"], ref["work"], err_msg=what + ": work")
    np.testing.assert_array_equal(out["profile"], ref["profile"], err_msg=what + ": profile")


# ---- 1. the fixtures on one emulated lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fl.DEP_FIXTURES)
def test_fused_kernel_source_on_host_equals_reference(name):
    """The twelve fixtures that carry the reference post-processor's results: work, profile and Q_sum equal dep_work,
    dep_profile and dep_q_sum for every profile the fixture holds, and the summaries equal the golden ones."""
    g, nml, p = load_golden(name)
    lib = fl.emul_lib()
    sl.set_axisym_tables(g, lib)
    for i, which in enumerate(fl.profile_names(g)):
        out = fl.emul_fused(p, g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], which, int(g["dep_n_bins"]),
                            rho=_rho(g), lib=lib)
        fl.assert_golden_deposition(out["work"], out["profile"], g, i, f"{name} {which}")
        fl.assert_golden_summaries(out, g, f"{name} {which}")


def test_profile_continues_the_carried_sums():
    """profile_in: the second block of rays continues the first block's running sums, and ends at the fixture's."""
    g, nml, p = load_golden("gold_slab16_damp_rk4")
    r0, n0, pw, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], int(g["dep_n_bins"])
    first = fl.emul_fused(p, r0[:7], n0[:7], pw[:7], "Ptotal_x", nb)
    second = fl.emul_fused(p, r0[7:], n0[7:], pw[7:], "Ptotal_x", nb, profile_in=first["profile"])
    np.testing.assert_array_equal(second["profile"], g["dep_profile"][0])
    np.testing.assert_array_equal(np.concatenate([first["work"], second["work"]]), g["dep_work"][0])


# ---- 2. bin re-entry -----------------------------------------------------------------------------------------------------
def test_rays_that_re_enter_a_bin_they_have_left():
    """gold_axisym64_solmag_damp_rk4: psiN along some rays is not monotonic and comes back into a bin it has left, so a
    bin receives additions that are not consecutive.  The count of such rays is asserted before the case is relied on;
    their rows equal the reference post-processor's."""
    g, nml, p = load_golden("gold_axisym64_solmag_damp_rk4")
    nb = int(g["dep_n_bins"])
    rv, npts = g["dep_ray_vec_full"], g["npoints_full"]
    from tests import diag_expect
    # psiN of 'solovev_magnetics' at the recorded points (the host restatement), for the sequence of bins only
    psin = [[diag_expect.psi_expected(p, None, rv[i, k]) for k in range(n)] for i, n in enumerate(npts)]
    re_enter = []
    for i, n in enumerate(npts):
        bins = np.floor(np.array(psin[i]) * nb).astype(int)
        runs = bins[np.concatenate([[True], bins[1:] != bins[:-1]])]
        if len(set(runs.tolist())) < len(runs):
            re_enter.append(i)
    assert len(re_enter) > 0, "no ray of this fixture re-enters a bin: the case checks nothing"
    lib = fl.emul_lib()
    sl.set_axisym_tables(g, lib)
    out = fl.emul_fused(p, g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], "Ptotal_psi", nb, lib=lib)
    np.testing.assert_array_equal(out["work"][re_enter], g["dep_work"][0][re_enter])
    assert out["work"][re_enter].any()


# ---- 3. whole emulated waves with refills ------------------------------------------------------------------------------------
VARIANTS = {"default": [], "cost0": ["-DRAYS_REFILL_EVENT_COST=0"]}


def _wave_case(name, nray, nstep_max):
    g, nml, p = load_golden(name)
    q = copy_params(p)
    q.nstep_max = min(q.nstep_max, nstep_max)
    reps = -(-nray // len(g["rvec0_full"]))
    r0 = np.tile(g["rvec0_full"], (reps, 1))[:nray].copy()
    n0 = np.tile(g["rindex_vec0_full"], (reps, 1))[:nray].copy()
    n0[9] *= 3.0   # far off the dispersion surface: refused at its initial check, one point and no segment
    # a power of its own for every ray: tiled rays are otherwise identical and a row / ray mix-up would pass
    power = (1.0 + 0.01 * np.arange(nray)) / nray
    return g, q, r0, n0, power


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rk4_waves_with_refills(variant):
    """170 damped eqdsk rays on ONE emulated wave (every lane is refilled once or twice), for two settings of
    RAYS_REFILL_EVENT_COST, in index order and long-first: a refilled lane starts its ray's x_prev / q_prev afresh and
    writes the row of the ray it holds.  Against the emulated trace + the emulated deposition."""
    g, q, r0, n0, power = _wave_case("gold_axisym64_eqdsk_damp_rk4", 170, 80)
    lib = fl.emul_lib(wave=True, tag="" if variant == "default" else variant, defs=VARIANTS[variant])
    sl.set_axisym_tables(g, lib)
    nb = 100
    ref = _two_step_emul(q, r0, n0, power, "Ptotal_psi", nb, None)
    assert ref["npoints"][9] == 1 and not ref["work"][9].any()
    # rays that end in total_absorption: their last step is refused by check_save, so it is neither recorded nor binned
    assert (ref["stop_code"] == [v for k, v in STOP_CODE.items() if k.strip() == "total_absorption"][0]).any()
    assert len({tuple(w) for w in ref["work"]}) > 150
    for stride in (0, 2):
        out = fl.emul_fused_waves(q, r0, n0, power, "Ptotal_psi", nb, "rk4", 1, stride, lib=lib)
        _assert_same(out, ref, f"stride {stride}")
    rho = _rho(g)
    _assert_same(fl.emul_fused_waves(q, r0, n0, power, "Ptotal_rho", nb, "rk4", 1, 2, rho=rho, lib=lib),
                 _two_step_emul(q, r0, n0, power, "Ptotal_rho", nb, rho), "Ptotal_rho")


def test_sg_waves_with_refills():
    """The same for sg_trace_kernel on the SG wave emulator: 150 rays on one wave, nstep_max = 12."""
    g, q, r0, n0, power = _wave_case("gold_axisym64_eqdsk_damp_sg", 150, 12)
    lib = fl.emul_lib(wave=True)
    sl.set_axisym_tables(g, lib)
    ref = _two_step_emul(q, r0, n0, power, "Ptotal_psi", 64, None)
    assert ref["npoints"][9] == 1 and ref["npoints"].max() == 13
    _assert_same(fl.emul_fused_waves(q, r0, n0, power, "Ptotal_psi", 64, "sg", 1, lib=lib), ref)


# ---- 4. the host entry on the emulated four-device runtime, stand-alone ----------------------------------------------------
def _case_file(path):
    """101 rays of the axisym_toroid + solovev_magnetics fixture (no eqdsk table needed), powers all different, one ray
    refused at its initial check; the expected bytes from the one-lane emulation of the fused kernel."""
    g, nml, p = load_golden("gold_axisym64_solmag_damp_rk4")
    q = copy_params(p)
    q.nstep_max = 60
    nray, nb = 101, 50
    r0 = np.tile(g["rvec0_full"], (2, 1))[:nray].copy()
    n0 = np.tile(g["rindex_vec0_full"], (2, 1))[:nray].copy()
    n0[40] *= 3.0
    power = (1.0 + 0.01 * np.arange(nray)) / nray
    ref = fl.emul_fused(q, r0, n0, power, "Ptotal_psi", nb)
    assert ref["npoints"][40] == 1 and ref["npoints"].max() == 61 and len(np.unique(ref["npoints"])) > 3
    assert ref["work"].any() and not ref["work"][40].any()
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    with open(path, "wb") as f:
        f.write(struct.pack("=6i", nray, q.nv, nb, fl.WHICH["Ptotal_psi"], len(z["fspl_re"]), len(bytes(q))))
        f.write(bytes(q))
        f.write(np.array([float(z["x_min"]), float(z["x_max"])]).tobytes())
        for a in (z["fspl_re"], r0, n0, power):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for k in sl.KEYS + ("work",):
            f.write(np.ascontiguousarray(ref[k], dtype=np.int32 if k in ("npoints", "stop_code") else np.float64).tobytes())


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_entry_on_emulated_devices(sanitize, tmp_path):
    """rays_hip_trace_deposition with 1 to 4 devices, a ragged last block and empty blocks: summaries and work equal the
    one-lane emulation's, the profile chained over the blocks equals the single block's ray-ordered sum; the named
    refusals; after rays_hip_finalize the emulated driver reports no live allocation, pinned block, stream or event.
    Once plain and once as an ASan + UBSan executable with its own main (leak detection on)."""
    subprocess.check_call(["make", "-s", "-j", str(min(4, os.cpu_count() or 1)), "-f", "Makefile.capi", "fused"] +
                          (["SAN=1"] if sanitize else []), cwd=EMUL_DIR)
    exe = os.path.join(EMUL_DIR, "build_capi_san/emul_fused_capi_san" if sanitize else "build_capi/emul_fused_capi")
    case = str(tmp_path / "fused_case.bin")
    _case_file(case)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS", "LD_PRELOAD")}
    env.update(RAYS_EMUL_DEVICES="4")
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, case], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fused capi ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 5. Python plumbing and the refusals ------------------------------------------------------------------------------------
def test_ray_deposition_record():
    from rays_amd import results
    from rays_amd.trace import RayDeposition, RaySummaries, deposition_grid_limits
    g, nml, p = load_golden("gold_slab16_damp_rk4")
    s = RaySummaries(np.array([3], dtype=np.int32), np.array([1], dtype=np.int32), np.zeros((1, 8)), np.zeros((1, 8)),
                     np.zeros(1), np.zeros(1))
    prof = g["dep_profile"][0]
    lo, hi = deposition_grid_limits(p, "Ptotal_x")
    assert (lo, hi) == (float(p.slab.xmin), float(p.slab.xmax)) and deposition_grid_limits(p, "Ptotal_rho") == (0.0, 1.0)
    d = RayDeposition(s, "Ptotal_x", len(prof), lo, hi, prof, None)
    assert [f.name for f in dataclasses.fields(RayDeposition)][:2] == ["summaries", "profile_name"]
    rec = d.profile_record
    assert d.Q_sum == float(g["dep_q_sum"][0]) == rec["Q_sum"] and rec["grid_name"] == "x"
    np.testing.assert_array_equal(rec["grid"], results.deposition_grid(lo, hi, len(prof)))


def test_python_layer_refuses_by_name(monkeypatch):
    """DeviceTrace / RaysRun: deposition=... with trajectories, an unknown profile, a malformed tuple, powers of the wrong
    length, profile_in without deposition; no tensor with an nstep_max + 1 axis is allocated for a fused trace."""
    from rays_amd import hip, trace
    g, nml, p = load_golden("gold_slab16_damp_rk4")
    allocated = []
    monkeypatch.setitem(sys.modules, "torch", _fake_torch(allocated))
    sys.modules["torch"].is_tensor = lambda x: False
    monkeypatch.setattr(hip, "check_params", lambda q: None)
    r0, n0 = g["rvec0"], g["rindex_vec0"]
    n, nb, npt = len(r0), 100, p.nstep_max + 1
    pw = np.ones(n)
    dt = trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_x", nb, pw))
    assert dt.ray_vec is None and dt.residual is None and dt.deposition == ("Ptotal_x", nb)
    assert dt.work.shape == (nb, n) and dt.profile.shape == (nb,) and dt.start_ray_vec.shape == (n, p.nv)
    assert allocated and all(npt not in s for s in allocated), allocated
    with pytest.raises(ValueError, match="trajectories=False"):
        trace.DeviceTrace(p, r0, n0, deposition=("Ptotal_x", nb, pw))
    with pytest.raises(ValueError, match="known are"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_y", nb, pw))
    with pytest.raises(ValueError, match=r"deposition=\(which, n_bins, power\)"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_x", nb))
    with pytest.raises(ValueError, match="one weight per ray"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_x", nb, pw[:-1]))
    with pytest.raises(ValueError, match="profile_in without"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, profile_in=object())
    with pytest.raises(ValueError, match="power weights"):
        trace.RaysRun(p, r0, n0).trace_rays(trajectories=False, deposition=("Ptotal_x", nb))
    run = trace.RaysRun(p, r0, n0, ray_pwr_wt=pw)
    with pytest.raises(ValueError, match="trajectories=False"):
        run.trace_rays(deposition=("Ptotal_x", nb))
    with pytest.raises(ValueError, match=r"deposition=\(which, n_bins\)"):
        run.trace_rays(trajectories=False, deposition=("Ptotal_x", nb, pw))
    with pytest.raises(ValueError, match="known are"):
        hip.trace_deposition_device(p, n, 1, 1, 1, "Ptotal", nb, 1, 1, 0, 1, 1, 1, 1, None, 1)


def test_binding_declares_the_entries():
    from rays_amd import hip
    for sym in ("rays_hip_trace_deposition_device", "rays_hip_trace_deposition", "rays_hip_deposition_kernel_name_for"):
        assert sym in hip.EXPORTED_SYMBOLS
    try:
        lib = hip.load()
    except hip.RaysHipError:
        pytest.skip("librays_hip.so is not built here")
    g, nml, p = load_golden("gold_slab16_damp_rk4")
    assert len(lib.rays_hip_trace_deposition_device.argtypes) == 17 and len(lib.rays_hip_trace_deposition.argtypes) == 16
    assert hip.deposition_kernel_name(p, 16) == "rk4_trace_kernel<100, 2, 0, 8>"
    assert hip.summary_kernel_name(p, 16) == "rk4_trace_kernel<36, 2, 0, 8>"
