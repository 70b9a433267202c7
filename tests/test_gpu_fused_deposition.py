"""GPU tier: fused trace and deposition -- rays_hip_trace_deposition_device / rays_hip_trace_deposition and the kernels
they launch (EQ + 96 in their names: the summary-only kernels that also bin every accepted point; no trajectory array
exists).  Everything is compared on bit patterns: with the reference post-processor's work / profile / Q_sum in the
golden files, and with rays_hip_trace_device followed by rays_hip_deposition_device on the same rays in the same
process.  No tolerance appears anywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import fused_deposition_lib as fl
from tests import summary_lib as sl
from tests.common import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _load(name):
    g, nml, p = load_golden(name)
    grid, fspl = fl.rho_table(g)
    if grid is not None:
        hip.set_rho_table(grid, fspl)
    return g, nml, p


def _fused(p, r0, n0, power, which, n_bins, profile_in=None):
    """rays_hip_trace_deposition_device through DeviceTrace(deposition=...): summaries, work[nray][n_bins], profile."""
    import torch
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0, trajectories=False, deposition=(which, n_bins, power), profile_in=profile_in)
    assert tr.ray_vec is None and tr.residual is None
    tr.work.fill_(float("nan"))   # the call zeroes work itself
    tr.launch()
    res = tr.results()
    out = {k: getattr(res, k) for k in sl.KEYS}
    out["work"] = np.ascontiguousarray(tr.work.cpu().numpy().T)
    out["profile"] = tr.profile.cpu().numpy()
    del tr
    torch.cuda.empty_cache()
    return out


def _two_step(p, r0, n0, power, which, n_bins):
    """rays_hip_trace_device, then rays_hip_deposition_device on its trajectories: the path the fused one replaces."""
    import torch
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0)
    tr.launch()
    nray = tr.nray
    d_pw = torch.as_tensor(np.ascontiguousarray(power, dtype=np.float64)).cuda()
    work = torch.zeros((n_bins, nray), dtype=torch.float64, device="cuda")
    prof = torch.zeros(n_bins, dtype=torch.float64, device="cuda")
    hip.deposition_device(p, which, n_bins, nray, tr.ray_vec.data_ptr(), tr.npoints.data_ptr(), d_pw.data_ptr(),
                          work.data_ptr(), None, prof.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: getattr(tr, k).cpu().numpy() for k in sl.KEYS if k != "start_ray_vec"}
    out["start_ray_vec"] = tr.ray_vec[:, 0, :].contiguous().cpu().numpy()
    out["work"] = np.ascontiguousarray(work.cpu().numpy().T)
    out["profile"] = prof.cpu().numpy()
    del tr, work
    torch.cuda.empty_cache()
    return out


def _assert_same(out, ref, what=""):
    sl.assert_same(out, ref, what)
    np.testing.assert_array_equal(out["work"], ref["work"], err_msg=what + ": work")
    np.testing.assert_array_equal(out["profile"], ref["profile"], err_msg=what + ": profile")


def _resident_lanes():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


def _tiled(r0, n0, nray):
    reps = nray // len(r0) + 1
    return np.tile(r0, (reps, 1))[:nray].copy(), np.tile(n0, (reps, 1))[:nray].copy()


def _distinct_powers(nray):
    """One weight per ray, all different: tiled rays are otherwise identical and a row / ray mix-up would pass."""
    return (1.0 + np.arange(nray, dtype=np.float64) * 0.001) / nray


# ---- 1. fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fl.DEP_FIXTURES)
def test_fixture_deposition_equals_golden(name):
    """The twelve fixtures with the reference post-processor's results (RK4 / SG, cold / finite-difference dD, eqdsk
    spline / bilinear / solovev_magnetics, splined profiles, slab Ptotal_x, multi-species damping with gradients): work,
    profile and Q_sum of every profile the fixture holds, and the summaries, bit for bit; the kernel is the summary-only
    one with the deposition bit (EQ + 64)."""
    g, nml, p = _load(name)
    r0, n0 = g["rvec0_full"], g["rindex_vec0_full"]
    head, rest = hip.summary_kernel_name(p, len(r0)).split("<", 1)
    eq, tail = rest.split(",", 1)
    assert hip.deposition_kernel_name(p, len(r0)) == f"{head}<{int(eq) + 64},{tail}"
    for i, which in enumerate(fl.profile_names(g)):
        out = _fused(p, r0, n0, g["dep_power"], which, int(g["dep_n_bins"]))
        fl.assert_golden_deposition(out["work"], out["profile"], g, i, f"{name} {which}")
        fl.assert_golden_summaries(out, g, f"{name} {which}")


# ---- 2. bin counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 7, 100, 320])
@pytest.mark.parametrize("name", ["gold_axisym64_eqdsk_damp_rk4", "gold_slab16_damp_rk4"])
def test_bin_counts_equal_the_two_step_path(name, n_bins):
    g, nml, p = _load(name)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    for which in fl.profile_names(g):
        out = _fused(p, r0, n0, power, which, n_bins)
        assert out["profile"].sum() > 0.0
        _assert_same(out, _two_step(p, r0, n0, power, which, n_bins), f"{name} {which} {n_bins} bins")


# ---- 3. refill -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["rk4", "sg"])
def test_refilled_lanes_start_their_ray_afresh(solver):
    """The 64 rays of the eqdsk + damping fixture tiled to resident lanes + 4500 rays (RK4: nstep_max = 40, handed out
    long-first; SG: nstep_max = 10), every ray with a power of its own, one ray outside the box and one refused at its
    initial check: work, profile and summaries equal the two-step path's."""
    g, nml, p0 = _load("gold_axisym64_eqdsk_damp_rk4" if solver == "rk4" else "gold_axisym64_eqdsk_damp_sg")
    p = copy_params(p0)
    p.nstep_max = 40 if solver == "rk4" else 10
    nray = _resident_lanes() + 4500
    r0, n0 = _tiled(g["rvec0_full"], g["rindex_vec0_full"], nray)
    r0[7, 0] = 10.0      # outside the box
    n0[11] *= 3.0        # stops at the initial check_save
    power = _distinct_powers(nray)
    want = ("rk4_trace_kernel" if solver == "rk4" else "sg_trace_kernel") + "<102, 2, 0, 8>"
    assert hip.deposition_kernel_name(p, nray) == want
    assert nray > _resident_lanes()
    nb = 100
    ref = _two_step(p, r0, n0, power, "Ptotal_psi", nb)
    # RK4: both hand-out orders, each asked for by name (the library reads the switch at every launch), so that the
    # long-first order is covered whatever the library's default is; the SG kernel hands out in index order
    orders = ("pilot2", "index") if solver == "rk4" else (None,)
    saved = os.environ.get("RAYS_HIP_RAY_ORDER")
    try:
        for order in orders:
            if order is not None:
                os.environ["RAYS_HIP_RAY_ORDER"] = order
            out = _fused(p, r0, n0, power, "Ptotal_psi", nb)
            assert out["npoints"][7] == 1 and out["npoints"][11] == 1 and out["npoints"].max() == p.nstep_max + 1
            assert not out["work"][7].any() and not out["work"][11].any()   # one point, no segment
            _assert_same(out, ref, f"{solver}, ray order {order}")
    finally:
        if saved is None:
            os.environ.pop("RAYS_HIP_RAY_ORDER", None)
        else:
            os.environ["RAYS_HIP_RAY_ORDER"] = saved


# ---- 4. chaining ------------------------------------------------------------------------------------------------------------
def test_two_blocks_chained_through_profile_in_equal_one_call():
    import torch
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], int(g["dep_n_bins"])
    h = 29
    for i, which in enumerate(fl.profile_names(g)):
        first = _fused(p, r0[:h], n0[:h], power[:h], which, nb)
        carry = torch.as_tensor(first["profile"]).cuda()
        second = _fused(p, r0[h:], n0[h:], power[h:], which, nb, profile_in=carry)
        np.testing.assert_array_equal(second["profile"], g["dep_profile"][i])
        np.testing.assert_array_equal(np.concatenate([first["work"], second["work"]]), g["dep_work"][i])
        assert not np.array_equal(first["profile"], second["profile"])


# ---- 5. the host form ---------------------------------------------------------------------------------------------------------
def test_host_entry_equals_trace_plus_deposition():
    """rays_hip_trace_deposition equals rays_hip_trace + rays_hip_deposition, with one slot and with three slots on one
    device (blocks of 22, 22, 20 rays chained in ray order); RaysRun returns the profile record the writer takes; a kept
    result image does not survive the call."""
    from rays_amd.trace import RayDeposition, RaysRun
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], int(g["dep_n_bins"])
    full = hip.trace_host(p, r0, n0, ngpu=1)
    ref = sl.summaries_of(full)
    for i, which in enumerate(fl.profile_names(g)):
        ref["work"], ref["profile"] = hip.deposition_host(p, which, nb, full["ray_vec"], full["npoints"], power)
        _assert_same(hip.trace_deposition_host(p, r0, n0, power, which, nb, ngpu=1), ref, which)
        hip.init_devices([0, 0, 0])
        try:
            out = hip.trace_deposition_host(p, r0, n0, power, which, nb, ngpu=None)
            _assert_same(out, ref, which + ", three slots")
            nowork = hip.trace_deposition_host(p, r0, n0, power, which, nb, ngpu=None, want_work=False)
            assert nowork["work"] is None
            np.testing.assert_array_equal(nowork["profile"], ref["profile"])
        finally:
            hip.load().rays_hip_init(1)
        fl.assert_golden_deposition(out["work"], out["profile"], g, i, which)
    run = RaysRun(p, r0, n0, ray_pwr_wt=power)
    res = run.trace_rays(ngpu=1, trajectories=False, deposition=("Ptotal_psi", nb))
    assert isinstance(res, RayDeposition) and res.work is None
    rec = res.profile_record
    np.testing.assert_array_equal(rec["profile"], g["dep_profile"][0])
    assert rec["Q_sum"] == float(g["dep_q_sum"][0]) and rec["grid_name"] == "psi" and len(rec["grid"]) == nb + 1
    np.testing.assert_array_equal(res.summaries.npoints, g["npoints_full"])
    with pytest.raises(ValueError, match="trajectories=False"):
        run.trace_rays(ngpu=1, deposition=("Ptotal_psi", nb))
    prev = hip.keep_last_result(True)
    try:
        hip.trace_host(p, r0, n0, ngpu=1)
        assert hip.deposition_last(p, "Ptotal_psi", nb, power) is not None
        hip.trace_deposition_host(p, r0, n0, power, "Ptotal_psi", nb, ngpu=1)
        assert hip.deposition_last(p, "Ptotal_psi", nb, power) is None
    finally:
        hip.keep_last_result(prev)


# ---- 6. memory -----------------------------------------------------------------------------------------------------------------
def test_cfg5b_shape_needs_no_trajectory_memory():
    """cfg 5b's shape (262 144 eqdsk rays with damping) at 100 bins.  hipMemGetInfo before the first call and after
    the stream is synchronised: device memory in use grows by less than n_bins * 8 + 1024 bytes per ray (the
    trajectories are 72 (nstep_max + 1) bytes per ray: 14 KB as the config stands, 64 KB at nstep_max = 1000).  Every 512th ray's row of work equals the two-step path's on those rays
    alone."""
    import torch

    import bench
    from rays_amd.trace import DeviceTrace
    nml, p, r0, n0 = bench.build_fan(os.path.join(ROOT, "configs", "cfg5b_axisym256k_rk4_damp.in"), 1)
    nray, nb = len(r0), 100
    assert nray == 262144 and p.nv == 8
    assert hip.deposition_kernel_name(p, nray) == "rk4_trace_kernel<102, 2, 0, 8>"
    power = _distinct_powers(nray)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free_before, _ = torch.cuda.mem_get_info()
    tr = DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_psi", nb, power))
    tr.launch()
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info()
    grown = free_before - free_after
    print(f"device memory in use grew by {grown} bytes = {grown / nray:.1f} B per ray")
    assert grown < (nb * 8 + 1024) * nray
    sel = np.arange(0, nray, 512)
    rows = tr.work[:, torch.as_tensor(sel).cuda()].cpu().numpy().T
    npoints = tr.npoints.cpu().numpy()
    prof = tr.profile.cpu().numpy()
    del tr
    torch.cuda.empty_cache()
    ref = _two_step(p, r0[sel], n0[sel], power[sel], "Ptotal_psi", nb)
    np.testing.assert_array_equal(npoints[sel], ref["npoints"])
    np.testing.assert_array_equal(rows, ref["work"])
    assert rows.any() and prof.sum() > 0.0


# ---- 7. the numerics setting ------------------------------------------------------------------------------------------------------
def test_tolerance_setting_still_runs_the_exact_kernels():
    g, nml, p = _load("gold_slab16_damp_rk4")
    r0, n0, nb = g["rvec0_full"], g["rindex_vec0_full"], int(g["dep_n_bins"])
    prev = hip.set_numerics("tolerance")
    try:
        assert hip.get_numerics() == "tolerance"
        assert hip.deposition_kernel_name(p, len(r0)) == "rk4_trace_kernel<100, 2, 0, 8>"
        out = _fused(p, r0, n0, g["dep_power"], "Ptotal_x", nb)
        fl.assert_golden_deposition(out["work"], out["profile"], g, 0, "device entry")
        fl.assert_golden_summaries(out, g, "device entry")
        host = hip.trace_deposition_host(p, r0, n0, g["dep_power"], "Ptotal_x", nb, ngpu=1)
        fl.assert_golden_deposition(host["work"], host["profile"], g, 0, "host entry")
    finally:
        hip.set_numerics(prev)
    assert hip.get_numerics() == prev


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    import torch
    lib = hip.load()
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    ok = dict(r=d.data_ptr(), n=d.data_ptr(), pw=d.data_ptr(), np_=i.data_ptr(), sc=i.data_ptr(), ev=d.data_ptr(),
              er=d.data_ptr(), mr=d.data_ptr(), work=d.data_ptr(), out=d.data_ptr())

    def dev(p, nray, which, n_bins, **kw):
        a = dict(ok, **kw)
        return lib.rays_hip_trace_deposition_device(C.byref(p), nray, a["r"], a["n"], a["pw"], hip.DEP_PROFILES[which],
                                                    n_bins, a["np_"], a["sc"], None, a["ev"], a["er"], a["mr"], a["work"],
                                                    None, a["out"], None)

    def refused(rc, text):
        assert rc != 0 and text in hip.last_error(), hip.last_error()

    g, nml, slab = _load("gold_slab16_damp_rk4")
    who = "rays_hip_trace_deposition_device"
    refused(dev(slab, -1, "Ptotal_x", 10), who + ": nray < 0")
    for nb in (0, -3, 321):
        refused(dev(slab, 1, "Ptotal_x", nb), f"{who}: n_bins = {nb} is outside 1..320")
    for which in ("Ptotal_psi", "Ptotal_rho"):
        refused(dev(slab, 1, which, 10), "unimplemented profile for this equilib_model")
    for key in ok:
        refused(dev(slab, 1, "Ptotal_x", 10, **{key: None}), who + ": null device pointer")
    assert dev(slab, 0, "Ptotal_x", 10, r=None, work=None) == 0      # nothing to trace: the carried profile, or zeros
    g, nml, nodamp = load_golden("cfg1_slab16_rk4")
    refused(dev(nodamp, 1, "Ptotal_x", 10), who + ": needs a run with damping")
    g, nml, sol = load_golden("gold_solovev64_damp_rk4")
    refused(dev(sol, 1, "Ptotal_psi", 10), "initialize_deposition_profiles: unimplemented equilib_model")
    g, nml, solmag = _load("gold_axisym64_solmag_damp_rk4")
    refused(dev(solmag, 1, "Ptotal_rho", 10), "rho is only implemented for eqdsk_magnetics_spline_interp")
    refused(dev(solmag, 1, "Ptotal_x", 10), "unimplemented profile for this equilib_model")
    # the host form names itself
    h, hi = np.zeros(4096), np.zeros(8, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    hd, hp = h.ctypes.data_as(dp), hi.ctypes.data_as(ip)

    def host(p, nray, which, n_bins, power=hd, profile=hd):
        return lib.rays_hip_trace_deposition(C.byref(p), nray, hd, hd, power, hip.DEP_PROFILES[which], n_bins, hp, hp,
                                             None, hd, hd, hd, None, profile, None)
    refused(host(slab, -1, "Ptotal_x", 10), "rays_hip_trace_deposition: nray < 0")
    refused(host(slab, 1, "Ptotal_x", 0), "rays_hip_trace_deposition: n_bins = 0 is outside 1..320")
    refused(host(slab, 1, "Ptotal_x", 10, power=None), "rays_hip_trace_deposition: null array argument")
    refused(host(slab, 1, "Ptotal_x", 10, profile=None), "rays_hip_trace_deposition: null array argument")
    refused(host(nodamp, 1, "Ptotal_x", 10), "rays_hip_trace_deposition: needs a run with damping")
    # a shape the library was not built with is refused by the message of every other entry
    q = copy_params(slab)
    q.nspec, q.nv = 4, 8
    if lib.rays_hip_check_params(C.byref(q)) != 0 and "no kernel built for this configuration" in hip.last_error():
        msg = hip.last_error()
        assert dev(q, 1, "Ptotal_x", 10) != 0 and hip.last_error() == msg
        assert lib.rays_hip_deposition_kernel_name_for(C.byref(q), 1) == b""
    # the Python layer
    from rays_amd.trace import DeviceTrace
    with pytest.raises(ValueError, match="trajectories=False"):
        DeviceTrace(slab, g["rvec0"], g["rindex_vec0"], deposition=("Ptotal_x", 10, np.ones(len(g["rvec0"]))))
    with pytest.raises(ValueError, match="known are"):
        DeviceTrace(slab, g["rvec0"], g["rindex_vec0"], trajectories=False, deposition=("Ptotal", 10, np.ones(len(g["rvec0"]))))
    torch.cuda.synchronize()


_NO_RHO_TABLE = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
from rays_amd import hip
from tests.common import load_golden
g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")   # hands over the eqdsk tables, never a rho table
hip.ensure_tables(p)
lib = hip.load()
rc = lib.rays_hip_trace_deposition_device(C.byref(p), 1, None, None, None, hip.DEP_PROFILES["Ptotal_rho"], 10, None, None,
                                          None, None, None, None, None, None, None, None)
print("RC", rc, hip.last_error())
h = (C.c_double * 64)()
hi = (C.c_int32 * 8)()
rc = lib.rays_hip_trace_deposition(C.byref(p), 1, h, h, h, hip.DEP_PROFILES["Ptotal_rho"], 10, hi, hi, None, h, h, h, None, h, None)
print("RC", rc, hip.last_error())
"""


def test_ptotal_rho_without_a_rho_table_is_refused():
    """'Ptotal_rho' in a process that never called rays_hip_set_rho_table: both entries refuse by name, before they look
    at a pointer.  (A fresh process: the library has no way to forget a table.)"""
    import sys
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _NO_RHO_TABLE.format(root=ROOT)],
                       capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RC ")]
    assert r.returncode == 0 and len(lines) == 2, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    for l in lines:
        assert l.split()[1] != "0" and "Ptotal_rho needs rays_hip_set_rho_table() first" in l, l


# ---- 9. the Fortran driver ----------------------------------------------------------------------------------------------------------
def test_fortran_driver_reproduces_the_python_path(tmp_path):
    """tests/fortran/fused_deposition_driver.f90 + the binding, built with amdflang and linked against librays_hip.so:
    rays_hip_trace_deposition returns the Python path's bytes."""
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    libdir = os.path.join(ROOT, "rays_amd", "lib")
    hipdir = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    srcs = [os.path.join(ROOT, "fortran", "rays_hip_m.f90"), os.path.join(ROOT, "tests", "fortran", "fused_deposition_driver.f90")]
    exe = str(tmp_path / "fused_deposition_driver")
    subprocess.check_call([fc, "-O2", "-ffp-contract=off", "-w", "-o", exe] + srcs +
                          ["-L" + libdir, "-lrays_hip", "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + hipdir], cwd=str(tmp_path))
    g, nml, p = _load("gold_slab16_damp_rk4")   # a slab: the driver needs no table
    r0, n0, power, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], 37
    nray, nv = len(r0), p.nv
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([nray, nv, nb, hip.DEP_PROFILES["Ptotal_x"]], dtype=np.int32).tobytes())
        f.write(bytes(p))
        for a in (r0, n0, power):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    with open(str(tmp_path / "zfun.bin"), "wb") as f:
        f.write(np.array([len(z["fspl_re"])], dtype=np.int32).tobytes())
        f.write(np.array([float(z["x_min"]), float(z["x_max"])]).tobytes())
        f.write(np.ascontiguousarray(z["fspl_re"], dtype=np.float64).tobytes())
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, str(tmp_path / "zfun.bin"), fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8)
    want = hip.trace_deposition_host(p, r0, n0, power, "Ptotal_x", nb, ngpu=1)
    off = 0
    for k, shape in [("npoints", (nray,)), ("stop_code", (nray,)), ("start_ray_vec", (nray, nv)), ("end_ray_vec", (nray, nv)),
                     ("end_residuals", (nray,)), ("max_residuals", (nray,)), ("work", (nray, nb)), ("profile", (nb,))]:
        integer = k in ("npoints", "stop_code")
        nbytes = int(np.prod(shape)) * (4 if integer else 8)
        got = raw[off:off + nbytes].view(np.int32 if integer else np.float64).reshape(shape)
        np.testing.assert_array_equal(got, want[k], err_msg="Fortran: " + k)
        off += nbytes
    assert off == raw.size
