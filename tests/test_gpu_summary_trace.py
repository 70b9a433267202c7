"""GPU tier: summary-only tracing -- rays_hip_trace_summary_device / rays_hip_scan_summary_device /
rays_hip_trace_summary and the kernels they launch (EQ + 32 in their names: no trajectory point is recorded, no
trajectory array exists).  Everything is compared on bit patterns: with the golden files, with the full trace of the
same rays in the same process, with the oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.namelist import read_namelist
from rays_amd.params import copy_params, params_from_namelist
from rays_amd.ray_init import fan_from_namelist
from tests import oracle_lib
from tests import summary_lib as sl
from tests.common import GOLDEN_CASES, ROOT, load_golden

pytestmark = pytest.mark.gpu


def _fan(cfg, overrides, tables=None, nray=None):
    """Namelist -> (params, rvec0, rindex_vec0), the fan built by the device launcher, cut to its first `nray` rays."""
    nml = read_namelist(os.path.join(ROOT, "configs", cfg))
    for group, kv in overrides.items():
        nml[group].update(kv)
    p = params_from_namelist(nml, tables)
    fan, nray_max = fan_from_namelist(nml)
    r0, n0, _ = hip.ray_init_host(p, fan, nray_max)
    if nray is not None:
        assert len(r0) >= nray
        r0, n0 = r0[:nray].copy(), n0[:nray].copy()
    return p, r0, n0


def _summary(p, r0, n0):
    """rays_hip_trace_summary_device through DeviceTrace(trajectories=False)."""
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0, trajectories=False)
    assert tr.ray_vec is None and tr.residual is None
    tr.launch()
    res = tr.results()
    return {k: getattr(res, k) for k in sl.KEYS}


def _full_summaries(p, r0, n0):
    """The summaries of rays_hip_trace_device on the same inputs (point 1 cut out on the device)."""
    import torch
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0)
    tr.launch()
    torch.cuda.synchronize()
    out = {k: getattr(tr, k).cpu().numpy() for k in sl.KEYS if k != "start_ray_vec"}
    out["start_ray_vec"] = tr.ray_vec[:, 0, :].contiguous().cpu().numpy()
    del tr
    torch.cuda.empty_cache()
    return out


def _resident_lanes():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


# ---- 1. fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_fixture_summaries_equal_golden(name):
    """All 38 fixtures (slab / Solovev / axisym, RK4 / SG, cold / finite-difference dD, damping, multi-species damping,
    gradients, 1 to 6 species): summaries equal the golden files', start_ray_vec the golden ray_vec[:, 0, :]."""
    g, nml, p = load_golden(name)
    # the recording kernel of this shape with the "no trajectory" bit in its EQ argument
    head, rest = hip.kernel_name(p, len(g["rvec0"])).split("<", 1)
    eq, tail = rest.split(",", 1)
    assert hip.summary_kernel_name(p, len(g["rvec0"])) == f"{head}<{int(eq) + 32},{tail}"
    sl.assert_same(_summary(p, g["rvec0"], g["rindex_vec0"]), sl.golden_summaries(g), name)


# ---- 2. the one-wave RK4 kernel with several rays per lane -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["slab", "solovev"])
def test_rk4_one_wave_kernel_refill_and_long_first_order(which):
    """70 000 rays, just above one wave per SIMD on 256 CUs, nstep_max = 40: lanes are refilled and the rays handed out
    long-first.  Summaries equal those of rays_hip_trace_device on the same inputs in the same process."""
    if which == "slab":
        p, r0, n0 = _fan("cfg4_slab1M_rk4.in", {
            "simple_slab_ray_init_list": dict(n_ky_launch=265, n_kz_launch=265, delta_rindex_y0=0.2 / 265,
                                              delta_rindex_z0=0.2 / 265),
            "ode_list": dict(nstep_max=40)}, nray=70000)
        want = "rk4_trace_kernel<36, 2, 0, 7>"
    else:
        p, r0, n0 = _fan("cfg3b_solovev64k_rk4.in", {
            "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=265, n_rindex_phi=265,
                                                      delta_rindex_theta=0.31 / 265, delta_rindex_phi=0.3875 / 265),
            "ray_init_list": dict(nray_max=265 * 265), "ode_list": dict(nstep_max=40)}, nray=70000)
        want = "rk4_trace_kernel<37, 2, 0, 7>"
    assert len(r0) == 70000 > _resident_lanes()
    assert hip.summary_kernel_name(p, len(r0)) == want
    out = _summary(p, r0, n0)
    assert out["npoints"].min() >= 1 and out["npoints"].max() == 41
    sl.assert_same(out, _full_summaries(p, r0, n0), which)


# ---- 3. the two-waves build ---------------------------------------------------------------------------------------------------
def test_rk4_two_waves_build():
    """A 132 000-ray Solovev fan, nstep_max = 40: the _w2 variant is the one dispatched, and equals the full trace."""
    p, r0, n0 = _fan("cfg3b_solovev64k_rk4.in", {
        "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=364, n_rindex_phi=364,
                                                  delta_rindex_theta=0.31 / 364, delta_rindex_phi=0.3875 / 364),
        "ray_init_list": dict(nray_max=364 * 364), "ode_list": dict(nstep_max=40)}, nray=132000)
    assert hip.summary_kernel_name(p, len(r0)) == "rk4_trace_kernel_w2<37, 2, 0, 7>"
    assert hip.kernel_name(p, len(r0)) == "rk4_trace_kernel_w2<5, 2, 0, 7>"
    out = _summary(p, r0, n0)
    assert out["npoints"].min() >= 1
    sl.assert_same(out, _full_summaries(p, r0, n0))


# ---- 4. SG refill ---------------------------------------------------------------------------------------------------------------
def _tiled(r0, n0, nray):
    reps = nray // len(r0) + 1
    return np.tile(r0, (reps, 1))[:nray].copy(), np.tile(n0, (reps, 1))[:nray].copy()


@pytest.mark.parametrize("which", ["sg_trace_kernel", "sg_group_kernel"])
def test_sg_kernels_refill(which):
    """More rays than resident lanes (sg_trace_kernel: one 256-lane block per CU; sg_group_kernel: four lanes per ray,
    up to four blocks per CU), nstep_max = 10, against the full trace."""
    if which == "sg_trace_kernel":
        g, nml, p0 = load_golden("gold_solovev64_sg_cold")
        p = copy_params(p0)
        nray, want = _resident_lanes() + 4500, "sg_trace_kernel<37, 2, 0, 7>"
        r0, n0 = _tiled(g["rvec0_full"], g["rindex_vec0_full"], nray)
    else:
        p, f0, fn = _fan("cfg3_solovev64k_sg_num.in", {
            "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=32, n_rindex_phi=32,
                                                      delta_rindex_theta=0.01, delta_rindex_phi=0.0125)})
        nray, want = _resident_lanes() + 40000, "sg_group_kernel<37, 2, 4>"   # > 4 blocks x 64 groups per CU
        r0, n0 = _tiled(f0, fn, nray)
    p.nstep_max = 10
    r0[7, 0] = 10.0      # outside the box
    n0[11] *= 3.0        # stops at the initial check_save
    assert hip.summary_kernel_name(p, nray) == want
    out = _summary(p, r0, n0)
    assert out["npoints"][7] == 1 and out["npoints"][11] == 1 and out["npoints"].max() > 2
    sl.assert_same(out, _full_summaries(p, r0, n0), which)


# ---- 5. the scan -------------------------------------------------------------------------------------------------------------------
def test_scan_summary():
    """3 runs x 16 rays with distinct ds: each run equals its stand-alone summary trace and the full scan's summaries."""
    from rays_amd.scan import RayScan
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::64].copy(), g["rindex_vec0_full"][::64].copy()
    n0[3] *= 3.0
    assert len(r0) == 16
    ds = [float(p.ds), 0.5 * float(p.ds), 1.7 * float(p.ds)]
    scan = RayScan(p, r0, n0, ds, trajectories=False)
    assert scan.ray_vec is None and scan.residual is None
    scan.launch()
    res = scan.results()
    full = RayScan(p, r0, n0, ds)
    full.launch()
    fres = full.results()
    assert len({int(r.npoints.sum()) for r in res}) == 3
    for k, (d, r) in enumerate(zip(ds, res)):
        q = copy_params(p)
        q.ds = d
        run = {key: getattr(r, key) for key in sl.KEYS}
        sl.assert_same(run, _summary(q, r0, n0), f"run {k} against its stand-alone summary trace")
        f = fres[k]
        sl.assert_same(run, sl.summaries_of({key: getattr(f, key) for key in
                                             ("npoints", "stop_code", "ray_vec", "end_ray_vec", "end_residuals",
                                              "max_residuals")}), f"run {k} against the full scan")


# ---- 6. the host entry ------------------------------------------------------------------------------------------------------------
def test_host_entry_equals_rays_hip_trace():
    """rays_hip_trace_summary equals rays_hip_trace's summaries on a fixture (1001 rays of cfg 2's fan), also with three
    slots on one device; a kept result image does not survive it."""
    from rays_amd.trace import RaysRun, RaySummaries
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][:1001], g["rindex_vec0_full"][:1001]
    ref = sl.summaries_of(hip.trace_host(p, r0, n0, ngpu=1))
    out = hip.trace_summary_host(p, r0, n0, ngpu=1)
    sl.assert_same(out, ref)
    sub = [int(i) for i in g["ray_index"] if i < 1001]
    np.testing.assert_array_equal(out["npoints"][sub], g["npoints"][:len(sub)])
    np.testing.assert_array_equal(out["end_ray_vec"][sub], g["end_ray_vec"][:len(sub)])
    hip.init_devices([0, 0, 0])
    try:
        sl.assert_same(hip.trace_summary_host(p, r0, n0, ngpu=None), ref, "three slots")
    finally:
        hip.load().rays_hip_init(1)
    res = RaysRun(p, r0, n0).trace_rays(ngpu=1, trajectories=False)
    assert isinstance(res, RaySummaries) and res.total_steps == int((ref["npoints"].astype(np.int64) - 1).sum())
    # the image an earlier rays_hip_trace kept is not this call's result: dropped, and none is left
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], int(g["dep_n_bins"])
    prev = hip.keep_last_result(True)
    try:
        full = hip.trace_host(p, r0, n0, ngpu=1)
        assert hip.deposition_last(p, "Ptotal_psi", nb, power) is not None
        sl.assert_same(hip.trace_summary_host(p, r0, n0, ngpu=1), sl.summaries_of(full), "eqdsk + damping")
        assert hip.deposition_last(p, "Ptotal_psi", nb, power) is None
    finally:
        hip.keep_last_result(prev)


# ---- 7. the numerics setting --------------------------------------------------------------------------------------------------------
def test_tolerance_setting_still_runs_the_exact_kernels():
    """Under rays_hip_set_numerics(TOLERANCE) the summary entries return the exact kernels' results, golden bit for bit,
    on cfg 2 (whose rays end at the mode coalescence, where the tolerance kernels hand steps over)."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    prev = hip.set_numerics("tolerance")
    try:
        assert hip.get_numerics() == "tolerance"
        assert hip.kernel_name(p, len(g["rvec0"])) == "rk4_trace_kernel<21, 2, 0, 7>"
        assert hip.summary_kernel_name(p, len(g["rvec0"])) == "rk4_trace_kernel<37, 2, 0, 7>"
        want = sl.golden_summaries(g)
        sl.assert_same(_summary(p, g["rvec0"], g["rindex_vec0"]), want, "device entry")
        sl.assert_same(hip.trace_summary_host(p, g["rvec0"], g["rindex_vec0"], ngpu=1), want, "host entry")
    finally:
        hip.set_numerics(prev)
    assert hip.get_numerics() == prev


# ---- 8. memory ------------------------------------------------------------------------------------------------------------------------
def test_cfg4_shape_needs_no_trajectory_memory():
    """cfg 4's shape (1 048 576 slab rays, nstep_max = 500) summary-only.  hipMemGetInfo before the first call and after
    the stream is synchronised: device memory in use grows by less than 1 KB per ray (the summaries are 136 B per ray,
    the inputs 48 B; the trajectories would be 32 KB per ray).  Every 4096th ray equals the oracle."""
    import torch
    from rays_amd.trace import DeviceTrace
    p, r0, n0 = _fan("cfg4_slab1M_rk4.in", {})
    assert len(r0) == 1024 * 1024 and p.nstep_max == 500
    assert hip.summary_kernel_name(p, len(r0)) == "rk4_trace_kernel_w2<36, 2, 0, 7>"
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free_before, _ = torch.cuda.mem_get_info()
    tr = DeviceTrace(p, r0, n0, trajectories=False)
    tr.launch()
    torch.cuda.synchronize()
    free_after, _ = torch.cuda.mem_get_info()
    grown = free_before - free_after
    print(f"device memory in use grew by {grown} bytes = {grown / len(r0):.1f} B per ray")
    assert grown < 1024 * len(r0)
    res = tr.results()
    assert int((res.npoints.astype(np.int64) - 1).sum()) == 524242966               # steps per pass
    sel = np.arange(0, len(r0), 4096)
    ora = sl.summaries_of(oracle_lib.trace(p, r0[sel], n0[sel], nthreads=os.cpu_count() or 1))
    sl.assert_same({k: getattr(res, k)[sel] for k in sl.KEYS}, ora)
    del tr
    torch.cuda.empty_cache()


# ---- 9. refusals and the Fortran driver -------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    import torch
    g, nml, p = load_golden("cfg1_slab16_rk4")
    lib = hip.load()
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    ok = dict(r=d.data_ptr(), n=d.data_ptr(), np_=i.data_ptr(), sc=i.data_ptr(), ev=d.data_ptr(), er=d.data_ptr(),
              mr=d.data_ptr())

    def dev(nray, **kw):
        a = dict(ok, **kw)
        return lib.rays_hip_trace_summary_device(C.byref(p), nray, a["r"], a["n"], a["np_"], a["sc"], None, a["ev"], a["er"],
                                                 a["mr"], None)

    def scan(n_runs, nray, ds=d.data_ptr(), **kw):
        a = dict(ok, **kw)
        return lib.rays_hip_scan_summary_device(C.byref(p), n_runs, ds, nray, a["r"], a["n"], a["np_"], a["sc"], None,
                                                a["ev"], a["er"], a["mr"], None)

    assert dev(-1) != 0 and "rays_hip_trace_summary_device: nray < 0" in hip.last_error()
    for key in ok:
        assert dev(1, **{key: None}) != 0 and "rays_hip_trace_summary_device: null device pointer" in hip.last_error(), key
    assert dev(0, r=None) == 0                                   # nothing to trace: nothing is looked at
    assert scan(-1, 1) != 0 and "rays_hip_scan_summary_device: n_runs, nray < 0" in hip.last_error()
    assert scan(1 << 16, 1 << 16) != 0 and "rays_hip_scan_summary_device: n_runs * nray exceeds 2^31 - 1" in hip.last_error()
    assert scan(1, 1, ds=None) != 0 and "rays_hip_scan_summary_device: null device pointer" in hip.last_error()
    h = np.zeros(8)
    hi = np.zeros(1, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    hd = h.ctypes.data_as(dp)
    assert lib.rays_hip_trace_summary(C.byref(p), -1, hd, hd, hi.ctypes.data_as(ip), hi.ctypes.data_as(ip), None, hd, hd,
                                      hd, None) != 0 and "rays_hip_trace_summary: nray < 0" in hip.last_error()
    assert lib.rays_hip_trace_summary(C.byref(p), 1, hd, hd, hi.ctypes.data_as(ip), None, None, hd, hd, hd, None) != 0 \
        and "rays_hip_trace_summary: null array argument" in hip.last_error()
    # a shape the library was not built with is refused by the message of every other entry
    q = copy_params(p)
    q.nspec, q.nv = 4, 7
    if lib.rays_hip_check_params(C.byref(q)) != 0 and "no kernel built for this configuration" in hip.last_error():
        msg = hip.last_error()
        assert lib.rays_hip_trace_summary_device(C.byref(q), 1, ok["r"], ok["n"], ok["np_"], ok["sc"], None, ok["ev"],
                                                 ok["er"], ok["mr"], None) != 0
        assert hip.last_error() == msg
        assert lib.rays_hip_summary_kernel_name_for(C.byref(q), 1) == b""
    torch.cuda.synchronize()


def test_fortran_driver_reproduces_the_python_path(tmp_path):
    """tests/fortran/summary_trace_driver.f90 + the binding, built with amdflang and linked against librays_hip.so and
    the HIP runtime: rays_hip_trace_summary and one rays_hip_scan_summary_device launch over three runs return the
    Python path's bytes."""
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    from rays_amd.scan import RayScan
    libdir = os.path.join(ROOT, "rays_amd", "lib")
    hipdir = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    srcs = [os.path.join(ROOT, "fortran", "rays_hip_m.f90"), os.path.join(ROOT, "tests", "fortran", "summary_trace_driver.f90")]
    exe = str(tmp_path / "summary_trace_driver")
    subprocess.check_call([fc, "-O2", "-ffp-contract=off", "-w", "-o", exe] + srcs +
                          ["-L" + libdir, "-lrays_hip", "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + hipdir], cwd=str(tmp_path))
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::16].copy(), g["rindex_vec0_full"][::16].copy()
    n0[3] *= 3.0
    ds = np.array([float(p.ds), 0.5 * float(p.ds), 1.7 * float(p.ds)])
    nray, nv, R = len(r0), p.nv, len(ds)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([nray, nv, R], dtype=np.int32).tobytes())
        f.write(bytes(p))
        for a in (r0, n0, ds):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8)

    def take(off, runs):
        out = {}
        for k in sl.KEYS:
            integer = k in ("npoints", "stop_code")
            shape = ((runs,) if runs else ()) + (nray,) + (() if k in ("npoints", "stop_code", "end_residuals",
                                                                          "max_residuals") else (nv,))
            nbytes = int(np.prod(shape)) * (4 if integer else 8)
            out[k] = raw[off:off + nbytes].view(np.int32 if integer else np.float64).reshape(shape)
            off += nbytes
        return out, off
    host, off = take(0, 0)
    scan, off = take(off, R)
    assert off == raw.size
    sl.assert_same(host, _summary(p, r0, n0), "Fortran: rays_hip_trace_summary")
    want = RayScan(p, r0, n0, ds, trajectories=False)
    want.launch()
    for k, res in enumerate(want.results()):
        sl.assert_same({key: scan[key][k] for key in sl.KEYS}, {key: getattr(res, key) for key in sl.KEYS},
                       f"Fortran: scan run {k}")
