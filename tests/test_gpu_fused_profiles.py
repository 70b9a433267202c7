"""GPU tier: fused deposition into both axisym_toroid profiles in ONE trace pass -- rays_hip_trace_profiles_device /
rays_hip_trace_profiles and the kernels they launch (EQ + 352 in their names: the fused deposition kernels that bin every
accepted point into two rows from one grid evaluation).  Everything is compared on bit patterns: with the reference
post-processor's work / profile / Q_sum in the golden files, and with rays_hip_trace_deposition_device (pinned by
tests/test_gpu_fused_deposition.py) called once per profile on the same rays.  No tolerance appears anywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import fused_deposition_lib as fl
from tests import fused_profiles_lib as pl
from tests import summary_lib as sl
from tests.common import ROOT, load_golden
from tests.test_gpu_fused_deposition import _distinct_powers, _fused, _load, _resident_lanes, _tiled

pytestmark = pytest.mark.gpu


def _profiles(p, r0, n0, power, specs, profile_in=None):
    """rays_hip_trace_profiles_device through DeviceTrace(deposition=[...]): summaries, works[i][nray][n_bins], profiles."""
    import torch
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0, trajectories=False, deposition=list(specs), ray_power=power, profile_in=profile_in)
    assert tr.ray_vec is None and tr.residual is None
    for w in tr.works:
        w.fill_(float("nan"))   # the call zeroes every work itself
    tr.launch()
    res = tr.results()
    out = {k: getattr(res[0].summaries, k) for k in sl.KEYS}
    assert all(r.summaries is res[0].summaries for r in res) and [r.profile_name for r in res] == [w for w, _ in specs]
    out["works"] = [r.work for r in res]
    out["profiles"] = [r.profile for r in res]
    del tr
    torch.cuda.empty_cache()
    return out


def _singles(p, r0, n0, power, specs):
    return [_fused(p, r0, n0, power, w, nb) for w, nb in specs]


# ---- 1. fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", pl.ORDERS, ids=["psi_rho", "rho_psi"])
@pytest.mark.parametrize("name", pl.TWO_PROFILE_FIXTURES)
def test_fixture_profiles_equal_golden(name, order):
    """The six fixtures with both profiles of the reference post-processor (RK4 / SG, cold / finite-difference dD, the
    65 x 65 and 129 x 129 tables): both from one pass, in both request orders; the kernel is the fused one + 256."""
    g, nml, p = _load(name)
    r0, n0 = g["rvec0_full"], g["rindex_vec0_full"]
    head, rest = hip.deposition_kernel_name(p, len(r0)).split("<", 1)
    eq, tail = rest.split(",", 1)
    assert hip.profiles_kernel_name(p, len(r0), 2) == f"{head}<{int(eq) + 256},{tail}"
    assert hip.profiles_kernel_name(p, len(r0), 1) == hip.deposition_kernel_name(p, len(r0))
    assert hip.deposition_profile_set(p) == ("Ptotal_psi", "Ptotal_rho")
    names, nb = fl.profile_names(g), int(g["dep_n_bins"])
    out = _profiles(p, r0, n0, g["dep_power"], [(w, nb) for w in order])
    for k, w in enumerate(order):
        fl.assert_golden_deposition(out["works"][k], out["profiles"][k], g, names.index(w), f"{name} {w}")
    fl.assert_golden_summaries(out, g, name)


# ---- 2. bin-count pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [(1, 320), (320, 1), (7, 100)])
def test_bin_count_pairs_equal_two_single_passes(bins):
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_psi", bins[0]), ("Ptotal_rho", bins[1])]
    out = _profiles(p, r0, n0, power, specs)
    assert out["profiles"][0].sum() > 0.0 and out["profiles"][1].sum() > 0.0
    pl.assert_same_as_single(out, _singles(p, r0, n0, power, specs), str(bins))


def test_first_segment_starts_at_each_profiles_own_grid_value():
    """No fixture ray absorbs power in its first segment, so the grid values of point 1 never reach a row there.  Rays
    launched inside the absorption layer (tests/test_cpu_fused_profiles.py) deposit from their first segment on."""
    from tests.test_cpu_fused_profiles import _rays_inside_the_absorption_layer
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0 = _rays_inside_the_absorption_layer(g)
    power = g["dep_power"][:len(r0)]
    specs = [("Ptotal_psi", 7), ("Ptotal_rho", 100)]
    out = _profiles(p, r0, n0, power, specs)
    assert (out["npoints"] > 5).all() and (out["end_ray_vec"][:, 7] > 0.0).all()
    pl.assert_same_as_single(out, _singles(p, r0, n0, power, specs), "rays inside the layer")


# ---- 3. refill -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["rk4", "sg"])
def test_refilled_lanes_start_their_ray_afresh(solver):
    """The 64 rays of the eqdsk + damping fixture tiled to resident lanes + 4500 rays (RK4: nstep_max = 40; SG:
    nstep_max = 10), every ray with a power of its own, one ray outside the box and one refused at its initial check:
    both works, both profiles and the summaries equal the two single-profile passes'."""
    g, nml, p0 = _load("gold_axisym64_eqdsk_damp_rk4" if solver == "rk4" else "gold_axisym64_eqdsk_damp_sg")
    p = copy_params(p0)
    p.nstep_max = 40 if solver == "rk4" else 10
    nray = _resident_lanes() + 4500
    r0, n0 = _tiled(g["rvec0_full"], g["rindex_vec0_full"], nray)
    r0[7, 0] = 10.0      # outside the box
    n0[11] *= 3.0        # stops at the initial check_save
    power = _distinct_powers(nray)
    want = ("rk4_trace_kernel" if solver == "rk4" else "sg_trace_kernel") + "<358, 2, 0, 8>"
    assert hip.profiles_kernel_name(p, nray, 2) == want
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 100)]
    out = _profiles(p, r0, n0, power, specs)
    assert out["npoints"][7] == 1 and out["npoints"][11] == 1 and out["npoints"].max() == p.nstep_max + 1
    for w in out["works"]:
        assert w.any() and not w[7].any() and not w[11].any()   # one point, no segment
    pl.assert_same_as_single(out, _singles(p, r0, n0, power, specs), solver)


# ---- 4. chaining ------------------------------------------------------------------------------------------------------------
def test_two_blocks_chained_through_profile_in_equal_one_call():
    import torch
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], int(g["dep_n_bins"])
    specs = [("Ptotal_psi", nb), ("Ptotal_rho", 33)]
    h = 29
    whole = _profiles(p, r0, n0, power, specs)
    first = _profiles(p, r0[:h], n0[:h], power[:h], specs)
    carry = [torch.as_tensor(q).cuda() for q in first["profiles"]]
    second = _profiles(p, r0[h:], n0[h:], power[h:], specs, profile_in=carry)
    for k in range(2):
        np.testing.assert_array_equal(second["profiles"][k], whole["profiles"][k])
        np.testing.assert_array_equal(np.concatenate([first["works"][k], second["works"][k]]), whole["works"][k])
        assert not np.array_equal(first["profiles"][k], second["profiles"][k])
    # one carry alone: the other profile starts from zero
    third = _profiles(p, r0[h:], n0[h:], power[h:], specs, profile_in=[None, carry[1]])
    np.testing.assert_array_equal(third["profiles"][1], whole["profiles"][1])
    assert not np.array_equal(third["profiles"][0], whole["profiles"][0])


# ---- 5. the host form ---------------------------------------------------------------------------------------------------------
def test_host_entry_equals_the_device_form(tmp_path):
    """rays_hip_trace_profiles with one slot and with three slots on one device (blocks of 22, 22, 20 rays chained in ray
    order) equals the device form; RaysRun(deposition="all") returns the fixture's two records, and the LD file written
    from them equals the one written from the fixture's arrays."""
    from rays_amd import results
    from rays_amd.trace import RayDeposition, RaysRun
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_rho", 50), ("Ptotal_psi", 64)]
    ref = _profiles(p, r0, n0, power, specs)

    def same(out, what):
        sl.assert_same(out, ref, what)
        for k in range(2):
            np.testing.assert_array_equal(out["works"][k], ref["works"][k], err_msg=f"{what}: work {k}")
            np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][k], err_msg=f"{what}: profile {k}")
    same(hip.trace_profiles_host(p, r0, n0, power, specs, ngpu=1), "one slot")
    hip.init_devices([0, 0, 0])
    try:
        same(hip.trace_profiles_host(p, r0, n0, power, specs, ngpu=None), "three slots")
        nowork = hip.trace_profiles_host(p, r0, n0, power, specs, ngpu=None, want_work=False)
        assert nowork["works"] == [None, None]
        for k in range(2):
            np.testing.assert_array_equal(nowork["profiles"][k], ref["profiles"][k])
    finally:
        hip.load().rays_hip_init(1)
    run = RaysRun(p, r0, n0, ray_pwr_wt=power)
    recs = run.trace_rays(ngpu=1, trajectories=False, deposition="all", n_bins=100)
    names = fl.profile_names(g)
    assert len(recs) == 2 and all(isinstance(r, RayDeposition) for r in recs) and recs[0].summaries is recs[1].summaries
    assert [r.profile_name for r in recs] == names == ["Ptotal_psi", "Ptotal_rho"] and int(g["dep_n_bins"]) == 100
    for i, r in enumerate(recs):
        np.testing.assert_array_equal(r.profile, g["dep_profile"][i])
        assert r.Q_sum == float(g["dep_q_sum"][i]) and r.work is None
    np.testing.assert_array_equal(recs[0].summaries.npoints, g["npoints_full"])
    want = [dict(profile_name=n, grid_name=n.split("_")[1], profile=g["dep_profile"][i],
                 grid=results.deposition_grid(0.0, 1.0, 100), Q_sum=float(g["dep_q_sum"][i]), n_bins=100, grid_min=0.0,
                 grid_max=1.0) for i, n in enumerate(names)]
    fa, fb = str(tmp_path / "a.LD"), str(tmp_path / "b.LD")
    results.write_deposition_profiles_LD(fa, [r.profile_record for r in recs])
    results.write_deposition_profiles_LD(fb, want)
    assert open(fa, "rb").read() == open(fb, "rb").read() and os.path.getsize(fa) > 0


# ---- 6. one profile is the single-profile entry ---------------------------------------------------------------------------------
def test_one_profile_is_the_single_profile_entry():
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    prev = hip.get_numerics()
    for numerics in ("exact", "tolerance"):
        hip.set_numerics(numerics)
        try:
            assert hip.profiles_kernel_name(p, len(r0), 1) == "rk4_trace_kernel<102, 2, 0, 8>"
            assert hip.profiles_kernel_name(p, len(r0), 2) == "rk4_trace_kernel<358, 2, 0, 8>"
            for which in ("Ptotal_psi", "Ptotal_rho"):
                out = _profiles(p, r0, n0, power, [(which, 77)])
                pl.assert_same_as_single(out, [_fused(p, r0, n0, power, which, 77)], f"{numerics} {which}")
            two = _profiles(p, r0, n0, power, [("Ptotal_psi", 100), ("Ptotal_rho", 100)])
            for k in range(2):
                fl.assert_golden_deposition(two["works"][k], two["profiles"][k], g, k, f"{numerics} two profiles")
        finally:
            hip.set_numerics(prev)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    import torch
    lib = hip.load()
    d = torch.full((4096,), -7.0, dtype=torch.float64, device="cuda")
    i = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    D, I = d.data_ptr(), i.data_ptr()
    g, nml, axi = _load("gold_axisym64_eqdsk_damp_rk4")

    def records(specs):
        arr = (hip.DepProfileStruct * max(len(specs), 1))()
        for r, s in zip(arr, specs):
            r.which, r.n_bins, r.work, r.profile_in, r.profile = s
        return arr

    def dev(p, nray, specs, n_profiles=None, r=D):
        return lib.rays_hip_trace_profiles_device(C.byref(p), nray, r, D, D, len(specs) if n_profiles is None else n_profiles,
                                                  records(specs), I, I, None, D, D, D, None)

    def refused(rc, text):
        assert rc != 0 and text in hip.last_error(), hip.last_error()

    PSI, RHO, X = (hip.DEP_PROFILES[k] for k in ("Ptotal_psi", "Ptotal_rho", "Ptotal_x"))
    who = "rays_hip_trace_profiles_device"
    ok = [(PSI, 10, D, None, D), (RHO, 12, D, None, D)]
    refused(dev(axi, 1, ok, n_profiles=0), who + ": n_profiles = 0 is outside 1..2")
    refused(dev(axi, 1, ok, n_profiles=3), who + ": n_profiles = 3 is outside 1..2")
    refused(dev(axi, -1, ok), who + ": nray < 0")
    refused(dev(axi, 1, [ok[0], ok[0]]), who + ": the same profile twice")
    for nb in (0, -3, 321):
        refused(dev(axi, 1, [ok[0], (RHO, nb, D, None, D)]), f"{who}: n_bins = {nb} is outside 1..320")
    refused(dev(axi, 1, [ok[0], (X, 10, D, None, D)]), "unimplemented profile for this equilib_model")
    refused(dev(axi, 1, [ok[0], (RHO, 12, None, None, D)]), who + ": null work or profile")
    refused(dev(axi, 1, [(PSI, 10, D, None, None), ok[1]]), who + ": null work or profile")
    refused(dev(axi, 1, [(PSI, 10, None, None, D)]), who + ": null work or profile")
    refused(dev(axi, 1, ok, r=None), who + ": null device pointer")
    # two profiles on a configuration that has one: the single-profile refusal's message
    gs, nmls, slab = _load("gold_slab16_damp_rk4")
    refused(dev(slab, 1, [(X, 10, D, None, D), (PSI, 10, D, None, D)]), "unimplemented profile for this equilib_model")
    refused(dev(slab, 1, [(X, 10, D, None, D), (X, 12, D, None, D)]), who + ": the same profile twice")
    g2, nml2, solmag = _load("gold_axisym64_solmag_damp_rk4")
    refused(dev(solmag, 1, ok), "rho is only implemented for eqdsk_magnetics_spline_interp")
    g3, nml3, nodamp = load_golden("cfg1_slab16_rk4")
    refused(dev(nodamp, 1, [(X, 10, D, None, D)]), who + ": needs a run with damping")
    g4, nml4, sol = load_golden("gold_solovev64_damp_rk4")
    refused(dev(sol, 1, ok), "initialize_deposition_profiles: unimplemented equilib_model")
    assert hip.deposition_profile_set(slab) == ("Ptotal_x",) and hip.deposition_profile_set(sol) == ()
    assert hip.deposition_profile_set(solmag) == ("Ptotal_psi",)
    assert hip.profiles_kernel_name(slab, 16, 2) == "" and hip.profiles_kernel_name(sol, 16, 2) == ""
    # the host form names itself, and takes no carry
    h, hi = np.full(4096, -7.0), np.full(8, -7, dtype=np.int32)
    H, HI = h.ctypes.data, hi.ctypes.data
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    hd, hp = h.ctypes.data_as(dp), hi.ctypes.data_as(ip)

    def host(p, nray, specs, n_profiles=None, power=hd):
        return lib.rays_hip_trace_profiles(C.byref(p), nray, hd, hd, power, len(specs) if n_profiles is None else n_profiles,
                                           records(specs), hp, hp, None, hd, hd, hd, None)
    who = "rays_hip_trace_profiles"
    hok = [(PSI, 10, H, None, H), (RHO, 12, None, None, H)]
    refused(host(axi, 1, hok, n_profiles=3), who + ": n_profiles = 3 is outside 1..2")
    refused(host(axi, -1, hok), who + ": nray < 0")
    refused(host(axi, 1, [hok[0], hok[0]]), who + ": the same profile twice")
    refused(host(axi, 1, [hok[0], (RHO, 12, None, H, H)]), who + ": profile_in is for the device form")
    refused(host(axi, 1, [(PSI, 10, None, H, H)]), who + ": profile_in is for the device form")
    refused(host(axi, 1, [hok[0], (RHO, 12, None, None, None)]), who + ": null array argument")
    refused(host(axi, 1, hok, power=None), who + ": null array argument")
    refused(host(slab, 1, [(X, 10, None, None, H), (RHO, 10, None, None, H)]), "unimplemented profile for this equilib_model")
    torch.cuda.synchronize()
    # nothing was written by any refused call
    assert (d.cpu().numpy() == -7.0).all() and (i.cpu().numpy() == -7).all() and (h == -7.0).all() and (hi == -7).all()
    # the Python layer
    from rays_amd.trace import DeviceTrace
    with pytest.raises(ValueError, match="does not exist for this equilib_model"):
        DeviceTrace(slab, gs["rvec0"], gs["rindex_vec0"], trajectories=False, deposition=[("Ptotal_x", 10), ("Ptotal_psi", 10)],
                    ray_power=np.ones(len(gs["rvec0"])))


# ---- 8. the Fortran driver ----------------------------------------------------------------------------------------------------------
def test_fortran_driver_reproduces_the_python_path(tmp_path):
    """tests/fortran/fused_profiles_driver.f90 + the binding, built with amdflang and linked against librays_hip.so:
    rays_hip_trace_profiles returns the Python path's bytes."""
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    libdir = os.path.join(ROOT, "rays_amd", "lib")
    hipdir = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    srcs = [os.path.join(ROOT, "fortran", "rays_hip_m.f90"), os.path.join(ROOT, "tests", "fortran", "fused_profiles_driver.f90")]
    exe = str(tmp_path / "fused_profiles_driver")
    subprocess.check_call([fc, "-O2", "-ffp-contract=off", "-w", "-o", exe] + srcs +
                          ["-L" + libdir, "-lrays_hip", "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + hipdir], cwd=str(tmp_path))
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_psi", 37), ("Ptotal_rho", 64)]
    nray, nv = len(r0), p.nv
    from rays_amd.params import axisym_tables_struct
    from tests import emul_build as eb
    from tests.test_cpu_fused_profiles import TABLE_FIELDS
    tab = eb.axisym_tables_of(g)
    t, keep = axisym_tables_struct(tab)
    rho = fl.rho_table(g)
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([nray, nv, specs[0][1], specs[1][1], hip.DEP_PROFILES[specs[0][0]], hip.DEP_PROFILES[specs[1][0]],
                          len(z["fspl_re"]), len(rho[0])], dtype=np.int32).tobytes())
        f.write(bytes(p))
        f.write(np.array([float(z["x_min"]), float(z["x_max"])]).tobytes())
        f.write(np.ascontiguousarray(z["fspl_re"], dtype=np.float64).tobytes())
        f.write(np.array([t.nr, t.nz, t.n_rb, t.n_ne, t.n_te, t.n_ti], dtype=np.int32).tobytes())
        for name in TABLE_FIELDS:
            a = np.ascontiguousarray(tab.get(name, ()), dtype=np.float64).ravel()
            f.write(np.array([a.size], dtype=np.int32).tobytes())
            f.write(a.tobytes())
        for a in (rho[0], rho[1], r0, n0, power):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8)
    want = hip.trace_profiles_host(p, r0, n0, power, specs, ngpu=1)
    want.update(work_a=want["works"][0], work_b=want["works"][1], profile_a=want["profiles"][0], profile_b=want["profiles"][1])
    off = 0
    for k, shape in [("npoints", (nray,)), ("stop_code", (nray,)), ("start_ray_vec", (nray, nv)), ("end_ray_vec", (nray, nv)),
                     ("end_residuals", (nray,)), ("max_residuals", (nray,)), ("work_a", (nray, specs[0][1])),
                     ("profile_a", (specs[0][1],)), ("work_b", (nray, specs[1][1])), ("profile_b", (specs[1][1],))]:
        integer = k in ("npoints", "stop_code")
        nbytes = int(np.prod(shape)) * (4 if integer else 8)
        got = raw[off:off + nbytes].view(np.int32 if integer else np.float64).reshape(shape)
        np.testing.assert_array_equal(got, want[k], err_msg="Fortran: " + k)
        off += nbytes
    assert off == raw.size
