"""GPU tier: deposition windows -- rays_hip_trace_window_profiles_device and the kernels it launches (EQ + 224 and
EQ + 480 in their names: the fused deposition kernels continued from a saved ray state), through
rays_amd.trace.WindowedDeposition.  Everything is compared on bit patterns: with the reference post-processor's work /
profile / Q_sum in the golden files, with one rays_hip_trace_profiles_device call on the same rays (pinned by
tests/test_gpu_fused_profiles.py), and with rays_hip_deposition_device on a recorded trace.  No tolerance appears."""
import ctypes as C
import itertools
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
from tests.test_gpu_fused_deposition import _distinct_powers, _load, _resident_lanes, _tiled
from tests.test_gpu_fused_profiles import _profiles

pytestmark = pytest.mark.gpu
STATE = ("v", "s", "nstep", "stop_code", "resid", "sg_err", "flags")


def _state_bytes(wd):
    return b"".join(np.ascontiguousarray(getattr(wd.state, k).cpu().numpy()).tobytes() for k in STATE)


def _work_bytes(wd):
    return b"".join(w.cpu().numpy().tobytes() for w in wd.works)


def _windowed(p, r0, n0, power, specs, sizes, profile_in=None, after_window=None, extra=1):
    """A whole run in deposition windows through WindowedDeposition: the sizes cycled until every ray has ended, the
    profiles summed in the last window only; `extra` more calls, which must change no byte.  Out as _profiles()."""
    import torch
    from rays_amd.trace import WindowedDeposition
    wd = WindowedDeposition(p, r0, n0, deposition=list(specs), ray_power=power, profile_in=profile_in)
    for w in wd.works:
        w.fill_(float("nan"))   # launch() zeroes the accumulators
    for q in wd.profiles:
        q.fill_(float("nan"))
    wd.launch()
    have = np.ones(len(r0), dtype=np.int64)
    windows = 0
    for k, n in enumerate(itertools.cycle(sizes)):
        assert k < 100000
        if wd.state.under_way == 0:
            break
        npw = wd.advance(n, profiles=False).cpu().numpy()
        assert (npw >= 0).all() and (npw <= n).all()
        have += npw
        windows += 1
        if after_window:
            after_window(k, wd)
    assert all(np.isnan(q.cpu().numpy()).all() for q in wd.profiles)   # profiles=False: no sum was run
    before = _state_bytes(wd) + _work_bytes(wd)
    for _ in range(extra):
        assert not wd.advance(5, profiles=True).cpu().numpy().any()
        assert _state_bytes(wd) + _work_bytes(wd) == before
    res = wd.results()
    out = {k: getattr(res[0].summaries, k) for k in sl.KEYS}
    assert np.array_equal(have, out["npoints"])
    out["works"] = [r.work for r in res]
    out["profiles"] = [r.profile for r in res]
    out["windows"] = windows
    del wd
    torch.cuda.empty_cache()
    return out


def _plus(name, offset):
    head, rest = name.split("<", 1)
    eq, tail = rest.split(",", 1)
    return f"{head}<{int(eq) + offset},{tail}"


# ---- 1. fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1], [7, 1, 13]], ids=["one_step", "7_1_13"])
@pytest.mark.parametrize("name", fl.DEP_FIXTURES)
def test_fixture_deposition_in_windows_equals_golden(name, sizes):
    """The twelve fixtures with the reference post-processor's results, every profile each carries, in one-step windows
    and in windows of 7, 1, 13: work, profile, Q_sum and the summaries, bit for bit; the kernel is the fused one with
    the continuation bit (EQ + 128)."""
    g, nml, p = _load(name)
    r0, n0 = g["rvec0_full"], g["rindex_vec0_full"]
    assert hip.window_profiles_kernel_name(p, len(r0), 1) == _plus(hip.deposition_kernel_name(p, len(r0)), 128)
    for i, which in enumerate(fl.profile_names(g)):
        out = _windowed(p, r0, n0, g["dep_power"], [(which, int(g["dep_n_bins"]))], sizes)
        fl.assert_golden_deposition(out["works"][0], out["profiles"][0], g, i, f"{name} {which}")
        fl.assert_golden_summaries(out, g, f"{name} {which}")
        assert out["profiles"][0].sum() > 0


@pytest.mark.parametrize("sizes", [[1], [7, 1, 13]], ids=["one_step", "7_1_13"])
@pytest.mark.parametrize("order", pl.ORDERS, ids=["psi_rho", "rho_psi"])
@pytest.mark.parametrize("name", pl.TWO_PROFILE_FIXTURES)
def test_fixture_profiles_in_windows_equal_golden(name, order, sizes):
    """The six fixtures with both profiles, both from one windowed run, in both request orders; the kernel is the
    fused one + 384."""
    g, nml, p = _load(name)
    r0, n0 = g["rvec0_full"], g["rindex_vec0_full"]
    assert hip.window_profiles_kernel_name(p, len(r0), 2) == _plus(hip.deposition_kernel_name(p, len(r0)), 384)
    names, nb = fl.profile_names(g), int(g["dep_n_bins"])
    out = _windowed(p, r0, n0, g["dep_power"], [(w, nb) for w in order], sizes)
    for k, w in enumerate(order):
        fl.assert_golden_deposition(out["works"][k], out["profiles"][k], g, names.index(w), f"{name} {w}")
    fl.assert_golden_summaries(out, g, name)


# ---- 2. refill -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["rk4", "sg"])
def test_refilled_lanes_in_windows_equal_one_fused_call(solver):
    """The 64 rays of the eqdsk + damping fixture tiled to resident lanes + 4500 rays (RK4: nstep_max = 40; SG:
    nstep_max = 10), every ray with a power of its own, one ray outside the box and one refused at its initial check,
    in windows of 7, 1, 13: a lane that takes over a ray re-establishes that ray's x_prev / q_prev.  Works, profiles
    and summaries equal ONE rays_hip_trace_profiles_device call."""
    g, nml, p0 = _load("gold_axisym64_eqdsk_damp_rk4" if solver == "rk4" else "gold_axisym64_eqdsk_damp_sg")
    p = copy_params(p0)
    p.nstep_max = 40 if solver == "rk4" else 10
    nray = _resident_lanes() + 4500
    r0, n0 = _tiled(g["rvec0_full"], g["rindex_vec0_full"], nray)
    r0[7, 0] = 10.0      # outside the box
    n0[11] *= 3.0        # stops at the initial check_save
    power = _distinct_powers(nray)
    want = ("rk4_trace_kernel" if solver == "rk4" else "sg_trace_kernel") + "<486, 2, 0, 8>"
    assert hip.window_profiles_kernel_name(p, nray, 2) == want
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 100)]
    ref = _profiles(p, r0, n0, power, specs)
    out = _windowed(p, r0, n0, power, specs, [7, 1, 13])
    assert out["npoints"][7] == 1 and out["npoints"][11] == 1 and out["npoints"].max() == p.nstep_max + 1
    assert out["windows"] >= 3
    sl.assert_same(out, ref, solver)
    for k in range(2):
        assert out["works"][k].any() and not out["works"][k][7].any() and not out["works"][k][11].any()
        np.testing.assert_array_equal(out["works"][k], ref["works"][k], err_msg=f"{solver}: work {k}")
        np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][k], err_msg=f"{solver}: profile {k}")


# ---- 3. the prefix contract -----------------------------------------------------------------------------------------------
def test_every_prefix_equals_the_deposition_of_the_clipped_trace():
    """After every window each work equals rays_hip_deposition_device on a recorded trace of the same rays with npoints
    clipped to state.nstep + 1."""
    import torch
    from rays_amd.trace import DeviceTrace
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_psi", 100), ("Ptotal_rho", 33)]
    tr = DeviceTrace(p, r0, n0)
    tr.launch()
    nray = tr.nray
    d_pw = torch.as_tensor(np.ascontiguousarray(power, dtype=np.float64)).cuda()
    full = tr.npoints.clone()
    seen = []

    def check(k, wd):
        clipped = torch.minimum(wd.state.nstep + 1, full).to(torch.int32).contiguous()
        assert torch.equal(clipped, wd.state.nstep + 1)
        for (w, nb), work in zip(specs, wd.works):
            ref = torch.full((nb, nray), float("nan"), dtype=torch.float64, device="cuda")
            prof = torch.zeros(nb, dtype=torch.float64, device="cuda")
            hip.deposition_device(p, w, nb, nray, tr.ray_vec.data_ptr(), clipped.data_ptr(), d_pw.data_ptr(),
                                  ref.data_ptr(), None, prof.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(work.cpu().numpy(), ref.cpu().numpy(), err_msg=f"{w} after window {k}")
        seen.append(int(clipped.sum().item()))

    out = _windowed(p, r0, n0, power, specs, [7, 1, 13], after_window=check)
    assert len(seen) >= 4 and seen == sorted(seen) and seen[0] < seen[-1]
    fl.assert_golden_deposition(out["works"][0], out["profiles"][0], g, 0, "after the last window")   # (100 bins)


# ---- 4. checkpoint ----------------------------------------------------------------------------------------------------------
def test_checkpoint_and_resume_equal_the_uninterrupted_run(tmp_path):
    """save() after three windows, load() into a fresh object, continue: every byte of the state, the works and the
    profiles equals the uninterrupted run's."""
    from rays_amd.trace import WindowedDeposition
    g, nml, p = _load("gold_axisym64_eqdsk_damp_sg")
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_rho", 50), ("Ptotal_psi", 100)]
    sizes = [7, 1, 13, 7, 1, 13, 1000]

    whole = WindowedDeposition(p, r0, n0, deposition=specs, ray_power=power)
    whole.launch()
    for n in sizes:
        whole.advance(n)
    assert whole.state.under_way == 0

    first = WindowedDeposition(p, r0, n0, deposition=specs, ray_power=power)
    first.launch()
    for n in sizes[:3]:
        first.advance(n, profiles=False)
    assert 0 < first.state.under_way
    path = str(tmp_path / "checkpoint.npz")
    first.save(path)
    del first
    second = WindowedDeposition.load(path, p, r0, n0)
    for n in sizes[3:]:
        second.advance(n)
    assert _state_bytes(second) == _state_bytes(whole) and _work_bytes(second) == _work_bytes(whole)
    a, b = whole.results(), second.results()
    for k in range(2):
        assert a[k].profile.tobytes() == b[k].profile.tobytes() and a[k].work.tobytes() == b[k].work.tobytes()
    fl.assert_golden_deposition(b[1].work, b[1].profile, g, fl.profile_names(g).index("Ptotal_psi"), "resumed")   # (100 bins)
    for key in sl.KEYS:
        np.testing.assert_array_equal(getattr(a[0].summaries, key), getattr(b[0].summaries, key), err_msg=key)


# ---- 5. stream and tail -------------------------------------------------------------------------------------------------------
def test_windows_queued_on_a_stream_and_blocks_chained_through_profile_in():
    """Windows queued on a non-default stream with no host synchronisation between them, profile = NULL in all but the
    last; two ray blocks chained through profile_in equal one call; calls after the end change nothing."""
    import torch
    from rays_amd.trace import WindowedDeposition
    g, nml, p = _load("gold_axisym64_eqdsk_damp_rk4")
    r0, n0, power, nb = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], int(g["dep_n_bins"])
    specs = [("Ptotal_psi", nb), ("Ptotal_rho", 33)]
    whole = _profiles(p, r0, n0, power, specs)
    sizes = [7, 1, 13] * 40   # more than the longest ray needs: the tail of the queue runs on ended rays
    assert sum(sizes) > int(g["npoints_full"].max())
    h = 29
    stream = torch.cuda.Stream()
    carry = None
    works = []
    for lo, hi in ((0, h), (h, len(r0))):
        with torch.cuda.stream(stream):
            wd = WindowedDeposition(p, r0[lo:hi], n0[lo:hi], deposition=specs, ray_power=power[lo:hi], profile_in=carry)
            wd.launch()
            for n in sizes[:-1]:
                wd.advance(n, profiles=False)
            npw = wd.advance(sizes[-1], profiles=True)
        stream.synchronize()
        assert wd.state.under_way == 0 and not npw.cpu().numpy().any()
        carry = [q.clone() for q in wd.profiles]
        works.append([w.cpu().numpy().T for w in wd.works])
    for k in range(2):
        np.testing.assert_array_equal(carry[k].cpu().numpy(), whole["profiles"][k])
        np.testing.assert_array_equal(np.concatenate([works[0][k], works[1][k]]), whole["works"][k])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_and_the_numerics_setting():
    import torch
    from rays_amd.trace import RayState
    lib = hip.load()
    d = torch.full((4096,), -7.0, dtype=torch.float64, device="cuda")
    i = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    D, I = d.data_ptr(), i.data_ptr()
    g, nml, axi = _load("gold_axisym64_eqdsk_damp_rk4")
    st = RayState(4, axi.nv, device="cuda")
    poison = b"".join(getattr(st, k).fill_(-7).cpu().numpy().tobytes() for k in STATE)

    def records(specs):
        arr = (hip.DepProfileStruct * max(len(specs), 1))()
        for r, s in zip(arr, specs):
            r.which, r.n_bins, r.work, r.profile_in, r.profile = s
        return arr

    def dev(p, nray, specs, n_profiles=None, state=st, n_steps=5, power=D, npw=I):
        s = None if state is None else C.byref(hip._state_struct(state))
        return lib.rays_hip_trace_window_profiles_device(C.byref(p), nray, s, n_steps, power,
                                                         len(specs) if n_profiles is None else n_profiles, records(specs),
                                                         npw, None)

    def refused(rc, text):
        assert rc != 0 and text in hip.last_error(), hip.last_error()

    PSI, RHO, X = (hip.DEP_PROFILES[k] for k in ("Ptotal_psi", "Ptotal_rho", "Ptotal_x"))
    who = "rays_hip_trace_window_profiles_device"
    ok = [(PSI, 10, D, None, D), (RHO, 12, D, None, None)]
    # what rays_hip_trace_profiles_device refuses, per record
    refused(dev(axi, 1, ok, n_profiles=0), who + ": n_profiles = 0 is outside 1..2")
    refused(dev(axi, 1, ok, n_profiles=3), who + ": n_profiles = 3 is outside 1..2")
    refused(dev(axi, -1, ok), who + ": nray < 0")
    refused(dev(axi, 1, [ok[0], ok[0]]), who + ": the same profile twice")
    for nb in (0, -3, 321):
        refused(dev(axi, 1, [ok[0], (RHO, nb, D, None, D)]), f"{who}: n_bins = {nb} is outside 1..320")
    refused(dev(axi, 1, [ok[0], (X, 10, D, None, D)]), "unimplemented profile for this equilib_model")
    refused(dev(axi, 1, [ok[0], (RHO, 12, None, None, D)]), who + ": null work")
    refused(dev(axi, 1, [(PSI, 10, None, None, None)]), who + ": null work")
    gs, nmls, slab = _load("gold_slab16_damp_rk4")
    sts = RayState(4, slab.nv, device="cuda")
    refused(dev(slab, 1, [(X, 10, D, None, D), (PSI, 10, D, None, D)], state=sts), "unimplemented profile for this equilib_model")
    g2, nml2, solmag = _load("gold_axisym64_solmag_damp_rk4")
    refused(dev(solmag, 1, ok), "rho is only implemented for eqdsk_magnetics_spline_interp")
    g3, nml3, nodamp = load_golden("cfg1_slab16_rk4")
    refused(dev(nodamp, 1, [(X, 10, D, None, D)]), who + ": needs a run with damping")
    g4, nml4, sol = load_golden("gold_solovev64_damp_rk4")
    refused(dev(sol, 1, ok), "initialize_deposition_profiles: unimplemented equilib_model")
    # what rays_hip_trace_window_device refuses
    refused(dev(axi, 1, ok, n_steps=0), who + ": n_steps < 1")
    refused(dev(axi, 1, ok, npw=None), who + ": null device pointer")
    refused(dev(axi, 1, ok, state=None), who + ": null pointer in the ray state")
    half = RayState(4, axi.nv, device="cuda")
    half.resid = None
    refused(dev(axi, 1, ok, state=half), who + ": null pointer in the ray state")
    refused(dev(axi, 4, ok, n_steps=2 ** 30), who + ": nray * n_steps exceeds 2^31 - 1")
    g5, nml5, sg = _load("gold_axisym64_eqdsk_damp_sg")
    nosg = RayState(4, sg.nv, device="cuda")
    nosg.sg_err = None
    refused(dev(sg, 1, ok, state=nosg), who + ": SG_ODE needs the ray state's sg_err")
    # its own
    refused(dev(axi, 1, ok, power=None), who + ": null initial_ray_power")
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -7.0).all() and (i.cpu().numpy() == -7).all()
    assert b"".join(getattr(st, k).cpu().numpy().tobytes() for k in STATE) == poison
    assert hip.window_profiles_kernel_name(slab, 16, 2) == "" and hip.window_profiles_kernel_name(sol, 16, 1) == ""
    # rays_hip_set_numerics(tolerance) changes nothing: the same kernels, the same bytes
    g, nml, axi = _load("gold_axisym64_eqdsk_damp_rk4")   # (its rho table again: the fixtures above set theirs)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    prev = hip.get_numerics()
    hip.set_numerics("tolerance")
    try:
        assert hip.window_profiles_kernel_name(axi, len(r0), 1) == "rk4_trace_kernel<230, 2, 0, 8>"
        assert hip.window_profiles_kernel_name(axi, len(r0), 2) == "rk4_trace_kernel<486, 2, 0, 8>"
        out = _windowed(axi, r0, n0, power, [("Ptotal_psi", 100), ("Ptotal_rho", 100)], [7, 1, 13])
        for k in range(2):
            fl.assert_golden_deposition(out["works"][k], out["profiles"][k], g, k, "tolerance setting")
    finally:
        hip.set_numerics(prev)
    # the Python layer keeps its refusal
    from rays_amd.trace import DeviceTrace
    with pytest.raises(ValueError, match="window=... does not go with deposition"):
        DeviceTrace(axi, r0, n0, trajectories=False, deposition=[("Ptotal_psi", 5)], ray_power=power, window=4)


# ---- 7. the Fortran driver ----------------------------------------------------------------------------------------------------------
def test_fortran_driver_reproduces_the_fused_pass(tmp_path):
    """tests/fortran/window_profiles_driver.f90 + the binding, built with amdflang and linked against librays_hip.so:
    state_init, deposition windows of 7, 1, 13 and the state summary through the Fortran interfaces return the bytes of
    one rays_hip_trace_profiles_device call."""
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    libdir = os.path.join(ROOT, "rays_amd", "lib")
    hipdir = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    srcs = [os.path.join(ROOT, "fortran", "rays_hip_m.f90"), os.path.join(ROOT, "tests", "fortran", "window_profiles_driver.f90")]
    exe = str(tmp_path / "window_profiles_driver")
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
    want = _profiles(p, r0, n0, power, specs)
    want.update(work_a=want["works"][0].T, work_b=want["works"][1].T, profile_a=want["profiles"][0],
                profile_b=want["profiles"][1])
    off = 0
    for k, shape in [("npoints", (nray,)), ("stop_code", (nray,)), ("start_ray_vec", (nray, nv)), ("end_ray_vec", (nray, nv)),
                     ("end_residuals", (nray,)), ("max_residuals", (nray,)), ("work_a", (specs[0][1], nray)),
                     ("profile_a", (specs[0][1],)), ("work_b", (specs[1][1], nray)), ("profile_b", (specs[1][1],))]:
        integer = k in ("npoints", "stop_code")
        nbytes = int(np.prod(shape)) * (4 if integer else 8)
        got = raw[off:off + nbytes].view(np.int32 if integer else np.float64).reshape(shape)
        np.testing.assert_array_equal(got, want[k], err_msg="Fortran: " + k)
        off += nbytes
    windows = int(raw[off:off + 4].view(np.int32)[0])
    assert off + 4 == raw.size and windows >= 3
