"""GPU tier: windowed tracing -- rays_hip_state_init_device / rays_hip_trace_window_device / rays_hip_state_summary_device /
rays_hip_trace_windowed and the kernels they launch (EQ + 128 in their names, EQ + 160 for summary windows).  Everything
is compared on bit patterns with the one-shot trace: the golden files, or rays_hip_trace_device / rays_hip_trace on the
same inputs in the same process -- never with the windowed path itself."""
import os

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.namelist import read_namelist
from rays_amd.params import copy_params, params_from_namelist
from rays_amd.ray_init import fan_from_namelist
from tests import summary_lib as sl
from tests.common import GOLDEN_CASES, ROOT, load_golden, stop_codes

pytestmark = pytest.mark.gpu
SUMMARY_KEYS = ("npoints", "stop_code", "end_ray_vec", "end_residuals", "max_residuals")
STATE_BYTES_PER_RAY = lambda nv: 8 * (nv + 1 + 3 + 2) + 3 * 4   # v, s, resid[3], sg_err[2]; nstep, stop_code, flags


def _fan(cfg, overrides, tables=None, nray=None):
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


def _resident_lanes():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


def _windowed(p, r0, n0, n_steps, policy="record", max_windows=10000):
    """A whole trace in windows through DeviceTrace(window=...), assembled on the device: the full arrays (nan where no
    recording window covered a point) and the state's summaries, as numpy arrays; plus the number of windows."""
    import torch
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0, window=n_steps, trajectories=policy != "summary")
    n, nv, npt = len(r0), p.nv, p.nstep_max + 1
    dev = tr.device
    full_v = torch.full((n, npt, nv), float("nan"), dtype=torch.float64, device=dev)
    full_r = torch.full((n, npt), float("nan"), dtype=torch.float64, device=dev)
    tr.launch()
    full_v[:, 0], full_r[:, 0] = tr.start_ray_vec, 0.0
    have = torch.ones(n, dtype=torch.int64, device=dev)
    col = torch.arange(n_steps, device=dev)[None, :]
    rows = torch.arange(n, device=dev)[:, None].expand(n, n_steps)
    windows = 0
    while tr.state.under_way:
        assert windows < max_windows
        rec = policy == "record" or (policy == "mixed" and windows % 2 == 0)
        rv, res, npw = tr.advance(recording=rec)
        npw = npw.to(torch.int64)
        assert int(npw.min()) >= 0 and int(npw.max()) <= n_steps
        if rec:
            live = col < npw[:, None]
            at = (have[:, None] + col)[live]
            full_v[rows[live], at] = rv[live]
            full_r[rows[live], at] = res[live]
        have += npw
        windows += 1
    s = tr.results()
    out = {k: getattr(s, k) for k in SUMMARY_KEYS}
    assert np.array_equal(have.cpu().numpy(), out["npoints"])
    out.update(ray_vec=full_v.cpu().numpy(), residual=full_r.cpu().numpy(), start_ray_vec=s.start_ray_vec, windows=windows,
               trace=tr)
    return out


def _one_shot(p, r0, n0):
    """rays_hip_trace_device on the same inputs, as numpy arrays."""
    import torch
    from rays_amd.trace import DeviceTrace
    tr = DeviceTrace(p, r0, n0)
    tr.launch()
    torch.cuda.synchronize()
    out = {k: getattr(tr, k).cpu().numpy() for k in SUMMARY_KEYS + ("ray_vec", "residual")}
    del tr
    torch.cuda.empty_cache()
    return out


def _assert_same(out, ref, what, covered_only=False):
    for k in SUMMARY_KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"{what}: {k}")
    npt = out["ray_vec"].shape[1]
    live = np.arange(npt)[None, :] < np.asarray(ref["npoints"])[:, None]
    got = ~np.isnan(out["residual"])
    if covered_only:
        assert not (got & ~live).any(), what
        live = live & got
    else:
        np.testing.assert_array_equal(got, live, err_msg=f"{what}: the points written")
    np.testing.assert_array_equal(out["ray_vec"][live], np.asarray(ref["ray_vec"])[live], err_msg=f"{what}: ray_vec")
    np.testing.assert_array_equal(out["residual"][live], np.asarray(ref["residual"])[live], err_msg=f"{what}: residual")


def _golden_ref(g, p):
    """A fixture's arrays padded to nstep_max + 1 points, with the golden summaries."""
    ref = sl.golden_summaries(g)
    n, keep = g["ray_vec"].shape[0], g["ray_vec"].shape[1]
    rv, res = np.zeros((n, p.nstep_max + 1, p.nv)), np.zeros((n, p.nstep_max + 1))
    rv[:, :keep], res[:, :keep] = g["ray_vec"], g["residual"]
    ref.update(ray_vec=rv, residual=res)
    return ref


# ---- 1. fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_fixtures_in_windows_equal_golden(name):
    """All 38 fixtures, window sizes 8 and 50, recording and summary-only, against the golden files; the kernel is the
    recording kernel of the shape (the one-ray-per-lane one) with the continuation bit in its EQ argument."""
    g, nml, p = load_golden(name)
    n = len(g["rvec0"])
    prev = os.environ.get("RAYS_HIP_SG_GROUP")
    os.environ["RAYS_HIP_SG_GROUP"] = "0"   # (name the one-ray-per-lane kernel where a lane-group kernel is the default)
    try:
        head, rest = hip.kernel_name(p, n).split("<", 1)
    finally:
        if prev is None:
            del os.environ["RAYS_HIP_SG_GROUP"]
        else:
            os.environ["RAYS_HIP_SG_GROUP"] = prev
    eq, tail = rest.split(",", 1)
    assert hip.window_kernel_name(p, n) == f"{head}<{int(eq) + 128},{tail}"
    assert hip.window_kernel_name(p, n, recording=False) == f"{head}<{int(eq) + 160},{tail}"
    ref = _golden_ref(g, p)
    for w in (8, 50):
        out = _windowed(p, g["rvec0"], g["rindex_vec0"], w)
        np.testing.assert_array_equal(out["stop_code"], stop_codes(g["stop_flag"]))
        np.testing.assert_array_equal(out["start_ray_vec"], ref["start_ray_vec"])
        _assert_same(out, ref, f"{name}, n_steps {w}")
        s = _windowed(p, g["rvec0"], g["rindex_vec0"], w, "summary")
        for k in SUMMARY_KEYS:
            np.testing.assert_array_equal(s[k], ref[k], err_msg=f"{name}, n_steps {w}, summary windows: {k}")


# ---- 2. the one-wave RK4 kernel with several rays per lane -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["slab", "solovev"])
def test_rk4_refill_and_long_first_order(which):
    """70 000 rays, just above one wave per SIMD on 256 CUs, nstep_max = 40, n_steps = 16: three windows, lanes refilled,
    rays handed out long-first; against rays_hip_trace_device in the same process.  Recording and summary windows
    mixed give the same summaries and the matching slices."""
    if which == "slab":
        p, r0, n0 = _fan("cfg4_slab1M_rk4.in", {
            "simple_slab_ray_init_list": dict(n_ky_launch=265, n_kz_launch=265, delta_rindex_y0=0.2 / 265,
                                              delta_rindex_z0=0.2 / 265),
            "ode_list": dict(nstep_max=40)}, nray=70000)
        want = "rk4_trace_kernel<164, 2, 0, 7>"
    else:
        p, r0, n0 = _fan("cfg3b_solovev64k_rk4.in", {
            "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=265, n_rindex_phi=265,
                                                      delta_rindex_theta=0.31 / 265, delta_rindex_phi=0.3875 / 265),
            "ray_init_list": dict(nray_max=265 * 265), "ode_list": dict(nstep_max=40)}, nray=70000)
        want = "rk4_trace_kernel<165, 2, 0, 7>"
    assert len(r0) == 70000 > _resident_lanes()
    assert hip.window_kernel_name(p, len(r0), recording=False) == want
    ref = _one_shot(p, r0, n0)
    assert ref["npoints"].max() == 41
    out = _windowed(p, r0, n0, 16)
    assert out["windows"] == 3
    _assert_same(out, ref, which)
    _assert_same(_windowed(p, r0, n0, 16, "mixed"), ref, which + ", mixed windows", covered_only=True)


def test_large_fan_takes_the_one_wave_kernel():
    """A 132 000-ray Solovev fan, nstep_max = 40: the one-shot trace dispatches the _w2 build, the windows the one-wave
    kernel with the continuation bit -- bit-identical."""
    p, r0, n0 = _fan("cfg3b_solovev64k_rk4.in", {
        "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=364, n_rindex_phi=364,
                                                  delta_rindex_theta=0.31 / 364, delta_rindex_phi=0.3875 / 364),
        "ray_init_list": dict(nray_max=364 * 364), "ode_list": dict(nstep_max=40)}, nray=132000)
    assert hip.kernel_name(p, len(r0)) == "rk4_trace_kernel_w2<5, 2, 0, 7>"
    assert hip.window_kernel_name(p, len(r0)) == "rk4_trace_kernel<133, 2, 0, 7>"
    _assert_same(_windowed(p, r0, n0, 16), _one_shot(p, r0, n0), "132 000 rays")


# ---- 3. SG refill ---------------------------------------------------------------------------------------------------------------
def test_sg_refill():
    """sg_trace_kernel's continuation variant with more rays than resident lanes (one 256-lane block per CU),
    nstep_max = 10, n_steps = 8, against the one-shot trace."""
    g, nml, p0 = load_golden("gold_solovev64_sg_cold")
    p = copy_params(p0)
    nray = _resident_lanes() + 4500
    reps = nray // len(g["rvec0_full"]) + 1
    r0 = np.tile(g["rvec0_full"], (reps, 1))[:nray].copy()
    n0 = np.tile(g["rindex_vec0_full"], (reps, 1))[:nray].copy()
    p.nstep_max = 10
    r0[7, 0] = 10.0      # outside the box
    n0[11] *= 3.0        # stops at the initial check_save
    assert hip.window_kernel_name(p, nray) == "sg_trace_kernel<133, 2, 0, 7>"
    ref = _one_shot(p, r0, n0)
    assert ref["npoints"][7] == 1 and ref["npoints"][11] == 1 and ref["npoints"].max() > 9
    out = _windowed(p, r0, n0, 8)
    assert out["windows"] == 2
    _assert_same(out, ref, "sg refill")


# ---- 4. cfg 5b's shape ---------------------------------------------------------------------------------------------------------
def test_cfg5b_shape():
    """nv = 8 with the eqdsk tables staged in LDS and the Z-function table: every 64th ray of cfg 5b's fan (4096 rays),
    n_steps = 25."""
    from rays_amd.trace import RaysRun
    run = RaysRun.from_namelist(os.path.join(ROOT, "configs", "cfg5b_axisym256k_rk4_damp.in"))
    p, r0, n0 = run.params, run.rvec0[::64].copy(), run.rindex_vec0[::64].copy()
    assert len(r0) == 4096 and p.nv == 8
    assert hip.window_kernel_name(p, len(r0)) == "rk4_trace_kernel<134, 2, 0, 8>"
    ref = _one_shot(p, r0, n0)
    out = _windowed(p, r0, n0, 25)
    assert out["windows"] > 3
    _assert_same(out, ref, "cfg 5b shape")


# ---- 5. memory -------------------------------------------------------------------------------------------------------------------
def test_memory_is_bounded_by_state_and_window():
    """The 70 000-ray slab fan with nstep_max = 1000 and n_steps = 16: torch.cuda memory in use grows over the windows by
    no more than nray * (16 * (nv + 1) * 8 + state bytes per ray) plus the blocks the Python holder documents beside
    them, none of which scales with n_steps or nstep_max -- inputs (48 B per ray), npoints_win and start_ray_vec
    (4 + 8 nv), the five summary arrays (8 (nv + 2) + 8) -- and what torch's caching allocator may add to each of the
    18 tensors: a request is cut from a segment of whole 2 MiB, and a remainder below 1 MiB is not split off but counted
    with it.  The count follows from the shapes and that rule alone (first run: 93 157 888 B in use against 92 960 000 B
    of tensors); the one-shot trajectories would be 64 KB per ray, 4.5 GB."""
    import torch
    from rays_amd.trace import DeviceTrace
    p, r0, n0 = _fan("cfg4_slab1M_rk4.in", {
        "simple_slab_ray_init_list": dict(n_ky_launch=265, n_kz_launch=265, delta_rindex_y0=0.2 / 265,
                                          delta_rindex_z0=0.2 / 265),
        "ode_list": dict(nstep_max=1000)}, nray=70000)
    n, nv, w = len(r0), p.nv, 16
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    tr = DeviceTrace(p, r0, n0, window=w)
    tr.launch()
    peak = torch.cuda.memory_allocated()
    for _ in range(4):
        tr.advance()
        peak = max(peak, torch.cuda.memory_allocated())
    torch.cuda.synchronize()
    grown = peak - before
    bound = n * (w * (nv + 1) * 8 + STATE_BYTES_PER_RAY(nv)) + n * (48 + 4 + 8 * nv + 8 * (nv + 2) + 8) + 18 * (1 << 20)
    print(f"torch.cuda memory in use grew by {grown} bytes = {grown / n:.1f} B per ray (bound {bound / n:.1f})")
    assert grown <= bound
    assert int(tr.state.nstep.max().item()) == 4 * w
    del tr
    torch.cuda.empty_cache()


# ---- 6. the host form and the Python host ----------------------------------------------------------------------------------------
def test_host_form_equals_rays_hip_trace():
    """rays_hip_trace_windowed against rays_hip_trace on a fixture (1001 rays of cfg 2's fan, n_steps = 50 and 7) and on
    the 70 000-ray Solovev fan; RaysRun.trace_rays(window=...) equals trace_rays()."""
    from rays_amd.trace import RayResults, RaysRun
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][:1001], g["rindex_vec0_full"][:1001]
    ref = hip.trace_host(p, r0, n0, ngpu=1)
    for w in (50, 7):
        out = hip.trace_windowed_host(p, r0, n0, w, ngpu=1)
        for k in SUMMARY_KEYS + ("ray_vec", "residual"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg=f"n_steps {w}: {k}")
    run = RaysRun(p, r0, n0)
    a, b = run.trace_rays(ngpu=1, window=64), run.trace_rays(ngpu=1)
    assert isinstance(a, RayResults)
    for k in SUMMARY_KEYS + ("ray_vec", "residual"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    p, r0, n0 = _fan("cfg3b_solovev64k_rk4.in", {
        "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=265, n_rindex_phi=265,
                                                  delta_rindex_theta=0.31 / 265, delta_rindex_phi=0.3875 / 265),
        "ray_init_list": dict(nray_max=265 * 265), "ode_list": dict(nstep_max=40)}, nray=70000)
    ref = hip.trace_host(p, r0, n0, ngpu=1)
    out = hip.trace_windowed_host(p, r0, n0, 16, ngpu=1)
    for k in SUMMARY_KEYS + ("ray_vec", "residual"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"70 000 rays: {k}")


def test_refusals_and_numerics_setting():
    """The refusals of the device entry by their messages, and rays_hip_set_numerics(tolerance) changes nothing."""
    import torch
    from rays_amd.trace import DeviceTrace
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0"], g["rindex_vec0"]
    tr = DeviceTrace(p, r0, n0, window=8)
    tr.launch()
    with pytest.raises(hip.RaysHipError, match="n_steps < 1"):
        tr.advance(0)
    with pytest.raises(hip.RaysHipError, match="given together or not at all"):
        hip.trace_window_device(p, tr.nray, tr.state, 8, tr.ray_vec.data_ptr(), 0, tr.npoints_win.data_ptr())
    with pytest.raises(hip.RaysHipError, match="null device pointer"):
        hip.trace_window_device(p, tr.nray, tr.state, 8, 0, 0, 0)
    keep = tr.state.resid
    tr.state.resid = None
    with pytest.raises(hip.RaysHipError, match="null pointer in the ray state"):
        tr.advance()
    tr.state.resid = keep
    q = copy_params(load_golden("gold_solovev64_sg_cold")[2])
    sg = DeviceTrace(q, r0, n0, window=8)
    sg.state.sg_err = None
    with pytest.raises(hip.RaysHipError, match="SG_ODE needs the ray state's sg_err"):
        sg.launch()
    torch.cuda.synchronize()
    prev = hip.set_numerics("tolerance")
    try:
        assert hip.window_kernel_name(p, len(r0)) == "rk4_trace_kernel<133, 2, 0, 7>"
        _assert_same(_windowed(p, r0, n0, 50), _golden_ref(g, p), "tolerance setting")
    finally:
        hip.set_numerics(prev)
