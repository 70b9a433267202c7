"""GPU tier: segmented deposition above the kernel -- the fused ds scan (rays_hip_scan_profiles_device through
RayScan(deposition=...)) and one profile per beam (rays_hip_trace_profiles_segments_device through
DeviceTrace(segments=...)).  Runs at a fixture's own ds are compared with the reference post-processor's work / profile /
Q_sum in the golden files, every other run with rays_hip_trace_profiles_device (pinned by tests/test_gpu_fused_profiles.py)
called on that run alone with ds replaced.  Every comparison is on bit patterns; no tolerance appears."""
import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import fused_deposition_lib as fl
from tests import summary_lib as sl
from tests.test_gpu_fused_deposition import _distinct_powers, _load, _resident_lanes, _tiled
from tests.test_gpu_fused_profiles import _profiles

pytestmark = pytest.mark.gpu

RK4, SG, SLAB = "gold_axisym64_eqdsk_damp_rk4", "gold_axisym64_eqdsk_damp_sg", "gold_slab16_damp_rk4"


def _ds_values(p):
    return [float(p.ds), 0.5 * float(p.ds), float(p.ds)]


def _scan(p, r0, n0, power, specs, ds_values, profile_in=None):
    """RayScan(deposition=[...]): per run the dictionary _profiles gives for one call"""
    import torch
    from rays_amd.scan import RayScan
    sc = RayScan(p, r0, n0, ds_values, trajectories=False, deposition=list(specs), ray_power=power, profile_in=profile_in)
    assert sc.ray_vec is None and sc.residual is None
    for w in sc.works:
        w.fill_(float("nan"))   # the call zeroes every work itself
    sc.launch()
    runs = []
    for recs in sc.results():
        assert all(r.summaries is recs[0].summaries for r in recs) and [r.profile_name for r in recs] == [w for w, _ in specs]
        out = {k: getattr(recs[0].summaries, k) for k in sl.KEYS}
        out["works"] = [r.work for r in recs]
        out["profiles"] = [r.profile for r in recs]
        runs.append(out)
    del sc
    torch.cuda.empty_cache()
    return runs


def _run_alone(p, ds, r0, n0, power, specs, profile_in=None):
    q = copy_params(p)
    q.ds = ds
    return _profiles(q, r0, n0, power, specs, profile_in=profile_in)


def _assert_same_run(out, ref, what):
    sl.assert_same(out, ref, what)
    for k in range(len(ref["works"])):
        np.testing.assert_array_equal(out["works"][k], ref["works"][k], err_msg=f"{what}: work {k}")
        np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][k], err_msg=f"{what}: profile {k}")


# ---- 1. fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [(SLAB, ("Ptotal_x",)), (RK4, ("Ptotal_psi", "Ptotal_rho")),
                                        (RK4, ("Ptotal_rho", "Ptotal_psi")), (RK4, ("Ptotal_rho",))],
                         ids=["slab_x", "psi_rho", "rho_psi", "rho"])
def test_scan_runs_at_the_fixture_ds_equal_golden(name, order):
    """Three runs, ds = [fixture, half, fixture]: runs 0 and 2 are the reference post-processor's records and the golden
    summaries; run 1 is the single call with its ds, and its profile differs from run 0's (a kernel that ignored the
    per-run step would pass everything else)."""
    g, nml, p = _load(name)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    names, nb = fl.profile_names(g), int(g["dep_n_bins"])
    specs = [(w, nb) for w in order]
    ds = _ds_values(p)
    runs = _scan(p, r0, n0, power, specs, ds)
    for r in (0, 2):
        for k, w in enumerate(order):
            fl.assert_golden_deposition(runs[r]["works"][k], runs[r]["profiles"][k], g, names.index(w), f"{name} run {r} {w}")
        fl.assert_golden_summaries(runs[r], g, f"{name} run {r}")
    _assert_same_run(runs[1], _run_alone(p, ds[1], r0, n0, power, specs), f"{name} run 1")
    assert (runs[1]["profiles"][0] != runs[0]["profiles"][0]).any()


@pytest.mark.parametrize("specs", [[("Ptotal_psi", 1), ("Ptotal_rho", 320)], [("Ptotal_rho", 7), ("Ptotal_psi", 100)],
                                   [("Ptotal_psi", 320)]], ids=["1_320", "7_100_rho_first", "one_320"])
def test_scan_bin_counts_equal_the_single_calls(specs):
    g, nml, p = _load(RK4)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    ds = _ds_values(p)
    runs = _scan(p, r0, n0, power, specs, ds)
    for r in (0, 1):
        _assert_same_run(runs[r], _run_alone(p, ds[r], r0, n0, power, specs), f"{specs} run {r}")
    _assert_same_run(runs[2], runs[0], f"{specs} run 2 = run 0")


def test_scan_on_the_sg_kernel():
    """The SG fixture with nstep_max cut to 10: each of the three runs against the single call."""
    g, nml, p0 = _load(SG)
    p = copy_params(p0)
    p.nstep_max = 10
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 100)]
    ds = _ds_values(p)
    assert hip.profiles_kernel_name(p, 3 * len(r0), 2).startswith("sg_trace_kernel")
    runs = _scan(p, r0, n0, power, specs, ds)
    for r in (0, 1):
        _assert_same_run(runs[r], _run_alone(p, ds[r], r0, n0, power, specs), f"sg run {r}")
    _assert_same_run(runs[2], runs[0], "sg run 2 = run 0")
    assert (runs[1]["profiles"][1] != runs[0]["profiles"][1]).any() and runs[0]["npoints"].max() == 11


# ---- 2. refill ------------------------------------------------------------------------------------------------------------
def test_refilled_lanes_take_their_runs_step_and_weight():
    """The fixture fan tiled to resident lanes + 4500 rays, three runs in one launch (every lane is refilled across run
    boundaries), every member with a power of its own, one member outside the box and one refused at its initial check:
    each run equals the single call."""
    g, nml, p0 = _load(RK4)
    p = copy_params(p0)
    p.nstep_max = 40
    nray = _resident_lanes() + 4500
    r0, n0 = _tiled(g["rvec0_full"], g["rindex_vec0_full"], nray)
    r0[7, 0] = 10.0      # outside the box
    n0[11] *= 3.0        # stops at the initial check_save
    power = _distinct_powers(nray)
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 100)]
    ds = _ds_values(p)
    runs = _scan(p, r0, n0, power, specs, ds)
    for r in (0, 1):
        out = runs[r]
        assert out["npoints"][7] == 1 and out["npoints"][11] == 1 and out["npoints"].max() == p.nstep_max + 1
        for w in out["works"]:
            assert w.any() and not w[7].any() and not w[11].any()
        _assert_same_run(out, _run_alone(p, ds[r], r0, n0, power, specs), f"refill run {r}")
    _assert_same_run(runs[2], runs[0], "refill run 2 = run 0")
    assert (runs[1]["profiles"][0] != runs[0]["profiles"][0]).any()


# ---- 3. chaining ------------------------------------------------------------------------------------------------------------
def test_member_blocks_chain_per_run_through_profile_in():
    import torch
    g, nml, p = _load(RK4)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_psi", 100), ("Ptotal_rho", 33)]
    ds = _ds_values(p)
    h = 40
    whole = _scan(p, r0, n0, power, specs, ds)
    first = _scan(p, r0[:h], n0[:h], power[:h], specs, ds)
    carry = [torch.as_tensor(np.stack([run["profiles"][k] for run in first])).cuda() for k in range(2)]
    second = _scan(p, r0[h:], n0[h:], power[h:], specs, ds, profile_in=carry)
    assert len(r0) - h == 24
    for r in range(3):
        for k in range(2):
            np.testing.assert_array_equal(second[r]["profiles"][k], whole[r]["profiles"][k])
            np.testing.assert_array_equal(np.concatenate([first[r]["works"][k], second[r]["works"][k]]), whole[r]["works"][k])
            assert not np.array_equal(first[r]["profiles"][k], second[r]["profiles"][k])
    # one carry alone: the other profile starts every run from zero
    third = _scan(p, r0[h:], n0[h:], power[h:], specs, ds, profile_in=[None, carry[1]])
    for r in range(3):
        np.testing.assert_array_equal(third[r]["profiles"][1], whole[r]["profiles"][1])
        assert not np.array_equal(third[r]["profiles"][0], whole[r]["profiles"][0])


# ---- 4. beams ---------------------------------------------------------------------------------------------------------------
SEGMENTS = [0, 0, 1, 64, 65, 150]


@pytest.mark.parametrize("specs", [[("Ptotal_psi", 100), ("Ptotal_rho", 64)], [("Ptotal_rho", 7)]], ids=["two", "one"])
def test_each_beam_gets_the_profile_of_its_own_rays(specs):
    """150 rays with powers of their own in five ragged beams, the first one empty: every beam's profile is the single
    call's on that slice of rays, work is the unsegmented call's; a carry per beam continues it; uniform beams of 64
    rays (the last one ragged) equal the offsets [0, 64, 128, 150]."""
    import torch
    from rays_amd.trace import DeviceTrace
    g, nml, p = _load(RK4)
    r0, n0 = _tiled(g["rvec0_full"], g["rindex_vec0_full"], 150)
    power = _distinct_powers(150)

    def beams(segments, profile_in=None):
        tr = DeviceTrace(p, r0, n0, trajectories=False, deposition=list(specs), ray_power=power, segments=segments,
                         profile_in=profile_in)
        for w in tr.works:
            w.fill_(float("nan"))
        tr.launch()
        return tr.results()
    whole = _profiles(p, r0, n0, power, specs)
    recs = beams(SEGMENTS)
    n_seg = len(SEGMENTS) - 1
    assert all(r.summaries is recs[0].summaries for r in recs)
    sl.assert_same({k: getattr(recs[0].summaries, k) for k in sl.KEYS}, whole, "beams: summaries")
    for k, (w, nb) in enumerate(specs):
        assert recs[k].profile.shape == (n_seg, nb) and recs[k].Q_sum.shape == (n_seg,)
        np.testing.assert_array_equal(recs[k].work, whole["works"][k])
        assert not recs[k].profile[0].any() and not np.signbit(recs[k].profile[0]).any()   # the empty beam: +0.0
    for s in range(1, n_seg):
        a, b = SEGMENTS[s], SEGMENTS[s + 1]
        alone = _profiles(p, r0[a:b], n0[a:b], power[a:b], specs)
        for k in range(len(specs)):
            np.testing.assert_array_equal(recs[k].profile[s], alone["profiles"][k], err_msg=f"beam {s} profile {k}")
            assert recs[k].Q_sum[s] == fl.ordered_sum(alone["profiles"][k])
    carry = [torch.as_tensor(np.ascontiguousarray(r.profile)).cuda() for r in recs]
    again = beams(SEGMENTS, profile_in=carry)
    for k in range(len(specs)):
        assert (again[k].profile[1:] != recs[k].profile[1:]).any()
        for s in range(n_seg):
            a, b = SEGMENTS[s], SEGMENTS[s + 1]
            want = recs[k].profile[s].copy()
            for row in recs[k].work[a:b]:
                want = want + row
            np.testing.assert_array_equal(again[k].profile[s], want)
    uni, off = beams(64), beams([0, 64, 128, 150])
    for k in range(len(specs)):
        assert uni[k].profile.shape == (3, specs[k][1])
        np.testing.assert_array_equal(uni[k].profile, off[k].profile)
        assert (uni[k].profile[2] != 0.0).any()   # the ragged last beam: rays 128..149


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
def test_ray_scan_deposition_all_equals_the_runs_traced_one_by_one():
    from rays_amd.scan import RayScan
    from rays_amd.trace import RayDeposition, RaysRun
    g, nml, p = _load(RK4)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    ds = _ds_values(p)
    sc = RayScan(p, r0, n0, ds, trajectories=False, deposition="all", n_bins=100, ray_power=power)
    sc.launch()
    res = sc.results()
    assert len(res) == 3
    for r, recs in enumerate(res):
        q = copy_params(p)
        q.ds = ds[r]
        want = RaysRun(q, r0, n0, ray_pwr_wt=power).trace_rays(ngpu=1, trajectories=False, deposition="all", n_bins=100,
                                                               want_work=True)
        assert len(recs) == len(want) == 2 and all(isinstance(x, RayDeposition) for x in recs)
        assert [x.profile_name for x in recs] == [x.profile_name for x in want] == ["Ptotal_psi", "Ptotal_rho"]
        for a, b in zip(recs, want):
            np.testing.assert_array_equal(a.profile, b.profile)
            np.testing.assert_array_equal(a.work, b.work)
            assert a.Q_sum == b.Q_sum and a.n_bins == b.n_bins and (a.grid_min, a.grid_max) == (b.grid_min, b.grid_max)
            for k in sl.KEYS:
                np.testing.assert_array_equal(getattr(a.summaries, k), getattr(b.summaries, k), err_msg=k)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    import ctypes as C
    import torch
    lib = hip.load()
    d = torch.full((4096,), -7.0, dtype=torch.float64, device="cuda")
    i = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    D, I = d.data_ptr(), i.data_ptr()
    g, nml, axi = _load(RK4)
    PSI, RHO = hip.DEP_PROFILES["Ptotal_psi"], hip.DEP_PROFILES["Ptotal_rho"]

    def records(specs):
        arr = (hip.DepProfileStruct * max(len(specs), 1))()
        for r, s in zip(arr, specs):
            r.which, r.n_bins, r.work, r.profile_in, r.profile = s
        return arr

    def scan(n_runs, nray, specs, ds=D, n_profiles=None):
        return lib.rays_hip_scan_profiles_device(C.byref(axi), n_runs, ds, nray, D, D, D,
                                                 len(specs) if n_profiles is None else n_profiles, records(specs), I, I, None,
                                                 D, D, D, None)

    def seg(nray, specs, n_seg, off, per):
        return lib.rays_hip_trace_profiles_segments_device(C.byref(axi), nray, D, D, D, len(specs), records(specs), n_seg, off,
                                                           per, I, I, None, D, D, D, None)

    def refused(rc, text):
        assert rc != 0 and text in hip.last_error(), hip.last_error()
    ok = [(PSI, 10, D, None, D), (RHO, 12, D, None, D)]
    who = "rays_hip_scan_profiles_device"
    refused(scan(-1, 1, ok), who + ": n_runs < 0")
    refused(scan(1 << 16, 1 << 15, ok), who + ": n_runs * nray exceeds 2^31 - 1")
    refused(scan(2, 1, ok, ds=None), who + ": null d_ds_values")
    refused(scan(2, -1, ok), who + ": nray < 0")
    refused(scan(2, 1, ok, n_profiles=3), who + ": n_profiles = 3 is outside 1..2")
    refused(scan(2, 1, [ok[0], ok[0]]), who + ": the same profile twice")
    refused(scan(2, 1, [ok[0], (RHO, 321, D, None, D)]), who + ": n_bins = 321 is outside 1..320")
    refused(scan(2, 1, [ok[0], (RHO, 12, None, None, D)]), who + ": null work or profile")
    assert scan(0, 1, ok) == 0   # no run: nothing to do
    who = "rays_hip_trace_profiles_segments_device"
    refused(seg(1, ok, -1, None, 1), who + ": n_seg < 0")
    refused(seg(1, ok, 2, None, 0), who + ": neither segment offsets nor a positive rays_per_seg")
    refused(seg(-1, ok, 2, None, 1), who + ": nray < 0")
    refused(seg(1, [ok[0], (RHO, 0, D, None, D)], 2, None, 1), who + ": n_bins = 0 is outside 1..320")
    refused(seg(1, [(PSI, 10, None, None, D)], 2, None, 1), who + ": null work or profile")
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -7.0).all() and (i.cpu().numpy() == -7).all()
    from rays_amd.scan import RayScan
    from rays_amd.trace import DeviceTrace
    r0, n0 = g["rvec0"], g["rindex_vec0"]
    with pytest.raises(ValueError, match="trajectories=False"):
        RayScan(axi, r0, n0, [0.01], deposition=[("Ptotal_psi", 10)], ray_power=np.ones(len(r0)))
    with pytest.raises(ValueError, match="non-decreasing"):
        DeviceTrace(axi, r0, n0, trajectories=False, deposition=[("Ptotal_psi", 10)], ray_power=np.ones(len(r0)),
                    segments=[0, 5, 3])


# ---- 7. the Fortran interfaces ------------------------------------------------------------------------------------------------
def test_fortran_driver_reproduces_the_python_path(tmp_path):
    """tests/fortran/scan_profiles_driver.f90 + the binding, built with amdflang and linked against librays_hip.so:
    rays_hip_scan_profiles_device returns the Python path's bytes, and rays_hip_profile_sum_segments_device on the work it
    wrote, with the runs as uniform segments, the same profiles."""
    import os
    import shutil
    import subprocess

    from rays_amd.params import axisym_tables_struct
    from tests import emul_build as eb
    from tests.common import ROOT
    from tests.test_cpu_fused_profiles import TABLE_FIELDS
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    libdir = os.path.join(ROOT, "rays_amd", "lib")
    hipdir = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    srcs = [os.path.join(ROOT, "fortran", "rays_hip_m.f90"), os.path.join(ROOT, "tests", "fortran", "scan_profiles_driver.f90")]
    exe = str(tmp_path / "scan_profiles_driver")
    subprocess.check_call([fc, "-O2", "-ffp-contract=off", "-w", "-o", exe] + srcs +
                          ["-L" + libdir, "-lrays_hip", "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + hipdir], cwd=str(tmp_path))
    g, nml, p = _load(RK4)
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    specs = [("Ptotal_psi", 37), ("Ptotal_rho", 64)]
    ds = _ds_values(p)
    nray, nv, R = len(r0), p.nv, len(ds)
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
        f.write(np.array([R], dtype=np.int32).tobytes())
        f.write(np.array(ds, dtype=np.float64).tobytes())
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8)
    runs = _scan(p, r0, n0, power, specs, ds)
    want = {k: np.concatenate([run[k] for run in runs]) for k in sl.KEYS}
    for i, key in enumerate(("a", "b")):
        want["work_" + key] = np.concatenate([run["works"][i] for run in runs]).T   # bin-major: [n_bins][R * nray]
        want["profile_" + key] = np.stack([run["profiles"][i] for run in runs])
    want["profile_again"] = want["profile_a"]
    total, off = R * nray, 0
    for k, shape in [("npoints", (total,)), ("stop_code", (total,)), ("start_ray_vec", (total, nv)), ("end_ray_vec", (total, nv)),
                     ("end_residuals", (total,)), ("max_residuals", (total,)), ("work_a", (specs[0][1], total)),
                     ("profile_a", (R, specs[0][1])), ("work_b", (specs[1][1], total)), ("profile_b", (R, specs[1][1])),
                     ("profile_again", (R, specs[0][1]))]:
        integer = k in ("npoints", "stop_code")
        nbytes = int(np.prod(shape)) * (4 if integer else 8)
        got = raw[off:off + nbytes].view(np.int32 if integer else np.float64).reshape(shape)
        np.testing.assert_array_equal(got, want[k], err_msg="Fortran: " + k)
        off += nbytes
    assert off == raw.size
