"""CPU tier: segmented deposition -- the fused ds scan (rays_hip_scan_profiles_device) and one profile per segment of rays
(rays_hip_trace_profiles_segments_device, rays_hip_profile_sum_segments_device) -- on the emulated C ABI: a stand-alone
program (tests/hip_emul/emul_scan_profiles_capi_main.cpp, plain and as an ASan + UBSan build) makes the calls, this file
compares what it wrote.  Runs at a fixture's own ds against the reference post-processor's work / profile / Q_sum and the
golden summaries, the run at half that ds against the emulated single fused call with that ds; the Python layer's argument
checks that need no device.  Every comparison is on bit patterns; no tolerance appears anywhere."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from rays_amd.params import axisym_tables_struct, copy_params
from tests import emul_build as eb
from tests import fused_deposition_lib as fl
from tests import fused_profiles_lib as pl
from tests import scan_profiles_lib as spl
from tests import summary_lib as sl
from tests.common import ROOT, load_golden
from tests.test_cpu_fused_deposition import _rho
from tests.test_cpu_fused_profiles import TABLE_FIELDS
from tests.test_cpu_summary_trace import _fake_torch

EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")
CASES = {"gold_slab16_damp_rk4": (["Ptotal_x"], [0, 0, 1, 7, 16]),
         "gold_axisym64_eqdsk_damp_rk4": (["Ptotal_psi", "Ptotal_rho"], [0, 0, 1, 40, 41, 64])}


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_of_the_segmented_sum():
    """tests/scan_profiles_lib.profile_sum_segments: a segment is dr.profile_sum of its slice continued from its carry;
    an empty one gives its carry or +0.0; offsets are clamped; rays outside every segment count nowhere; the sum depends
    on the ray order."""
    from tests import deposition_ref as dr
    work = spl.synthetic_work(200, 5)
    off = [3, 3, 4, 70, 199]
    carry = spl.synthetic_carry(4, 5)
    got = spl.profile_sum_segments(work, off, carry)
    for s in range(4):
        np.testing.assert_array_equal(got[s], dr.profile_sum(work[off[s]:off[s + 1]], carry[s]))
    np.testing.assert_array_equal(got[0], carry[0])
    zero = spl.profile_sum_segments(work, off, None)[0]
    assert not zero.any() and not np.signbit(zero).any()
    clamped = spl.profile_sum_segments(work, [-9, 10, 4, 999], None)   # [0, 10), nothing (the end lies before the start), [4, 200)
    np.testing.assert_array_equal(clamped, [dr.profile_sum(work[:10]), np.zeros(5), dr.profile_sum(work[4:])])
    np.testing.assert_array_equal(spl.profile_sum_segments(work, spl.uniform_offsets(3, 64), None)[2],
                                  dr.profile_sum(work[128:192]))
    assert (spl.profile_sum_segments(work, off, None, reverse=True) != spl.profile_sum_segments(work, off, None)).any()


# ---- 2. the entries on the emulated C ABI, stand-alone -------------------------------------------------------------------
def _case_file(path, name):
    g, nml, p = load_golden(name)
    order, seg = CASES[name]
    nb = int(g["dep_n_bins"])
    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    nray = len(r0)
    ds = [float(p.ds), 0.5 * float(p.ds), float(p.ds)]
    axisym = int(p.equilib_model) != 0
    rho = _rho(g)
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    which = [fl.WHICH[w] for w in order] + [0] * (2 - len(order))
    with open(path, "wb") as f:
        f.write(struct.pack("=12i", nray, p.nv, len(order), nb, nb if len(order) == 2 else 0, which[0], which[1],
                            len(z["fspl_re"]), len(bytes(p)), len(ds), int(axisym), len(seg) - 1))
        f.write(bytes(p))
        f.write(np.array([float(z["x_min"]), float(z["x_max"])]).tobytes())
        f.write(np.ascontiguousarray(z["fspl_re"], dtype=np.float64).tobytes())
        if axisym:
            tab = eb.axisym_tables_of(g)
            t, keep = axisym_tables_struct(tab)
            f.write(struct.pack("=6i", t.nr, t.nz, t.n_rb, t.n_ne, t.n_te, t.n_ti))
            for field in TABLE_FIELDS:
                a = np.ascontiguousarray(tab.get(field, ()), dtype=np.float64).ravel()
                f.write(struct.pack("=i", a.size))
                f.write(a.tobytes())
        f.write(struct.pack("=i", 0 if rho is None else len(rho[0])))
        for a in (() if rho is None else rho) + (r0, n0, power, ds):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(seg, dtype=np.int32).tobytes())
    return g, p, order, nb, ds, seg


class _Reader:
    def __init__(self, path):
        self.raw, self.at = np.fromfile(path, dtype=np.uint8), 0

    def take(self, shape, dtype=np.float64):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = self.raw[self.at:self.at + n].view(dtype).reshape(shape)
        self.at += n
        return a

    def summaries(self, rows, nv):
        return dict(npoints=self.take((rows,), np.int32), stop_code=self.take((rows,), np.int32),
                    start_ray_vec=self.take((rows, nv)), end_ray_vec=self.take((rows, nv)), end_residuals=self.take((rows,)),
                    max_residuals=self.take((rows,)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("name", list(CASES))
def test_entries_on_the_emulated_c_abi(name, sanitize, tmp_path):
    """Three runs, ds = [fixture, half, fixture], in ONE call of rays_hip_scan_profiles_device: runs 0 and 2 are the
    reference post-processor's work / profile / Q_sum and the golden summaries; run 1 is the emulated single fused call with
    its ds, and its profile differs from run 0's (a kernel that ignored the per-run step would pass everything else).
    Member blocks chained through profile_in give the unsplit scan's profiles.  The segments entry: the unsegmented
    call's work and summaries, and per segment the restatement's sum over that work.  The program checks the refusals,
    the empty calls, that a repeated call allocates nothing and that rays_hip_finalize leaves nothing behind -- once plain
    and once as an ASan + UBSan executable with its own main (leak detection on)."""
    subprocess.check_call(["make", "-s", "-j", str(min(4, os.cpu_count() or 1)), "-f", "Makefile.scan_profiles", "scan_profiles"] +
                          (["SAN=1"] if sanitize else []), cwd=EMUL_DIR)
    exe = os.path.join(EMUL_DIR, "build_capi_san/emul_scan_profiles_capi_san" if sanitize else "build_capi/emul_scan_profiles_capi")
    case, result = str(tmp_path / "scan_case.bin"), str(tmp_path / "scan_out.bin")
    g, p, order, nb, ds, seg = _case_file(case, name)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS", "LD_PRELOAD")}
    env.update(RAYS_EMUL_DEVICES="1")
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, case, result], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "scan profiles capi ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

    r0, n0, power = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    nray, nv, R, names = len(r0), p.nv, len(ds), fl.profile_names(g)
    rd = _Reader(result)
    # (1) the scan
    summ = rd.summaries(R * nray, nv)
    works, profs = [], []
    for _ in order:
        works.append(rd.take((nb, R * nray)))
        profs.append(rd.take((R, nb)))
    runs = []
    for k in range(R):
        out = {key: a[k * nray:(k + 1) * nray] for key, a in summ.items()}
        out["works"] = [np.ascontiguousarray(w[:, k * nray:(k + 1) * nray].T) for w in works]
        out["profiles"] = [q[k] for q in profs]
        runs.append(out)
    for k in (0, 2):
        for i, w in enumerate(order):
            fl.assert_golden_deposition(runs[k]["works"][i], runs[k]["profiles"][i], g, names.index(w), f"{name} run {k} {w}")
        fl.assert_golden_summaries(runs[k], g, f"{name} run {k}")
    q = copy_params(p)
    q.ds = ds[1]
    lib = pl.emul_lib() if len(order) == 2 else fl.emul_lib()
    sl.set_axisym_tables(g, lib)
    if len(order) == 2:
        alone = pl.emul_profiles(q, r0, n0, power, [(w, nb) for w in order], rho=_rho(g), lib=lib)
    else:
        one = fl.emul_fused(q, r0, n0, power, order[0], nb, rho=_rho(g), lib=lib)
        alone = dict(one, works=[one["work"]], profiles=[one["profile"]])
    sl.assert_same(runs[1], alone, f"{name} run 1")
    for i in range(len(order)):
        np.testing.assert_array_equal(runs[1]["works"][i], alone["works"][i], err_msg=f"run 1 work {i}")
        np.testing.assert_array_equal(runs[1]["profiles"][i], alone["profiles"][i], err_msg=f"run 1 profile {i}")
        assert (runs[1]["profiles"][i] != runs[0]["profiles"][i]).any()
    # (2) member blocks chained per run
    for i in range(len(order)):
        np.testing.assert_array_equal(rd.take((R, nb)), profs[i], err_msg=f"chained profile {i}")
    # (3) one profile per segment
    ssum = rd.summaries(nray, nv)
    sl.assert_same(ssum, runs[0], f"{name} segments: summaries")
    for i in range(len(order)):
        swork, sprof = rd.take((nb, nray)), rd.take((len(seg) - 1, nb))
        np.testing.assert_array_equal(swork.T, runs[0]["works"][i], err_msg=f"segments work {i}")
        np.testing.assert_array_equal(sprof, spl.profile_sum_segments(swork.T, seg), err_msg=f"segments profile {i}")
        assert not sprof[0].any() and sprof[1:].any()
    assert rd.at == rd.raw.size


# ---- 3. the Python layer's argument checks ----------------------------------------------------------------------------------
def test_python_layer_argument_checks(monkeypatch):
    from rays_amd import hip, scan, trace
    allocated = []
    monkeypatch.setitem(sys.modules, "torch", _fake_torch(allocated))
    sys.modules["torch"].is_tensor = lambda x: False
    monkeypatch.setattr(hip, "check_params", lambda q: None)
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    r0, n0 = g["rvec0"], g["rindex_vec0"]
    n, npt = len(r0), p.nstep_max + 1
    pw = np.ones(n)
    lst = [("Ptotal_rho", 7), ("Ptotal_psi", 100)]
    # segments
    assert trace.check_segments([0, 0, 1, n], n, "t")[0] == 3 and trace.check_segments(5, 12, "t") == (3, None, 5)
    for bad, text in (([0, 5, 3], "non-decreasing"), ([-1, 3], "within 0..nray"), ([0, n + 1], "within 0..nray"),
                      ([], "n_seg \\+ 1 integer offsets"), ([0.5, 2.0], "n_seg \\+ 1 integer offsets"), (0, "at least one ray")):
        with pytest.raises(ValueError, match=text):
            trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=lst, ray_power=pw, segments=bad)
    with pytest.raises(ValueError, match="segments= goes with the list spelling"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_psi", 9, pw), segments=[0, n])
    with pytest.raises(ValueError, match="segments= goes with the list spelling"):
        trace.DeviceTrace(p, r0, n0, segments=[0, n])
    dt = trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=lst, ray_power=pw, segments=[0, 2, 2, n])
    assert [q.shape for q in dt.profiles] == [(3, 7), (3, 100)] and [w.shape for w in dt.works] == [(7, n), (100, n)]
    assert dt.segments[0] == 3 and dt.segments[2] == 0
    # the scan
    with pytest.raises(ValueError, match="RayScan: deposition=... is the fused scan without trajectories"):
        scan.RayScan(p, r0, n0, [0.01, 0.02], trajectories=True, deposition=lst, ray_power=pw)
    with pytest.raises(ValueError, match="one weight per fan member"):
        scan.RayScan(p, r0, n0, [0.01, 0.02], trajectories=False, deposition=lst)
    with pytest.raises(ValueError, match="one weight per fan member"):
        scan.RayScan(p, r0, n0, [0.01, 0.02], trajectories=False, deposition=lst, ray_power=pw[:-1])
    with pytest.raises(ValueError, match="one entry"):
        scan.RayScan(p, r0, n0, [0.01, 0.02], trajectories=False, deposition=lst, ray_power=pw, profile_in=[None])
    with pytest.raises(ValueError, match="go with deposition"):
        scan.RayScan(p, r0, n0, [0.01, 0.02], trajectories=False, ray_power=pw)
    with pytest.raises(ValueError, match="twice"):
        scan.RayScan(p, r0, n0, [0.01], trajectories=False, deposition=[("Ptotal_psi", 5), ("Ptotal_psi", 6)], ray_power=pw)
    allocated.clear()
    sc = scan.RayScan(p, r0, n0, [0.01, 0.02, 0.03], trajectories=False, deposition=lst, ray_power=pw)
    assert sc.ray_vec is None and sc.residual is None and sc.deposition == lst
    assert [w.shape for w in sc.works] == [(7, 3 * n), (100, 3 * n)] and [q.shape for q in sc.profiles] == [(3, 7), (3, 100)]
    assert allocated and all(npt not in s for s in allocated), allocated
    # Q_sum of a profile per segment: one ordered sum per row
    rec = trace.RayDeposition(None, "Ptotal_psi", 3, 0.0, 1.0, np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.5]]), None)
    np.testing.assert_array_equal(rec.Q_sum, [6.0, 0.5])


def test_binding_declares_the_entries():
    from rays_amd import hip
    for sym in ("rays_hip_profile_sum_segments_device", "rays_hip_scan_profiles_device",
                "rays_hip_trace_profiles_segments_device"):
        assert sym in hip.EXPORTED_SYMBOLS
        assert sym in open(os.path.join(ROOT, "include", "rays_hip.h")).read()
        assert sym in open(os.path.join(ROOT, "fortran", "rays_hip_m.f90")).read()
    try:
        lib = hip.load()
    except hip.RaysHipError:
        pytest.skip("librays_hip.so is not built here")
    assert len(lib.rays_hip_profile_sum_segments_device.argtypes) == 9
    assert len(lib.rays_hip_scan_profiles_device.argtypes) == 16
    assert len(lib.rays_hip_trace_profiles_segments_device.argtypes) == 17
