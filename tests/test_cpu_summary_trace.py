"""CPU tier: summary-only tracing (rays_hip_trace_summary*, kernels with kEqNoTraj in EQ) -- the product kernel
sources in the variant that records no trajectory point, on the host emulation with TraceArgs::ray_vec and ::residual
NULL (a store the variant should not have crashes here, on the host); the host entry on the emulated four-device
runtime as a stand-alone program, plain and under ASan + UBSan; the Python plumbing.  Every comparison is on bit
patterns."""
import dataclasses
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

from rays_amd.params import copy_params
from tests import emul_lib, oracle_lib
from tests import summary_lib as sl
from tests.common import GOLDEN_CASES, ROOT, load_golden

EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")


# ---- 1. the fixtures on one emulated lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_summary_kernel_source_on_host_equals_reference(name):
    """All 38 fixtures: npoints, stop codes, end_ray_vec and the residual statistics are the golden files', and
    start_ray_vec is the golden ray_vec[:, 0, :] -- also for the rays the initial check_save refuses.  The recording
    kernel's own summaries of the same rays (the existing emulation) are the same bytes."""
    g, nml, p = load_golden(name)
    lib = sl.emul_lib()
    sl.set_axisym_tables(g, lib)
    out = sl.emul_trace(p, g["rvec0"], g["rindex_vec0"], lib=lib)
    sl.assert_same(out, sl.golden_summaries(g), name)
    sl.assert_same(out, sl.summaries_of(emul_lib.trace(p, g["rvec0"], g["rindex_vec0"])), name + " (recording kernel)")


def test_summary_scan_launch_on_host():
    """The fused scan's launch (ds per run): each run is its stand-alone summary trace and the full scan's summaries."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::64].copy(), g["rindex_vec0_full"][::64].copy()
    n0[3] *= 3.0   # stops at its initial check
    ds = np.array([p.ds, 0.5 * p.ds, 1.7 * p.ds])
    out = sl.emul_trace(p, r0, n0, ds_values=ds)
    full = emul_lib.scan(p, r0, n0, ds)
    for r, d in enumerate(ds):
        q = copy_params(p)
        q.ds = float(d)
        run = {k: out[k][r] for k in sl.KEYS}
        sl.assert_same(run, sl.emul_trace(q, r0, n0), f"run {r} against its stand-alone trace")
        sl.assert_same(run, sl.summaries_of({k: v[r] for k, v in full.items()}), f"run {r} against the full scan")
    assert len({tuple(out["npoints"][r]) for r in range(3)}) == 3


# ---- 2. whole emulated waves ---------------------------------------------------------------------------------------------
VARIANTS = {"default": [], "cost0": ["-DRAYS_REFILL_EVENT_COST=0"]}


def _wave_lib(variant):
    return sl.emul_lib(wave=True, tag="" if variant == "default" else variant, defs=VARIANTS[variant])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rk4_waves_with_refills(variant):
    """200 rays of the Solovev fan at their natural, ragged lengths on ONE wave (three times more rays than lanes: every
    lane is refilled, the last pass finds the counter dry), for two settings of RAYS_REFILL_EVENT_COST: in index order,
    "long rays first" with two neighbourhood sizes, and through the two-waves-per-SIMD build's body."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::5][:200].copy(), g["rindex_vec0_full"][::5][:200].copy()
    n0[7] *= 3.0   # far off the dispersion surface: stops at its initial check
    ref = sl.summaries_of(oracle_lib.trace(p, r0, n0))
    assert len(set(ref["npoints"].tolist())) > 20 and ref["npoints"][7] == 1
    lib = _wave_lib(variant)
    for stride in (0, 2, 16):
        sl.assert_same(sl.emul_waves(p, r0, n0, "rk4", 1, stride, lib=lib), ref, f"stride {stride}")
    sl.assert_same(sl.emul_waves(p, r0, n0, "rk4_w2", 1, lib=lib), ref, "two-waves body")


def test_rk4_waves_eqdsk_damping():
    """nv = 8 with the eqdsk tables and the Z-function table: 150 short rays on one wave."""
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    lib = _wave_lib("default")
    sl.set_axisym_tables(g, lib)
    reps = -(-150 // len(g["rvec0_full"]))
    r0, n0 = np.tile(g["rvec0_full"], (reps, 1))[:150], np.tile(g["rindex_vec0_full"], (reps, 1))[:150]
    q = copy_params(p)
    q.nstep_max = min(q.nstep_max, 60)
    ref = sl.summaries_of(oracle_lib.trace(q, r0, n0))
    sl.assert_same(sl.emul_waves(q, r0, n0, "rk4", 1, 0, lib=lib), ref, "index order")
    sl.assert_same(sl.emul_waves(q, r0, n0, "rk4", 1, 4, lib=lib), ref, "long rays first")


def test_sg_waves_with_refills():
    """sg_trace_kernel: 160 rays of the Solovev fan on ONE wave, every lane refilled once or twice."""
    g, nml, p = load_golden("gold_solovev64_sg_cold")
    reps = -(-160 // len(g["rvec0_full"]))
    r0 = np.tile(g["rvec0_full"], (reps, 1))[:160].copy()
    n0 = np.tile(g["rindex_vec0_full"], (reps, 1))[:160].copy()
    n0[5] *= 3.0
    q = copy_params(p)
    q.nstep_max = min(q.nstep_max, 40)
    ref = sl.summaries_of(oracle_lib.trace(q, r0, n0))
    assert ref["npoints"][5] == 1
    sl.assert_same(sl.emul_waves(q, r0, n0, "sg", 1, lib=_wave_lib("default")), ref)


@pytest.mark.parametrize("G", [4, 8])
def test_sg_group_waves_with_refills(G):
    """sg_group_kernel (one ray per group of G lanes): 80 rays on ONE resident block, finished groups pull the rest;
    a ray outside the box and one that stops at its initial check."""
    g, nml, p = load_golden("gold_solovev64_sg_num")
    q = copy_params(p)
    q.nstep_max = 3
    r0 = np.tile(g["rvec0_full"], (2, 1))[:80].copy()
    n0 = np.tile(g["rindex_vec0_full"], (2, 1))[:80].copy()
    r0[2, 0] = 10.0
    n0[3] *= 3.0
    ref = sl.summaries_of(oracle_lib.trace(q, r0, n0))
    sl.assert_same(sl.emul_waves(q, r0, n0, "sg_group", 1, G, lib=_wave_lib("default")), ref)


# ---- 3. the host entry on the emulated four-device runtime, stand-alone ----------------------------------------------------
def _case_file(path):
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    q = copy_params(p)
    q.nstep_max = 125
    r0, n0 = g["rvec0_full"][:301].copy(), g["rindex_vec0_full"][:301].copy()
    r0[17, 0] = 10.0      # launched outside the box: npoints = 1
    n0[40] *= 3.0         # off the dispersion surface: stops at the initial check
    full = oracle_lib.trace(q, r0, n0)
    ref = sl.summaries_of(full)
    assert ref["npoints"].min() == 1 and ref["npoints"].max() == 126 and len(np.unique(ref["npoints"])) > 5
    with open(path, "wb") as f:
        f.write(struct.pack("=3i", len(r0), q.nv, len(bytes(q))))
        f.write(bytes(q))
        for a in (r0, n0):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for k in sl.KEYS:
            f.write(np.ascontiguousarray(ref[k], dtype=np.int32 if k in ("npoints", "stop_code") else np.float64).tobytes())
        # the trajectories of the same trace, packed: points 1..npoints of ray 0, of ray 1, ... (ray_vec, then residual)
        for k in ("ray_vec", "residual"):
            f.write(np.concatenate([np.asarray(full[k], dtype=np.float64)[r, :n].ravel()
                                    for r, n in enumerate(ref["npoints"])]).tobytes())


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_entry_on_emulated_devices(sanitize, tmp_path):
    """rays_hip_trace_summary with 1 to 4 devices, a ragged last block and empty blocks, equals the oracle; the named
    refusals; after rays_hip_finalize the emulated driver reports no live allocation, pinned block, stream or event.
    rays_hip_trace on the same device lists and on one that repeats a device, with and without the kept result, and
    rays_hip_trace_gather on one device reproduce the oracle's trajectories bit for bit and write nothing else.
    Once plain and once as an ASan + UBSan executable with its own main (leak detection on)."""
    subprocess.check_call(["make", "-s", "-j", str(min(4, os.cpu_count() or 1)), "-f", "Makefile.capi", "summary"] +
                          (["SAN=1"] if sanitize else []), cwd=EMUL_DIR)
    exe = os.path.join(EMUL_DIR, "build_capi_san/emul_summary_capi_san" if sanitize else "build_capi/emul_summary_capi")
    case = str(tmp_path / "summary_case.bin")
    _case_file(case)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS", "LD_PRELOAD")}
    env.update(RAYS_EMUL_DEVICES="4")
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, case], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "summary capi ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 4. Python plumbing ------------------------------------------------------------------------------------------------
def test_ray_summaries_properties():
    from rays_amd import hip
    from rays_amd.trace import RaySummaries
    assert [f.name for f in dataclasses.fields(RaySummaries)][:6] == list(sl.KEYS)
    end = np.arange(14.0).reshape(2, 7)
    s = RaySummaries(np.array([5, 1], dtype=np.int32), np.array([1, 17], dtype=np.int32), np.zeros((2, 7)), end,
                     np.zeros(2), np.zeros(2))
    np.testing.assert_array_equal(s.end_ray_parameter, end[:, 6])
    assert s.total_steps == 4
    try:
        hip.load()
    except hip.RaysHipError:
        pytest.skip("librays_hip.so is not built here (stop flag texts come from the library)")
    assert s.ray_stop_flag == [hip.stop_flag_text(1), hip.stop_flag_text(17)]


class _FakeTensor:
    def __init__(self, shape):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)

    def to(self, device):
        return self

    def data_ptr(self):
        return 0


def _fake_torch(allocated):
    """The few torch names DeviceTrace / RayScan construct their tensors with; records every allocation's shape."""
    t = types.SimpleNamespace(float64="f64", int32="i32", int64="i64")

    def zeros(shape, dtype=None, device=None):
        x = _FakeTensor(shape)
        allocated.append(x.shape)
        return x
    t.zeros = zeros
    t.as_tensor = lambda a, dtype=None: _FakeTensor(np.shape(a))
    t.device = lambda *a: "cuda:0"

    class _Ctx:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False
    t.cuda = types.SimpleNamespace(current_device=lambda: 0, device=lambda d: _Ctx())
    return t


def test_trajectories_false_allocates_no_trajectory_tensor(monkeypatch):
    """DeviceTrace / RayScan(trajectories=False): ray_vec and residual are None, no tensor with an nstep_max + 1 axis
    is allocated, start_ray_vec exists; diagnostics() raises a clear error.  (torch and the parameter check are
    stand-ins here: what is examined is the object's attributes.)"""
    from rays_amd import hip, scan, trace
    g, nml, p = load_golden("cfg1_slab16_rk4")
    allocated = []
    monkeypatch.setitem(sys.modules, "torch", _fake_torch(allocated))
    monkeypatch.setattr(hip, "check_params", lambda q: None)
    npt, nv, n = p.nstep_max + 1, p.nv, len(g["rvec0"])
    dt = trace.DeviceTrace(p, g["rvec0"], g["rindex_vec0"], trajectories=False)
    assert dt.ray_vec is None and dt.residual is None and dt.trajectories is False
    assert dt.start_ray_vec.shape == (n, nv) and dt.end_ray_vec.shape == (n, nv) and dt.npoints.shape == (n,)
    assert allocated and all(npt not in s for s in allocated), allocated
    with pytest.raises(RuntimeError, match="summary-only"):
        dt.diagnostics()
    del allocated[:]
    sc = scan.RayScan(p, g["rvec0"], g["rindex_vec0"], [p.ds, 2 * p.ds], trajectories=False)
    assert sc.ray_vec is None and sc.residual is None and sc.start_ray_vec.shape == (2, n, nv)
    assert allocated and all(npt not in s for s in allocated), allocated
    # the default still allocates the trajectories
    del allocated[:]
    full = trace.DeviceTrace(p, g["rvec0"], g["rindex_vec0"])
    assert full.ray_vec.shape == (n, npt, nv) and full.residual.shape == (n, npt) and full.start_ray_vec is None
