"""CPU tier: deposition windows (rays_hip_trace_window_profiles_device; the trace kernels with kEqContinue | kEqNoTraj |
kEqDeposit [| kEqDeposit2] in EQ) -- the product kernel sources in the variant that continues rays from a saved state
and bins every point it accepts, on the host emulation; the C ABI entry on the emulated runtime, stand-alone; the Python
surface without a device.  Every comparison is on bit patterns; no tolerance appears anywhere."""
import os
import subprocess

import numpy as np
import pytest

from rays_amd.params import STOP_CODE, copy_params
from tests import emul_build as eb
from tests import emul_lib
from tests import fused_deposition_lib as fl
from tests import fused_profiles_lib as pl
from tests import summary_lib as sl
from tests import window_deposition_lib as wd
from tests import window_lib as wl
from tests.common import ROOT, load_golden
from tests.test_cpu_fused_deposition import _rho, _wave_case
from tests.test_cpu_fused_profiles import _case_file

EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")
SEQUENCES = {"one_step": lambda p: [1], "7_1_13": lambda p: [7, 1, 13], "one_window": lambda p: [p.nstep_max + 1]}


def _lib_for(g, wave=False):
    lib = wd.emul_lib(wave=wave)
    sl.set_axisym_tables(g, lib)
    return lib


# ---- 1. the fixtures on one emulated lane, one profile per run --------------------------------------------------------
@pytest.mark.parametrize("seq", list(SEQUENCES))
@pytest.mark.parametrize("name", fl.DEP_FIXTURES)
def test_windowed_kernel_source_on_host_equals_reference(name, seq):
    """The twelve fixtures with the reference post-processor's results, full fan, the fixture's 100 bins, every profile
    each carries: from state_init and zeroed works, windows of one step, of 7, 1, 13 steps cycled, and one window longer
    than any ray end at dep_work, dep_profile and dep_q_sum and at the golden summaries.  Under one-step windows every
    segment that deposits starts from an x_prev / q_prev the `first` arm re-established.  Calls after the end of every ray
    change no byte and return npoints_win = 0 (wd.run_windowed)."""
    g, nml, p = load_golden(name)
    lib = _lib_for(g)
    nb = int(g["dep_n_bins"])
    assert nb == 100
    for i, which in enumerate(fl.profile_names(g)):
        out = wd.run_windowed(p, g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], [(which, nb)], SEQUENCES[seq](p),
                              rho=_rho(g), lib=lib, extra_windows=2)
        what = f"{name} {which} {seq}"
        fl.assert_golden_deposition(out["works"][0], out["profiles"][0], g, i, what)
        fl.assert_golden_summaries(out, g, what)
        assert out["profiles"][0].sum() > 0, what
        if seq == "one_step":
            assert out["windows"] >= int(g["npoints_full"].max()) - 1
        if seq == "one_window":
            assert out["windows"] == 1


# ---- 2. both profiles in one windowed run ------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [(1, 320), (320, 1), (7, 100)])
@pytest.mark.parametrize("order", pl.ORDERS, ids=["psi_rho", "rho_psi"])
@pytest.mark.parametrize("name", pl.TWO_PROFILE_FIXTURES)
def test_two_profiles_equal_two_single_profile_windowed_runs(name, order, bins):
    """The six two-profile fixtures, both request orders, three pairs of bin counts, windows of 7, 1, 13 steps: each work
    and profile of the two-profile windowed run equals the single-profile windowed run's, and the summaries agree."""
    g, nml, p = load_golden(name)
    lib = _lib_for(g)
    r0, n0, pw, rho = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], _rho(g)
    specs = [(order[0], bins[0]), (order[1], bins[1])]
    out = wd.run_windowed(p, r0, n0, pw, specs, [7, 1, 13], rho=rho, lib=lib)
    for k, spec in enumerate(specs):
        ref = wd.run_windowed(p, r0, n0, pw, [spec], [7, 1, 13], rho=rho, lib=lib)
        sl.assert_same(out, ref, f"{name} {spec}")
        np.testing.assert_array_equal(out["works"][k], ref["works"][0], err_msg=f"{name} {spec}: work")
        np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][0], err_msg=f"{name} {spec}: profile")
        assert out["works"][k].any()
    fl.assert_golden_summaries(out, g, name)


def test_two_profiles_one_step_windows_equal_the_one_shot_pass():
    """One-step windows of the two-profile kernel against the ONE-SHOT two-profile emulation: both x_prev are
    re-established before every segment."""
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_sg")
    lib = _lib_for(g)
    r0, n0, pw, rho = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], _rho(g)
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 100)]
    ref = pl.emul_profiles(p, r0, n0, pw, specs, rho=rho, lib=lib)
    out = wd.run_windowed(p, r0, n0, pw, specs, [1], rho=rho, lib=lib)
    sl.assert_same(out, ref, "summaries")
    for k in range(2):
        np.testing.assert_array_equal(out["works"][k], ref["works"][k])
        np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][k])
    assert not np.array_equal(ref["works"][0], np.zeros_like(ref["works"][0]))


# ---- 3. the prefix contract -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gold_axisym64_eqdsk_damp_rk4", "gold_slab16_damp_rk4"])
def test_every_prefix_equals_the_deposition_of_the_clipped_trajectories(name):
    """After every window of 7, 1, 13 (cycled) each work equals the existing deposition emulation (deposit_ray) on the
    fixture's full trajectories with npoints clipped to state.nstep + 1."""
    g, nml, p = load_golden(name)
    lib = _lib_for(g)
    tab = eb.axisym_tables_of(g)
    if tab is not None:
        emul_lib.set_axisym_tables(tab)
    rho = _rho(g)
    grid, fspl = rho if rho is not None else (np.zeros(2), np.zeros(8))
    names = fl.profile_names(g)
    specs = [(w, 100) for w in names]
    rv, pw = g["dep_ray_vec_full"], g["dep_power"]
    q = copy_params(p)   # the fixture keeps the trajectories up to its longest ray: the padded layout of THAT length
    q.nstep_max = rv.shape[1] - 1
    seen = []

    def check(k, st, works):
        clipped = np.minimum(st["nstep"] + 1, g["npoints_full"]).astype(np.int32)
        np.testing.assert_array_equal(clipped, st["nstep"] + 1)
        for (w, nb), work in zip(specs, works):
            ref, _ = emul_lib.deposition(q, fl.WHICH[w], nb, rv, clipped, pw, grid, fspl)
            np.testing.assert_array_equal(work.T, ref, err_msg=f"{name} {w} after window {k}")
        seen.append(int(clipped.sum()))

    out = wd.run_windowed(p, g["rvec0_full"], g["rindex_vec0_full"], pw, specs, [7, 1, 13], rho=rho, lib=lib,
                          after_window=check)
    assert len(seen) >= 4 and seen == sorted(seen) and seen[0] < seen[-1]
    for i, w in enumerate(names):
        fl.assert_golden_deposition(out["works"][i], out["profiles"][i], g, i, f"{name} {w}")


# ---- 4. whole emulated waves ------------------------------------------------------------------------------------------
def _outside_the_box(g, r0):
    """Ray 5 launched far outside the equilibrium's box: it starts (the initial check looks at the dispersion relation
    only where the equilibrium says so) or is refused -- either way it ends at once and its row stays zero."""
    r0 = r0.copy()
    r0[5] = r0[5] * 50.0
    return r0


def test_rk4_waves_with_refills_in_windows():
    """192 damped eqdsk rays on ONE emulated wave -- three times more rays than lanes, so every lane is refilled twice in
    every window and a refilled lane re-establishes x_prev / q_prev of the ray it takes over -- with one ray outside
    the box and one refused at its initial check, distinct powers, in index order and long-first; windows of 7, 1, 13.
    One and two profiles, against the one-shot fused wave emulation."""
    g, q, r0, n0, power = _wave_case("gold_axisym64_eqdsk_damp_rk4", 192, 80)
    r0 = _outside_the_box(g, r0)
    lane, lib = _lib_for(g), _lib_for(g, wave=True)
    rho = _rho(g)
    specs = [("Ptotal_psi", 100), ("Ptotal_rho", 64)]
    ref = pl.emul_profiles_waves(q, r0, n0, power, specs, "rk4", 1, 0, rho=rho, lib=lib)
    assert ref["npoints"][9] == 1 and not ref["works"][0][9].any() and ref["npoints"][5] == 1
    assert (ref["stop_code"] == [v for k, v in STOP_CODE.items() if k.strip() == "total_absorption"][0]).any()
    assert len({tuple(w) for w in ref["works"][0]}) > 150
    for stride in (0, 2):
        out = wd.run_windowed(q, r0, n0, power, specs, [7, 1, 13], rho=rho, lib=lane, waves=("rk4", 1, stride),
                              wave_lib=lib, extra_windows=1)
        sl.assert_same(out, ref, f"stride {stride}")
        for k in range(2):
            np.testing.assert_array_equal(out["works"][k], ref["works"][k], err_msg=f"stride {stride}: work {k}")
            np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][k], err_msg=f"stride {stride}: profile {k}")
    one = wd.run_windowed(q, r0, n0, power, specs[1:], [7, 1, 13], rho=rho, lib=lane, waves=("rk4", 1, 2), wave_lib=lib)
    np.testing.assert_array_equal(one["works"][0], ref["works"][1])
    sl.assert_same(one, ref, "one profile")


def test_sg_waves_with_refills_in_windows():
    """The same for sg_trace_kernel on the SG wave emulator: 192 rays on one wave, nstep_max = 12, windows of 5, 1, 3."""
    g, q, r0, n0, power = _wave_case("gold_axisym64_eqdsk_damp_sg", 192, 12)
    r0 = _outside_the_box(g, r0)
    lane, lib = _lib_for(g), _lib_for(g, wave=True)
    rho = _rho(g)
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 50)]
    ref = pl.emul_profiles_waves(q, r0, n0, power, specs, "sg", 1, rho=rho, lib=lib)
    assert ref["npoints"][9] == 1 and ref["npoints"][5] == 1 and ref["npoints"].max() == 13
    assert len({tuple(w) for w in ref["works"][1]}) > 64
    out = wd.run_windowed(q, r0, n0, power, specs, [5, 1, 3], rho=rho, lib=lane, waves=("sg", 1, 0), wave_lib=lib,
                          extra_windows=1)
    sl.assert_same(out, ref, "sg")
    for k in range(2):
        np.testing.assert_array_equal(out["works"][k], ref["works"][k])
        np.testing.assert_array_equal(out["profiles"][k], ref["profiles"][k])
    single = fl.emul_fused_waves(q, r0, n0, power, "Ptotal_psi", 50, "sg", 1, rho=rho, lib=lib)
    one = wd.run_windowed(q, r0, n0, power, specs[1:], [5, 1, 3], rho=rho, lib=lane, waves=("sg", 1, 0), wave_lib=lib)
    np.testing.assert_array_equal(one["works"][0], single["work"])


# ---- 5. one-token changes to the new device code -----------------------------------------------------------------------
MUTATIONS = {
    # the `first` arm's re-establishing call dropped (RK4, one profile)
    "first_arm_call_dropped": (
        "rays_rk4_body.inc",
        "} else if constexpr (kDeposit) {\n              const TraceArgs& A = cold_args(A_hot);\n"
        "              dep_trace_point(P, *A.dep(), ray, v, dep_x_prev, dep_q_prev);",
        "} else if constexpr (false) {\n              const TraceArgs& A = cold_args(A_hot);\n"
        "              dep_trace_point(P, *A.dep(), ray, v, dep_x_prev, dep_q_prev);"),
    # the second profile's x_prev taken from the first grid value (what the `first` arm of the two-profile kernels calls)
    "x_prev_of_b_from_a": ("rays_deposition.hpp", "  xb_prev = xb;  // (its own", "  xb_prev = xa;  // (its own"),
    # the power of ray 0 used for q_prev (SG `first` arm, one profile)
    "q_prev_with_power_of_ray_0": (
        "rays_sg.hpp",
        "{\n            const TraceArgs& A = cold_args(A_hot);\n            dep_trace_point(P, *A.dep(), ray, yy,",
        "{\n            const TraceArgs& A = cold_args(A_hot);\n            dep_trace_point(P, *A.dep(), 0, yy,"),
}
MUTATION_CASES = {"first_arm_call_dropped": ("gold_axisym64_eqdsk_damp_rk4", [("Ptotal_psi", 100)]),
                  "x_prev_of_b_from_a": ("gold_axisym64_eqdsk_damp_rk4", [("Ptotal_psi", 7), ("Ptotal_rho", 100)]),
                  "q_prev_with_power_of_ray_0": ("gold_axisym64_eqdsk_damp_sg", [("Ptotal_psi", 100)])}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_one_token_changes_are_caught(mutation, tmp_path):
    """Three one-token changes to the new device code, each built into an emulation library of its
    own.  Each breaks the comparison of tests 1 and 2 on eight rays of a fixture under one-step windows -- the rays'
    powers made distinct, as in test 4, for the third -- while the unchanged sources pass the same comparison."""
    file, old, new = MUTATIONS[mutation]
    out_lib = str(tmp_path / "librays_emul_windep_mut.so")
    eb.build(wd.SRC, out_lib, pl.BASE_DEFS, directory=eb.mutated_tree(str(tmp_path / "tree"), file, old, new))
    bad = eb.load(out_lib)
    wd.declare(bad, False)
    name, specs = MUTATION_CASES[mutation]
    g, nml, p = load_golden(name)
    sl.set_axisym_tables(g, bad)
    good = _lib_for(g)
    r0, n0, rho = g["rvec0_full"][:8], g["rindex_vec0_full"][:8], _rho(g)
    pw = g["dep_power"][:8] * (1.0 + 0.25 * np.arange(8))
    if len(specs) == 2:
        ref = pl.emul_profiles(p, r0, n0, pw, specs, rho=rho, lib=good)["works"]
    else:
        ref = [fl.emul_fused(p, r0, n0, pw, *specs[0], rho=rho, lib=good)["work"]]
    assert all(w.any() for w in ref)

    def same(lib, sizes):
        out = wd.run_windowed(p, r0, n0, pw, specs, sizes, rho=rho, lib=lib)
        return all(np.array_equal(a, b) for a, b in zip(out["works"], ref))
    assert same(good, [1])
    assert not same(bad, [1])


# ---- 6. the C ABI entry on the emulated runtime, stand-alone -----------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_c_abi_entry_on_the_emulated_runtime(sanitize, tmp_path):
    """rays_hip_trace_window_profiles_device on the emulated runtime (emul_window_profiles_capi_main.cpp): 101 rays with
    distinct powers, one refused at its initial check; two records in both orders and each record alone; exactly sized,
    poisoned work rows; the profile summed only where asked; calls after the end; every named refusal; after
    rays_hip_finalize the emulated driver holds nothing.  Once plain and once as an ASan + UBSan executable with its
    own main (leak detection on)."""
    subprocess.check_call(["make", "-s", "-j", str(min(4, os.cpu_count() or 1)), "-f", "Makefile.window_profiles",
                           "window_profiles"] + (["SAN=1"] if sanitize else []), cwd=EMUL_DIR)
    exe = os.path.join(EMUL_DIR, "build_capi_san/emul_window_profiles_capi_san" if sanitize
                       else "build_capi/emul_window_profiles_capi")
    case = str(tmp_path / "window_profiles_case.bin")
    _case_file(case)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS", "LD_PRELOAD")}
    env.update(RAYS_EMUL_DEVICES="4")
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, case], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "window profiles capi ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 7. the Python surface, without a device ----------------------------------------------------------------------------
def test_python_surface_without_a_device(monkeypatch, tmp_path):
    """WindowedDeposition on CPU tensors: what it allocates, its refusals by name, save() / load() byte for byte, the
    kernels refused on a CPU object -- and DeviceTrace(window=..., deposition=...) goes on raising."""
    torch = pytest.importorskip("torch")
    from rays_amd import hip, trace
    monkeypatch.setattr(hip, "check_params", lambda q: None)
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    r0, n0 = g["rvec0"], g["rindex_vec0"]
    n = len(r0)
    pw = np.linspace(0.5, 1.5, n)
    specs = [("Ptotal_rho", 7), ("Ptotal_psi", 100)]
    w = trace.WindowedDeposition(p, r0, n0, deposition=specs, ray_power=pw, device="cpu")
    assert w.deposition == specs and [tuple(x.shape) for x in w.works] == [(7, n), (100, n)]
    assert [tuple(x.shape) for x in w.profiles] == [(7,), (100,)] and w.state.nray == n and w.state.nv == p.nv
    assert tuple(w.npoints_win.shape) == (n,) and w.npoints_win.dtype == torch.int32
    # nothing with an nstep_max + 1 axis
    assert all(p.nstep_max + 1 not in tuple(t.shape) for t in vars(w).values() if torch.is_tensor(t))
    monkeypatch.setattr(hip, "deposition_profile_set", lambda q: ("Ptotal_psi", "Ptotal_rho"))
    al = trace.WindowedDeposition(p, r0, n0, deposition="all", n_bins=50, ray_power=pw, device="cpu")
    assert al.deposition == [("Ptotal_psi", 50), ("Ptotal_rho", 50)]
    with pytest.raises(ValueError, match="needs ray_power="):
        trace.WindowedDeposition(p, r0, n0, deposition=specs, device="cpu")
    with pytest.raises(ValueError, match="ray_power must hold one weight per ray"):
        trace.WindowedDeposition(p, r0, n0, deposition=specs, ray_power=pw[:-1], device="cpu")
    with pytest.raises(ValueError, match=r"deposition=\[\(which, n_bins\), \.\.\.\] or \"all\""):
        trace.WindowedDeposition(p, r0, n0, deposition=("Ptotal_psi", 5, pw), ray_power=pw, device="cpu")
    with pytest.raises(ValueError, match=r"deposition=\[\(which, n_bins\), \.\.\.\] or \"all\""):
        trace.WindowedDeposition(p, r0, n0, ray_power=pw, device="cpu")
    with pytest.raises(ValueError, match="twice"):
        trace.WindowedDeposition(p, r0, n0, deposition=[("Ptotal_psi", 5), ("Ptotal_psi", 6)], ray_power=pw, device="cpu")
    with pytest.raises(ValueError, match=r"takes 1\.\.2 profiles"):
        trace.WindowedDeposition(p, r0, n0, deposition=[], ray_power=pw, device="cpu")
    with pytest.raises(ValueError, match="'Ptotal_x' does not exist for this equilib_model"):
        trace.WindowedDeposition(p, r0, n0, deposition=[("Ptotal_x", 5)], ray_power=pw, device="cpu")
    with pytest.raises(ValueError, match="needs n_bins=n"):
        trace.WindowedDeposition(p, r0, n0, deposition="all", ray_power=pw, device="cpu")
    with pytest.raises(ValueError, match="one entry"):
        trace.WindowedDeposition(p, r0, n0, deposition=specs, ray_power=pw, profile_in=[None], device="cpu")
    with pytest.raises(ValueError, match="one tensor"):
        trace.WindowedDeposition(p, r0, n0, deposition=specs, ray_power=pw, works=[torch.zeros((7, n))], device="cpu")
    with pytest.raises(ValueError, match="one tensor"):
        trace.WindowedDeposition(p, r0, n0, deposition=specs, ray_power=pw, device="cpu",
                                 works=[torch.zeros((7, n)), torch.zeros((n, 100))])
    with pytest.raises(ValueError, match="state= does not match this fan"):
        trace.WindowedDeposition(p, r0, n0, deposition=specs, ray_power=pw, device="cpu",
                                 state=trace.RayState(n + 1, p.nv, device="cpu"))
    with pytest.raises(ValueError, match="n_steps must be >= 1"):
        w.advance(0)
    for call in (w.launch, lambda: w.advance(3), w.results):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # save / load: the state of an emulated run after two windows, both works, the powers and the list
    lib = _lib_for(g)
    st, _ = wd.state_init(p, r0, n0, lib=lib)
    works = wd.new_works(specs, n)
    for k in (7, 1):
        wd.window(p, st, k, pw, specs, works, rho=_rho(g), lib=lib)
    assert all(x.any() for x in works) or st["nstep"].max() == 8
    for name, _ in trace.RayState.FIELDS:
        getattr(w.state, name).copy_(torch.as_tensor(st[name]))
    for t, a in zip(w.works, works):
        t.copy_(torch.as_tensor(a))
    path = str(tmp_path / "run.npz")
    w.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted([k for k, _ in trace.RayState.FIELDS] + ["work_0", "work_1", "ray_power", "which", "n_bins"])
    back = trace.WindowedDeposition.load(path, p, r0, n0, device="cpu")
    assert back.deposition == specs and back.device.type == "cpu"
    assert wl.state_bytes(back.state.numpy()) == wl.state_bytes(st)
    for t, a in zip(back.works, works):
        assert t.numpy().tobytes() == a.tobytes()
    assert back.power.numpy().tobytes() == pw.tobytes()
    # the unchanged refusal of DeviceTrace
    with pytest.raises(ValueError, match="window=... does not go with deposition"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=specs, ray_power=pw, window=4, device="cpu")


def test_binding_declares_the_entries():
    from rays_amd import hip
    for sym in ("rays_hip_trace_window_profiles_device", "rays_hip_window_profiles_kernel_name_for"):
        assert sym in hip.EXPORTED_SYMBOLS
    assert callable(hip.trace_window_profiles_device) and callable(hip.window_profiles_kernel_name)
    try:
        lib = hip.load()
    except hip.RaysHipError:
        pytest.skip("librays_hip.so is not built here")
    assert len(lib.rays_hip_trace_window_profiles_device.argtypes) == 9
    assert len(lib.rays_hip_window_profiles_kernel_name_for.argtypes) == 3
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    assert hip.window_profiles_kernel_name(p, 64, 1) == "rk4_trace_kernel<230, 2, 0, 8>"
    assert hip.window_profiles_kernel_name(p, 64, 2) == "rk4_trace_kernel<486, 2, 0, 8>"
    # the existing answers do not move
    assert hip.profiles_kernel_name(p, 64, 2) == "rk4_trace_kernel<358, 2, 0, 8>"
    assert hip.window_kernel_name(p, 64, recording=False) == "rk4_trace_kernel<166, 2, 0, 8>"
    gs, nmls, ps = load_golden("gold_slab16_damp_rk4")
    assert hip.window_profiles_kernel_name(ps, 16, 1) == hip.deposition_kernel_name(ps, 16).replace("<100,", "<228,")
    assert hip.window_profiles_kernel_name(ps, 16, 2) == ""
