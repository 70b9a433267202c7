"""CPU tier: fused deposition into BOTH axisym_toroid profiles in one trace pass (rays_hip_trace_profiles*, kernels with
kEqNoTraj | kEqDeposit | kEqDeposit2 in EQ) -- the product kernel sources in the variant that bins every accepted point
into two rows from one grid evaluation, on the host emulation; the host entry on the emulated four-device runtime; the
Python plumbing and its refusals.  Every comparison is on bit patterns; no tolerance appears anywhere."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from rays_amd.params import STOP_CODE, axisym_tables_struct, copy_params
from tests import emul_build as eb
from tests import fused_deposition_lib as fl
from tests import fused_profiles_lib as pl
from tests import summary_lib as sl
from tests.common import ROOT, load_golden
from tests.test_cpu_fused_deposition import _rho, _wave_case
from tests.test_cpu_summary_trace import _fake_torch

EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")


def _single(p, r0, n0, power, specs, rho, lib):
    return [fl.emul_fused(p, r0, n0, power, w, nb, rho=rho, lib=lib) for w, nb in specs]


# ---- 1. the fixtures on one emulated lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", pl.ORDERS, ids=["psi_rho", "rho_psi"])
@pytest.mark.parametrize("name", pl.TWO_PROFILE_FIXTURES)
def test_two_profile_kernel_source_on_host_equals_reference(name, order):
    """The six fixtures with both profiles of the reference post-processor, both binned in ONE pass: each work, profile
    and Q_sum equals dep_work[i], dep_profile[i], dep_q_sum[i], and the summaries equal the golden ones -- whichever
    order the two records are given in."""
    g, nml, p = load_golden(name)
    names = fl.profile_names(g)
    assert sorted(names) == ["Ptotal_psi", "Ptotal_rho"]
    lib = pl.emul_lib()
    sl.set_axisym_tables(g, lib)
    nb = int(g["dep_n_bins"])
    out = pl.emul_profiles(p, g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], [(w, nb) for w in order],
                           rho=_rho(g), lib=lib)
    for k, w in enumerate(order):
        fl.assert_golden_deposition(out["works"][k], out["profiles"][k], g, names.index(w), f"{name} {w}")
    fl.assert_golden_summaries(out, g, name)
    if "129" in name:   # the rho(psiN) spline of the 129 x 129 table is NaN: the whole rho profile lands in bin 1
        rho_prof = out["profiles"][order.index("Ptotal_rho")]
        assert rho_prof[0] != 0.0 and not rho_prof[1:].any()


# ---- 2. independent bin counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [(1, 320), (320, 1), (7, 100)])
def test_bin_counts_are_independent(bins):
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    lib = pl.emul_lib()
    sl.set_axisym_tables(g, lib)
    specs = [("Ptotal_psi", bins[0]), ("Ptotal_rho", bins[1])]
    r0, n0, pw, rho = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"], _rho(g)
    out = pl.emul_profiles(p, r0, n0, pw, specs, rho=rho, lib=lib)
    assert out["works"][0].shape[1] == bins[0] and out["works"][1].shape[1] == bins[1]
    assert out["works"][0].any() and out["works"][1].any()
    pl.assert_same_as_single(out, _single(p, r0, n0, pw, specs, rho, lib), str(bins))


def _rays_inside_the_absorption_layer(g, n=16):
    """No fixture ray absorbs power before its sixth point, and the binner skips a segment without absorbed power
    whatever its ends are: the grid value of POINT 1 never reaches a row.  These rays start where fixture rays were
    already being absorbed -- at the point after the first one with ray_vec(8) > 0, with that point's k -- so their
    first segment deposits, from x_prev as set at point 1."""
    rv, npt = g["dep_ray_vec_full"], g["npoints_full"]
    k0 = rv[0, 0, 3] / g["rindex_vec0_full"][0, 0]   # ray_vec(4:6) = k0 * rindex_vec
    rows = np.array([rv[i, int(np.argmax(rv[i, :npt[i], 7] > 0)) + 1] for i in range(n)])
    return rows[:, 0:3].copy(), rows[:, 3:6] / k0


def test_first_segment_starts_at_each_profiles_own_grid_value():
    """Rays launched inside the absorption layer: the first segment of every ray deposits (asserted on the emulated full
    trace), on either grid from that grid's own value at point 1.  Against two single-profile emulations."""
    from tests import emul_lib
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    r0, n0 = _rays_inside_the_absorption_layer(g)
    emul_lib.set_axisym_tables(eb.axisym_tables_of(g))
    full = emul_lib.trace(p, r0, n0)
    assert (full["npoints"] > 5).all() and (full["ray_vec"][:, 1, 7] > 0.0).all()
    lib = pl.emul_lib()
    sl.set_axisym_tables(g, lib)
    specs = [("Ptotal_psi", 7), ("Ptotal_rho", 100)]
    pw, rho = g["dep_power"][:len(r0)], _rho(g)
    out = pl.emul_profiles(p, r0, n0, pw, specs, rho=rho, lib=lib)
    sl.assert_same(out, sl.summaries_of(full), "rays inside the layer")
    pl.assert_same_as_single(out, _single(p, r0, n0, pw, specs, rho, lib), "rays inside the layer")


# ---- 3. whole emulated waves with refills ------------------------------------------------------------------------------------
def test_rk4_waves_with_refills():
    """170 damped eqdsk rays on ONE emulated wave (every lane is refilled once or twice), in index order and long-first:
    a refilled lane starts its ray's two x_prev and its q_prev afresh and writes the rows of the ray it holds.  Against
    the two single-profile wave emulations."""
    g, q, r0, n0, power = _wave_case("gold_axisym64_eqdsk_damp_rk4", 170, 80)
    lib = pl.emul_lib(wave=True)
    sl.set_axisym_tables(g, lib)
    rho = _rho(g)
    specs = [("Ptotal_psi", 100), ("Ptotal_rho", 64)]
    for stride in (0, 2):
        ref = [fl.emul_fused_waves(q, r0, n0, power, w, nb, "rk4", 1, stride, rho=rho, lib=lib) for w, nb in specs]
        assert ref[0]["npoints"][9] == 1 and not ref[0]["work"][9].any() and not ref[1]["work"][9].any()
        assert (ref[0]["stop_code"] == [v for k, v in STOP_CODE.items() if k.strip() == "total_absorption"][0]).any()
        for r in ref:
            assert len({tuple(w) for w in r["work"]}) > 150
        out = pl.emul_profiles_waves(q, r0, n0, power, specs, "rk4", 1, stride, rho=rho, lib=lib)
        pl.assert_same_as_single(out, ref, f"stride {stride}")


def test_sg_waves_with_refills():
    """The same for sg_trace_kernel on the SG wave emulator: 150 rays on one wave, nstep_max = 12."""
    g, q, r0, n0, power = _wave_case("gold_axisym64_eqdsk_damp_sg", 150, 12)
    lib = pl.emul_lib(wave=True)
    sl.set_axisym_tables(g, lib)
    rho = _rho(g)
    specs = [("Ptotal_rho", 64), ("Ptotal_psi", 50)]
    ref = [fl.emul_fused_waves(q, r0, n0, power, w, nb, "sg", 1, rho=rho, lib=lib) for w, nb in specs]
    assert ref[0]["npoints"][9] == 1 and ref[0]["npoints"].max() == 13
    for r in ref:   # more different rows than the wave has lanes: refilled lanes wrote rows of their own
        assert len({tuple(w) for w in r["work"]}) > 64
    pl.assert_same_as_single(pl.emul_profiles_waves(q, r0, n0, power, specs, "sg", 1, rho=rho, lib=lib), ref, "sg")


# ---- 4. chaining -----------------------------------------------------------------------------------------------------------
def test_both_profiles_continue_their_carried_sums():
    """Two blocks of rays chained through both profile_ins end at the fixture's profiles."""
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    lib = pl.emul_lib()
    sl.set_axisym_tables(g, lib)
    names = fl.profile_names(g)
    nb, rho = int(g["dep_n_bins"]), _rho(g)
    specs = [("Ptotal_rho", nb), ("Ptotal_psi", nb)]
    r0, n0, pw = g["rvec0_full"], g["rindex_vec0_full"], g["dep_power"]
    first = pl.emul_profiles(p, r0[:23], n0[:23], pw[:23], specs, rho=rho, lib=lib)
    second = pl.emul_profiles(p, r0[23:], n0[23:], pw[23:], specs, rho=rho, profile_in=first["profiles"], lib=lib)
    for k, (w, _) in enumerate(specs):
        i = names.index(w)
        np.testing.assert_array_equal(second["profiles"][k], g["dep_profile"][i])
        np.testing.assert_array_equal(np.concatenate([first["works"][k], second["works"][k]]), g["dep_work"][i])
    assert not np.array_equal(first["profiles"][0], first["profiles"][1])


# ---- 5. the host entry on the emulated four-device runtime, stand-alone ----------------------------------------------------
TABLE_FIELDS = ("r_grid", "z_grid", "psi_fspl", "rb_grid", "rb_fspl", "ne_grid", "ne_fspl", "te_grid", "te_fspl", "ti_grid",
                "ti_fspl")


def _case_file(path):
    """101 rays of the damped eqdsk fixture tiled, powers all different, one ray refused at its initial check; bins
    (50, 64); the expected bytes from the one-lane emulation of the two-profile kernel."""
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    q = copy_params(p)
    q.nstep_max = 60
    nray, specs = 101, [("Ptotal_psi", 50), ("Ptotal_rho", 64)]
    r0 = np.tile(g["rvec0_full"], (2, 1))[:nray].copy()
    n0 = np.tile(g["rindex_vec0_full"], (2, 1))[:nray].copy()
    n0[40] *= 3.0
    power = (1.0 + 0.01 * np.arange(nray)) / nray
    lib = pl.emul_lib()
    sl.set_axisym_tables(g, lib)
    rho = _rho(g)
    ref = pl.emul_profiles(q, r0, n0, power, specs, rho=rho, lib=lib)
    assert ref["npoints"][40] == 1 and ref["npoints"].max() == 61 and len(np.unique(ref["npoints"])) > 3
    assert all(w.any() and not w[40].any() for w in ref["works"])
    tab = eb.axisym_tables_of(g)
    t, keep = axisym_tables_struct(tab)
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    with open(path, "wb") as f:
        f.write(struct.pack("=8i", nray, q.nv, specs[0][1], specs[1][1], fl.WHICH[specs[0][0]], fl.WHICH[specs[1][0]],
                            len(z["fspl_re"]), len(bytes(q))))
        f.write(bytes(q))
        f.write(np.array([float(z["x_min"]), float(z["x_max"])]).tobytes())
        f.write(np.ascontiguousarray(z["fspl_re"], dtype=np.float64).tobytes())
        f.write(struct.pack("=6i", t.nr, t.nz, t.n_rb, t.n_ne, t.n_te, t.n_ti))
        for name in TABLE_FIELDS:
            a = np.ascontiguousarray(tab.get(name, ()), dtype=np.float64).ravel()
            f.write(struct.pack("=i", a.size))
            f.write(a.tobytes())
        f.write(struct.pack("=i", len(rho[0])))
        for a in (rho[0], rho[1], r0, n0, power):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for k in sl.KEYS:
            f.write(np.ascontiguousarray(ref[k], dtype=np.int32 if k in ("npoints", "stop_code") else np.float64).tobytes())
        for w in ref["works"]:
            f.write(np.ascontiguousarray(w, dtype=np.float64).tobytes())


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_entry_on_emulated_devices(sanitize, tmp_path):
    """rays_hip_trace_profiles with 1 to 4 devices, a ragged last block and empty blocks: summaries and both works equal
    the one-lane emulation's, each profile chained over the blocks equals the single block's ray-ordered sum; one record
    equals the single-profile entry; every named refusal; after rays_hip_finalize the emulated driver reports no live
    allocation, pinned block, stream or event.  Once plain and once as an ASan + UBSan executable with its own main
    (leak detection on)."""
    subprocess.check_call(["make", "-s", "-j", str(min(4, os.cpu_count() or 1)), "-f", "Makefile.profiles", "profiles"] +
                          (["SAN=1"] if sanitize else []), cwd=EMUL_DIR)
    exe = os.path.join(EMUL_DIR, "build_capi_san/emul_profiles_capi_san" if sanitize else "build_capi/emul_profiles_capi")
    case = str(tmp_path / "profiles_case.bin")
    _case_file(case)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS", "LD_PRELOAD")}
    env.update(RAYS_EMUL_DEVICES="4")
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, case], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "profiles capi ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 6. Python plumbing and the refusals ------------------------------------------------------------------------------------
def test_python_layer_list_spelling(monkeypatch):
    """DeviceTrace / RaysRun with deposition=[(which, n_bins), ...] and "all": the lists they build, the refusals by name,
    and no tensor with an nstep_max + 1 axis."""
    from rays_amd import hip, trace
    allocated = []
    monkeypatch.setitem(sys.modules, "torch", _fake_torch(allocated))
    sys.modules["torch"].is_tensor = lambda x: False
    monkeypatch.setattr(hip, "check_params", lambda q: None)
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    r0, n0 = g["rvec0"], g["rindex_vec0"]
    n, npt = len(r0), p.nstep_max + 1
    pw = np.ones(n)
    dt = trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[("Ptotal_rho", 7), ("Ptotal_psi", 100)], ray_power=pw)
    assert dt.ray_vec is None and dt.residual is None and dt.deposition == [("Ptotal_rho", 7), ("Ptotal_psi", 100)]
    assert [w.shape for w in dt.works] == [(7, n), (100, n)] and [q.shape for q in dt.profiles] == [(7,), (100,)]
    assert dt.start_ray_vec.shape == (n, p.nv) and dt.work is None and dt.profile is None
    assert allocated and all(npt not in s for s in allocated), allocated
    one = trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[("Ptotal_psi", 5)], ray_power=pw)
    assert one.deposition == [("Ptotal_psi", 5)] and len(one.works) == 1
    monkeypatch.setattr(hip, "deposition_profile_set", lambda q: ("Ptotal_psi", "Ptotal_rho"))
    al = trace.DeviceTrace(p, r0, n0, trajectories=False, deposition="all", n_bins=100, ray_power=pw)
    assert al.deposition == [("Ptotal_psi", 100), ("Ptotal_rho", 100)]
    # the tuple spelling keeps its meaning
    old = trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_psi", 9, pw))
    assert old.deposition == ("Ptotal_psi", 9) and old.work.shape == (9, n) and old.works is None
    lst = [("Ptotal_psi", 5), ("Ptotal_rho", 5)]
    with pytest.raises(ValueError, match="trajectories=False"):
        trace.DeviceTrace(p, r0, n0, deposition=lst, ray_power=pw)
    with pytest.raises(ValueError, match="needs ray_power="):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=lst)
    with pytest.raises(ValueError, match="ray_power must hold one weight per ray"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=lst, ray_power=pw[:-1])
    with pytest.raises(ValueError, match="do not mix"):   # the tuple spelling's power inside a list
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[("Ptotal_psi", 5, pw)], ray_power=pw)
    with pytest.raises(ValueError, match="tuple spelling carries its power"):   # the list spelling's power beside a tuple
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=("Ptotal_psi", 5, pw), ray_power=pw)
    with pytest.raises(ValueError, match="twice"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[("Ptotal_psi", 5), ("Ptotal_psi", 6)], ray_power=pw)
    with pytest.raises(ValueError, match=r"takes 1\.\.2 profiles"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[], ray_power=pw)
    with pytest.raises(ValueError, match="known are"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[("Ptotal_y", 5)], ray_power=pw)
    with pytest.raises(ValueError, match="'Ptotal_x' does not exist for this equilib_model"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=[("Ptotal_psi", 5), ("Ptotal_x", 5)], ray_power=pw)
    with pytest.raises(ValueError, match='needs n_bins=n'):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition="all", ray_power=pw)
    with pytest.raises(ValueError, match="one entry"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=lst, ray_power=pw, profile_in=[None])
    with pytest.raises(ValueError, match="window=... does not go with deposition"):
        trace.DeviceTrace(p, r0, n0, trajectories=False, deposition=lst, ray_power=pw, window=4)
    # a slab has one profile: a list of one is fine, two are refused by name
    gs, nmls, ps = load_golden("gold_slab16_damp_rk4")
    ns = len(gs["rvec0"])
    slab = trace.DeviceTrace(ps, gs["rvec0"], gs["rindex_vec0"], trajectories=False, deposition=[("Ptotal_x", 11)],
                             ray_power=np.ones(ns))
    assert slab.deposition == [("Ptotal_x", 11)] and slab.works[0].shape == (11, ns)
    with pytest.raises(ValueError, match="'Ptotal_psi' does not exist for this equilib_model"):
        trace.DeviceTrace(ps, gs["rvec0"], gs["rindex_vec0"], trajectories=False,
                          deposition=[("Ptotal_x", 11), ("Ptotal_psi", 11)], ray_power=np.ones(ns))
    # RaysRun: the powers are the launcher's
    with pytest.raises(ValueError, match="power weights"):
        trace.RaysRun(p, r0, n0).trace_rays(trajectories=False, deposition=lst)
    run = trace.RaysRun(p, r0, n0, ray_pwr_wt=pw)
    with pytest.raises(ValueError, match="trajectories=False"):
        run.trace_rays(deposition=lst)
    with pytest.raises(ValueError, match="do not mix"):
        run.trace_rays(trajectories=False, deposition=[("Ptotal_psi", 5, pw)])
    with pytest.raises(ValueError, match='goes with deposition="all" only'):
        run.trace_rays(trajectories=False, deposition=lst, n_bins=5)
    called = {}

    def fake_host(params, rv, nv_, power, specs, ngpu=0, want_work=True):
        called["specs"] = specs
        zero = dict(npoints=np.zeros(n, dtype=np.int32), stop_code=np.zeros(n, dtype=np.int32),
                    start_ray_vec=np.zeros((n, p.nv)), end_ray_vec=np.zeros((n, p.nv)), end_residuals=np.zeros(n),
                    max_residuals=np.zeros(n), elapsed_s=0.0)
        zero["works"] = [None for _ in specs]
        zero["profiles"] = [np.arange(float(nb)) for _, nb in specs]
        return zero
    monkeypatch.setattr(hip, "trace_profiles_host", fake_host)
    recs = run.trace_rays(trajectories=False, deposition="all", n_bins=4)
    assert called["specs"] == [("Ptotal_psi", 4), ("Ptotal_rho", 4)] and len(recs) == 2
    assert recs[0].summaries is recs[1].summaries and [r.profile_name for r in recs] == ["Ptotal_psi", "Ptotal_rho"]
    assert recs[1].profile_record["grid_name"] == "rho" and recs[1].Q_sum == 6.0


def test_binding_declares_the_entries():
    from rays_amd import hip
    for sym in ("rays_hip_trace_profiles_device", "rays_hip_trace_profiles", "rays_hip_profiles_kernel_name_for",
                "rays_hip_deposition_profile_set"):
        assert sym in hip.EXPORTED_SYMBOLS
    assert [f[0] for f in hip.DepProfileStruct._fields_] == ["which", "n_bins", "work", "profile_in", "profile"]
    import ctypes
    assert ctypes.sizeof(hip.DepProfileStruct) == 32
    try:
        lib = hip.load()
    except hip.RaysHipError:
        pytest.skip("librays_hip.so is not built here")
    assert len(lib.rays_hip_trace_profiles_device.argtypes) == 14 and len(lib.rays_hip_trace_profiles.argtypes) == 14
    assert len(lib.rays_hip_profiles_kernel_name_for.argtypes) == 3 and len(lib.rays_hip_deposition_profile_set.argtypes) == 2
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    assert hip.profiles_kernel_name(p, 64, 1) == "rk4_trace_kernel<102, 2, 0, 8>"
    assert hip.profiles_kernel_name(p, 64, 2) == "rk4_trace_kernel<358, 2, 0, 8>"
    for name in ("gold_slab16_damp_rk4", "gold_solovev64_4spec_rk4_num"):
        gs, nmls, ps = load_golden(name)
        assert hip.profiles_kernel_name(ps, 16, 2) == ""
    gs, nmls, ps = load_golden("gold_slab16_damp_rk4")
    assert hip.deposition_profile_set(ps) == ("Ptotal_x",)


# ---- 7. one-token changes to the new device code -------------------------------------------------------------------------------
MUTATIONS = {
    "x_prev_of_b_from_a": ("rays_deposition.hpp", "  xb_prev = xb;  // (its own", "  xb_prev = xa;  // (its own"),
    "both_rows_into_a": ("rays_deposition.hpp", "deposit_segment(T.prof[1].work + ray,", "deposit_segment(T.prof[0].work + ray,"),
    "bin_count_of_b_from_a": ("rays_deposition.hpp", "(long long)nray, T.prof[1].n_bins,", "(long long)nray, T.prof[0].n_bins,"),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_one_token_changes_are_caught(mutation, tmp_path):
    """Three one-token changes to the new device code, each built into an emulation library of its
    own: (a) the second profile's x_prev set from the first profile's grid value at point 1; (b) both profiles stored into the first row; (c) the second bin count taken from the first.
    Each has to break a comparison of test 2: (b) and (c) on the fixture's own rays at 7 + 100 bins, (a) on the rays
    launched inside the absorption layer -- on the fixtures' own launch points no first segment deposits, and (a) is
    invisible (asserted here: it is NOT caught there)."""
    file, old, new = MUTATIONS[mutation]
    out_lib = str(tmp_path / "librays_emul_profiles_mut.so")
    eb.build("emul_fused_profiles.cpp", out_lib, pl.BASE_DEFS,
             directory=eb.mutated_tree(str(tmp_path / "tree"), file, old, new))
    lib = eb.load(out_lib)
    pl.declare(lib, False)
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    sl.set_axisym_tables(g, lib)
    # (bin counts under which the changed code stays inside the rows it was given: (b) writes the second profile's
    # bins into the first profile's rows, (c) bins the second profile with the first one's count)
    specs = [("Ptotal_psi", 100), ("Ptotal_rho", 7)] if mutation == "both_rows_into_a" else [("Ptotal_psi", 7), ("Ptotal_rho", 100)]
    good = pl.emul_lib()
    sl.set_axisym_tables(g, good)
    rho = _rho(g)

    def caught(r0, n0, pw):
        out = pl.emul_profiles(p, r0, n0, pw, specs, rho=rho, lib=lib)
        try:
            pl.assert_same_as_single(out, _single(p, r0, n0, pw, specs, rho, good), mutation)
        except AssertionError:
            return True
        return False
    on_fixture_rays = caught(g["rvec0_full"][:8], g["rindex_vec0_full"][:8], g["dep_power"][:8])
    if mutation == "x_prev_of_b_from_a":
        assert not on_fixture_rays
        r0, n0 = _rays_inside_the_absorption_layer(g, 8)
        assert caught(r0, n0, g["dep_power"][:8])
    else:
        assert on_fixture_rays
