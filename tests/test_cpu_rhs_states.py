"""CPU tier: the right-hand side at THRESHOLD states (tests/rhs_state_cases.py: box bounds, the plasma edge, the damping
argument beside +-5 and beside the Z-function's knots, check_save's limits, RK4 stages that refuse) against what the
reference's own routines make of the same states (tests/golden/rhs_state_cases.npz, oracle/ref_states_driver.f90).
Every comparison is bit for bit with NaN equal to NaN: the oracle (oracle_lib.probe / step), the device headers
compiled for the host (tests/hip_emul/emul_probe.cpp) and the emulated ray diagnostics.  The controls build the emulated
probe from a copy of rays_device_arith.inc with ONE token changed: each must fail in the class that owns the threshold."""
import numpy as np
import pytest

from tests import diag_expect as dx, emul_build as eb, oracle_lib, probe_emul_lib as pe, rhs_state_cases as rc
from tests.common import load_golden

DAMPED = [c for c in rc.CASES if load_golden(c)[2].damping_model]
NEW_BOX = "gold_axisym16_eqdsk49x65_tspline_damp_rk4"      # (the box whose grid spacings are no powers of two)


# the floors of the axisym_toroid profiles: (column of the eq record, the floored value); the splined temperatures of the
# configurations stay above T_scrape_off up to the plasma edge, so Ti has no state and Te only the parabolic ones
FLOORS = {"C.dens_floor": lambda p: (28, p.n0s[0] * p.axisym.d_scrape_off),
          "C.Te_floor": lambda p: (32, p.t0s[0] * p.axisym.T_scrape_off),
          "C.Ti_floor": lambda p: (44, p.t0s[1] * p.axisym.T_scrape_off)}


def _case(case, classes="A-H"):
    g, nml, p = load_golden(case)
    return g, p, eb.axisym_tables_of(g), rc.load_fixture(case, classes)


# ---- the fixture itself ----
def test_the_fixture_is_the_generators_states():
    """the committed states are what tests/rhs_state_cases.py generates today (labels and sides included), at most 2000"""
    total = 0
    for case in rc.CASES:
        v, s, label, side = rc.states(case)
        f = rc.load_fixture(case)
        dx.assert_bits(f["v"], v, case)
        dx.assert_bits(f["s"], s, case)
        assert list(f["label"]) == list(label) and list(f["side"]) == list(side), case
        assert np.array_equal(f["geom"], rc.reference_undefined(case, v)), case
        total += len(v)
    assert total <= rc.MAX_STATES


def test_coverage_of_the_thresholds():
    """From the fixture alone: every label that has a threshold holds states on both of its sides; where the threshold
    decides a flag the reference's flag differs between the sides; B and C are value-compared for at least a third of
    their states, and no more than 40 % of all states are flags-only."""
    n = flags_only = 0
    per_class = {}
    for case in rc.CASES:
        f = rc.load_fixture(case)
        values, pr, st = f["ok"]["values"], f["probe"], f["step"]
        n += len(values)
        flags_only += int((~values).sum())
        assert set(f["cls"]) >= set("ABDEGH"), case
        assert (f["cls"] == "A").sum() == rc.N_INTERIOR and values[f["cls"] == "A"].all(), case
        for c in "BC":
            rows = f["cls"] == c
            a, b = per_class.get(c, (0, 0))
            per_class[c] = (a + int(rows.sum()), b + int((rows & values).sum()))
        for label in sorted(set(f["label"])):
            rows = f["label"] == label
            sides = set(f["side"][rows].tolist())
            if sides == {0}:
                continue
            assert sides >= {-1, 1}, f"{case}: {label} has states on one side only"
            lo, hi = rows & (f["side"] < 0), rows & (f["side"] > 0)
            cls = label[0]
            if cls == "B" and "m" in label:      # a bound: refused beyond it, not refused on and inside it
                ok = f["ok"]["flags"]
                assert (f["eq_code"][hi & ok] != 0).all() and (hi & ok).any(), (case, label)
                assert not np.isin(f["eq_code"][lo & ok], rc.BOX_FLAGS).any(), (case, label)
            if label in ("C.psi_limit", "C.neg_temp", "C.neg_dens"):
                assert (f["eq_code"][hi] != 0).all() and (f["eq_code"][lo] == 0).all(), (case, label)
            if label in FLOORS:                  # value-compared on both sides: at the floor on one, above it on the other
                col, floor = FLOORS[label](load_golden(case)[2])
                assert values[lo].all() and values[hi].all(), (case, label)
                assert (pr["eq"][hi, col] == floor).all() and (pr["eq"][lo, col] > floor).all(), (case, label)
                assert (pr["eq"][hi, col + 1:col + 4] == 0).all() and pr["eq"][lo, col + 1:col + 4].any(axis=1).all(), (case, label)
            if label in ("F.xi5", "F.xi-5"):     # |xi| > 5: no damping
                assert (pr["dvds"][hi, 7] == 0).all() if label == "F.xi5" else (pr["dvds"][lo, 7] == 0).all(), (case, label)
                assert (pr["dvds"][lo, 7] != 0).all() if label == "F.xi5" else (pr["dvds"][hi, 7] != 0).all(), (case, label)
            if label == "F.damping_limit":
                assert (f["cs_code"][hi] == 42).all() and (f["cs_code"][lo] != 42).all(), (case, label)
            if label == "G.resid_limit":
                assert (f["cs_code"][hi] == 40).all() and (f["cs_code"][lo] == 0).all(), (case, label)
            if label == "H.step":                # a stage refuses | the step is taken
                assert (st["step_stop"][hi] == 1).any() and (st["step_stop"][lo] == 0).all(), (case, label)
    for c, (total, compared) in per_class.items():
        assert 3 * compared >= total, f"class {c}: {compared} of {total} states are value-compared"
    assert flags_only <= 0.4 * n, f"{flags_only} of {n} states are flags-only"
    assert {label for c in rc.CASES for label in rc.load_fixture(c)["label"] if label in FLOORS} == set(FLOORS) - {"C.Ti_floor"}
    for case in DAMPED:        # two states beside each knot: 64 knots where k_par is a component of the state, 32 elsewhere
        assert (rc.load_fixture(case)["label"] == "F.knot").sum() >= 2 * (64 if case == "gold_slab16_damp_rk4" else 32), case


@pytest.mark.parametrize("case", rc.CASES)
def test_interior_states_reproduce_the_trajectory_fixture(case):
    """Class A is the anchor: at the fixture's own probed points the new driver's record is the old driver's, and one
    reference step from a recorded point is the next recorded point and its residual."""
    g, p, tab, f = _case(case)
    pr, st = f["probe"], f["step"]
    if (f["label"] == "A.probe").any():
        old = {x["v"].tobytes(): x for x in g["probes"]}
        for i in np.flatnonzero(f["label"] == "A.probe"):
            rec = old[f["v"][i].tobytes()]
            for key in ("eq", "cold", "num", "dvds", "resid"):
                dx.assert_bits(pr[key][i], rec[key], f"{case} state {i} {key}")
    else:
        nxt = {}
        for r, n in enumerate(g["npoints"]):
            for k in range(int(n) - 1):
                nxt[g["ray_vec"][r, k].tobytes()] = (g["ray_vec"][r, k + 1], g["residual"][r, k + 1])
        rows = np.flatnonzero(f["label"] == "A.point")
        assert len(rows) == rc.N_INTERIOR
        for i in rows:
            v1, resid = nxt[f["v"][i].tobytes()]
            assert st["step_stop"][i] == 0 and st["cs1_stop"][i] == 0
            dx.assert_bits(st["v1"][i], v1, f"{case} state {i} v1")
            dx.assert_bits(st["resid1"][i], resid, f"{case} state {i} resid")


# ---- the oracle ----
@pytest.mark.parametrize("case", rc.CASES)
def test_oracle_equals_the_reference_at_every_state(case):
    g, p, tab, f = _case(case)
    got = [oracle_lib.probe(p, v) for v in f["v"]]
    got = {k: np.array([o[k] for o in got]) for k in ("eq", "cold", "num", "dvds", "resid", "codes")}
    rc.compare_probe(f, got, f"{case}: oracle_lib.probe")
    v1, resid, code, stopped = oracle_lib.step(p, f["v"], f["s"])
    rc.compare_step(f, v1, resid, np.where(stopped, code, 0), f"{case}: oracle_lib.step")


# ---- the device headers on the host ----
def _compare_emulated(case, lib_=None, only=None, classes="A-H"):
    g, p, tab, f = _case(case, classes)
    f = dict(f, only=None if only is None else np.isin(f["cls"], list(only)))
    got = pe.probe(p, f["v"], tab, lib_)
    rc.compare_probe(f, got, f"{case}: emulated probe", eq_columns=pe.eq_columns(p))
    v1, resid, codes = pe.step(p, f["v"], f["s"], tab, lib_)
    code = np.where(codes[:, 0] != 0, codes[:, 0], np.where(codes[:, 2] != 0, codes[:, 1], 0))
    rc.compare_step(f, v1, resid, code, f"{case}: emulated step")


@pytest.mark.parametrize("case", rc.CASES)
def test_device_source_on_host_equals_the_reference_at_every_state(case):
    _compare_emulated(case)


@pytest.mark.parametrize("case", rc.CASES)
def test_trace_kernel_step_on_host_equals_the_reference_at_every_state(case):
    """rays_hip_ode_step_device's launch through the RK4 trace kernel's own state machine on the host (emul_lib.ode_step):
    the stop code at every state -- a state whose own check_save sets stop_ode never starts --, v1 and the residual of
    every step taken and kept."""
    from tests import emul_lib
    g, p, tab, f = _case(case)
    v1, resid, code = emul_lib.ode_step(p, f["v"], f["s"])
    want_code, code_rows, v1_rows, zero_rows = rc.expected_ode_step(f)
    what = f"{case}: emul_lib.ode_step"
    rc._check(f, what, "the stop code", code, want_code, code_rows)
    kept = v1_rows & (want_code == 0) & code_rows
    rc._check(f, what, "v1", v1, f["step"]["v1"], kept)
    rc._check(f, what, "the residual at v1", resid, f["step"]["resid1"], kept & f["ok"]["step_cs"])
    h = (f["cls"] == "H") & code_rows
    if (want_code[h] == 0).any():      # (one case's class H lies off its rays: no trace starts there)
        assert (code[h] != 0).any() and (code[h] == 0).any()


@pytest.mark.parametrize("case", rc.CASES)
def test_emulated_diagnostics_at_the_states(case):
    """rays_emul_ray_diagnostics on arrays whose points are the states, one "ray" per class: all nineteen fields equal
    diag_expect.expected_at_points, at the states where the reference defines values (the expectation needs an
    equilibrium inside the box)."""
    g, p, tab, f = _case(case)
    dx.emul_set_tables(tab)
    ray_vec, residual, npoints, rows = rc.class_rays(f)
    got, bad = dx.emul_diagnostics(p, ray_vec, residual, npoints)
    for r, idx in enumerate(rows):
        want = dx.expected_at_points(p, tab, f["v"][idx], f["probe"]["resid"][idx])
        for name in dx.FIELDS:
            dx.assert_bits(got[name][r, :len(idx)], want[name], f"{case} class {f['cls'][idx[0]]} {name}")
        for k, i in enumerate(idx):      # and straight from the reference's eq record, for the fields it determines
            for name, val in dx.from_eq_record(p, f["v"][i], f["probe"]["eq"][i], f["probe"]["resid"][i]).items():
                dx.assert_bits(got[name][r, k], val, f"{case} state {i} {name} (reference eq record)")


# ---- controls: one token of rays_device_arith.inc changed; the state comparison must fail in the owning class ----
# Two changes no state can show, because no output of the reference depends on them (DESIGN.md has the reasoning):
#   * `if (R3 == 0.) return 0.;` removed: with k3 = 0 the argument xi = (w + wc) / (k3 vth) is +-inf and the next line,
#     `fabs(xi) > 5.`, returns the same 0 (xi is NaN only at w + wc = 0 exactly, |gamma_e| = 1, where dD/dw and with it
#     the whole row are NaN with and without the guard);
#   * `k3 > 0.` -> `k3 >= 0.`: the two differ at k3 = 0 alone, which the guard above has already answered.
# The branch itself is held by `k3 > 0.` -> `k3 < 0.`.
# A third, of the bilinear model's cell index (class K): `1 + (int)q` -> `(int)ceil(q)`.  The two differ where the quotient q
# is a whole number -- on a grid line, or a double below one where q rounds up to it -- and there they name neighbouring
# cells with the fraction 0 in one and 1 (or a negative fraction of 1e-16) in the other: the bilinear form is continuous
# across the line, three of its four products are then exact zeros, and the value has the same bits either way.  What K
# holds is the index itself (`1 +` -> `2 +`), which every class of that configuration sees as well.
MUTATIONS = {
    "slab box < -> <=": ("gold_slab16_damp_rk4", "if (x < P.xmin || x > P.xmax) err", "if (x <= P.xmin || x > P.xmax) err", "B"),
    "axisym Tiny margin dropped": ("gold_axisym64_eqdsk129_tspline_damp_rk4", "r > P.a_box_rmax + Tiny", "r > P.a_box_rmax", "B"),
    "psiN <= 1.0 -> < 1.0": ("gold_axisym64_eqdsk129_tspline_damp_rk4", "if (psiN <= 1.0) {\n          Te = te", "if (psiN < 1.0) {\n          Te = te", "C"),
    "spline density floor dropped": ("gold_axisym64_eqdsk129_tspline_damp_rk4", "      if (dens < P.a_d_scrape) {", "      if (dens < 0.) {", "C"),
    "parabolic floor dropped": ("gold_axisym64_solmag_damp_rk4", "  if (f < f_min) {", "  if (f < 0.) {", "C"),
    "psiN > limit -> >=": ("gold_axisym64_solmag_damp_rk4", "psiN > P.a_psi_limit", "psiN >= P.a_psi_limit", "C"),
    "k3 > 0. -> k3 < 0.": ("gold_solovev64_damp_rk4", "  if (k3 > 0.) {\n    zf = zfun_real_arg_spline(P, xi);", "  if (k3 < 0.) {\n    zf = zfun_real_arg_spline(P, xi);", "F"),
    "fabs(xi) > 5. -> >= 5.": ("gold_slab16_damp_rk4", "if (fabs(xi) > 5.) return 0.;", "if (fabs(xi) >= 5.) return 0.;", "F"),
    "(float) of delta_im removed": ("gold_slab16_damp_rk4", "const float delta_im = (float)divdc3(num, den).im;", "const double delta_im = divdc3(num, den).im;", "F"),
    "v[7] > limit -> >=": ("gold_solovev64_damp_rk4", "] > P.total_damping_limit) {", "] >= P.total_damping_limit) {", "F"),
    # the cell search of the table lookups (class K: tests/golden/eq_knot_states.npz)
    "spl_settle: arms exchanged": (NEW_BOX, "i = z < lo ? i - 1 : i + 1;", "i = z < lo ? i + 1 : i - 1;", "K"),
    "spl_settle: z > hi -> >=": (NEW_BOX, "if (RAYS_RARE(z < lo || z > hi)) {", "if (RAYS_RARE(z < lo || z >= hi)) {", "K"),
    "spl2_fpp: offx || offy -> &&": (NEW_BOX, "if (RAYS_RARE(offx || offy)) {", "if (RAYS_RARE(offx && offy)) {", "K"),
    "spl1_ax: lo not fetched again": ("gold_axisym64_eqdsk_tspline_rk4_num", "  if (spl_settle(n, z, lo, hi, i)) {\n    lo = grid[i - 1];\n    c = fspl", "  if (spl_settle(n, z, lo, hi, i)) {\n    c = fspl", "K"),
    "eqlin: cell index one higher": ("gold_axisym64_eqlin_damp_rk4", "const int j = 1 + (int)div(Z - z1, Rhz);", "const int j = 2 + (int)div(Z - z1, Rhz);", "K"),
    "spl_guess: product with the stored reciprocal": (NEW_BOX, "div(nxm * (z - x1), const_recip(xn - x1, ax[2]))", "((nxm * (z - x1)) * ax[2])", "K"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_one_changed_token_fails_in_the_class_that_owns_the_threshold(name, tmp_path):
    case, old, new, classes = MUTATIONS[name]
    lib_ = pe.mutated_lib(tmp_path, old, new)
    with pytest.raises(AssertionError, match=rf"\(class [{classes}],") as e:
        _compare_emulated(case, lib_, only=classes, classes="K" if classes == "K" else "A-H")      # the states of the owning class ALONE have to show it
    print(f"{name}: {e.value}")


def test_what_the_trajectory_fixtures_make_of_a_changed_threshold(tmp_path):
    """Evidence, not a requirement (nothing is asserted on the outcome): the trajectory-based emulation test
    (tests/test_cpu_kernel_emul.py: test_kernel_source_on_host_equals_reference) run against the trace kernels built from
    the copy with the slab box's `<` changed to `<=`.  When this test was written all 38 trajectory fixtures let that
    change through -- as they did the dropped 1e-13 margin, `psiN <= 1.0` -> `<`, `psiN > limit` -> `>=`,
    `fabs(xi) > 5.` -> `>=` and `v[7] > limit` -> `>=`; they caught the swapped Z-function branch and the removed
    (float) truncation."""
    from tests import emul_lib
    from tests.common import GOLDEN_CASES, assert_matches_golden
    case, old, new, classes = MUTATIONS["slab box < -> <="]
    out = str(tmp_path / "librays_emul_mutated.so")
    eb.build("emul_trace.cpp", out, directory=eb.mutated_tree(str(tmp_path / "tree"), "rays_device_arith.inc", old, new))
    saved, caught = emul_lib._lib, []
    emul_lib._lib = emul_lib._load(out)
    try:
        for name in [c for c in GOLDEN_CASES if "slab" in c]:
            g, nml, p = load_golden(name)
            try:
                assert_matches_golden(emul_lib.trace(p, g["rvec0"], g["rindex_vec0"]), g, p, exact=True)
            except AssertionError:
                caught.append(name)
    finally:
        emul_lib._lib = saved
    print("slab box `<` -> `<=`: " + (f"caught by {caught}" if caught else "let through by every slab trajectory fixture"))
