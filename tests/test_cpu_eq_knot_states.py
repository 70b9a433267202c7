"""CPU tier: the equilibrium's table lookups ON AND BESIDE THEIR KNOTS (class K of tests/rhs_state_cases.py: grid nodes of the
R-Z tables, their neighbouring doubles, psiN on and beside the knots of the profile splines, the truncating cell index of
the bilinear model) against what the reference's own routines make of the same states (tests/golden/eq_knot_states.npz,
oracle/ref_states_driver.f90).  A trajectory reaches such a point with probability zero, and only there do the cell
search's rare branches run: the estimate one cell off, the node that ends in the cell below it.  The comparisons are those
of tests/test_cpu_rhs_states.py, bit for bit with NaN equal to NaN."""
import collections

import numpy as np
import pytest

from tests import diag_expect as dx, emul_lib, oracle_lib, probe_emul_lib as pe, rhs_state_cases as rc
from tests.common import load_golden
from tests.test_cpu_rhs_states import _case, _compare_emulated

NEW = "gold_axisym16_eqdsk49x65_tspline_damp_rk4"
# what the restatement of the reference's search (rc.cell_estimate) makes of the states of each label's coordinate on its
# grid: (estimate exact, settled one cell down, settled one cell up, states ON a node that ends in the cell below it).
# From the tables of the reference alone; a change of tables or of the generator that empties a kind shows here.
#   K.psi_knot.*: the same of psiN on the profile's grid;
#   K.corner: (R estimate off alone, Z estimate off alone, both off);
#   lin_cell.Z / .R (the bilinear model, over K.z_node, K.r_node and K.lin_cell together): what the TRUNCATING index of
#   GetPsi makes of the states -- (the cell the point lies in, the cell below, the cell above, 0); this is the search that
#   case performs in R and Z, its K.z_node / K.r_node tuples only describe where the states lie.
KINDS = {
    "gold_axisym64_eqdsk129_tspline_damp_rk4": {"K.z_node": (223, 87, 10, 6), "K.r_node": (20, 0, 0, 0), "K.corner": (0, 6, 0),
                                                "K.psi_knot.ne": (60, 5, 0, 0), "K.psi_knot.te": (46, 3, 0, 0)},
    "gold_axisym64_eqdsk_tspline_rk4_num": {"K.z_node": (124, 45, 6, 3), "K.r_node": (20, 0, 0, 0), "K.corner": (0, 6, 0),
                                            "K.psi_knot.te": (46, 3, 0, 0)},
    "gold_axisym64_eqlin_damp_rk4": {"K.z_node": (124, 45, 6, 3), "K.r_node": (20, 0, 0, 0), "K.corner": (0, 6, 0),
                                     "K.psi_knot.ne": (60, 5, 0, 0), "lin_cell.Z": (131, 0, 74, 0), "lin_cell.R": (205, 0, 0, 0)},
    NEW: {"K.z_node": (122, 48, 5, 3), "K.r_node": (122, 8, 0, 14), "K.corner": (4, 4, 2),
          "K.psi_knot.ne": (77, 9, 0, 0), "K.psi_knot.te": (67, 5, 0, 0)},
}
# the bars of the issue: value-compared K.z_node states on lower-cell nodes, and with the estimate off
Z_BARS = {"gold_axisym64_eqdsk129_tspline_damp_rk4": (5, 40), "gold_axisym64_eqdsk_tspline_rk4_num": (3, 20),
          "gold_axisym64_eqlin_damp_rk4": (3, 20), NEW: (3, 20)}


def _tables(case):
    g = load_golden(case)[0]
    return {k[4:]: g[k] for k in g.files if k.startswith("axi_") and g[k].ndim}


def _kinds(grid, xs, cell=rc.cell_estimate):
    kinds = [rc.knot_kind(grid, x, cell) for x in xs]
    c = collections.Counter(k for k, _ in kinds)
    return np.array([k != "exact" for k, _ in kinds]), np.array([low for _, low in kinds]), \
        (c["exact"], c["down"], c["up"], sum(low for _, low in kinds))


def _R(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])


def test_the_fixture_is_the_generators_states():
    total = 0
    for case in rc.K_CASES:
        v, s, label, side = rc.knot_states(case)
        f = rc.load_fixture(case, "K")
        dx.assert_bits(f["v"], v, case)
        dx.assert_bits(f["s"], s, case)
        assert list(f["label"]) == list(label) and list(f["side"]) == list(side), case
        assert np.array_equal(f["geom"], rc.reference_undefined(case, v)), case
        assert set(f["cls"]) == {"K"}
        total += len(v)
    assert total <= rc.MAX_KNOT_STATES
    assert "gold_axisym64_solmag_damp_rk4" not in rc.K_CASES and not any(
        a.size for a in _tables("gold_axisym64_solmag_damp_rk4").values())          # (no table: no knots)


def test_coverage_of_the_knots():
    """From the fixture and the numpy restatement of the reference's search alone."""
    n = compared = 0
    for case in rc.K_CASES:
        f, tab = rc.load_fixture(case, "K"), _tables(case)
        values, v, label = f["ok"]["values"], f["v"], f["label"]
        n += len(values)
        compared += int(values.sum())
        # RBphi(R) is tabulated on the R grid itself: the K.r_node states are its knots too
        if "rb_grid" in tab:
            assert np.array_equal(tab["rb_grid"], tab["r_grid"]) and not (label == "K.rb_node").any(), case
        # Te(psi) and Ti(psi): the reference builds both on ONE grid (temperature_spline_interp_m.f90:95-107)
        if "ti_grid" in tab:
            assert np.array_equal(tab["ti_grid"], tab["te_grid"]) and not (label == "K.psi_knot.ti").any(), case
        for lab, grid, x in (("K.z_node", tab["z_grid"], v[:, 2]), ("K.r_node", tab["r_grid"], _R(v))):
            rows = label == lab
            off, low, counts = _kinds(grid, x[rows])
            print(f"{case}: {lab}: exact / down / up / node in the lower cell = {counts}; value-compared {int(values[rows].sum())} of {int(rows.sum())}")
            assert counts == KINDS[case][lab], (case, lab, counts)
            assert set(f["side"][rows].tolist()) == {-1, 0, 1}
            if lab == "K.z_node":
                assert (low & values[rows]).sum() >= Z_BARS[case][0] and (off & values[rows]).sum() >= Z_BARS[case][1], case
            if lab == "K.r_node" and case == NEW:
                assert (low & values[rows]).sum() >= 4 and (off & values[rows]).sum() >= 2
        # corners: what the estimate does in R and in Z at once
        rows = label == "K.corner"
        offx = _kinds(tab["r_grid"], _R(v)[rows])[0]
        offy = _kinds(tab["z_grid"], v[rows, 2])[0]
        print(f"{case}: K.corner: offx only {int((offx & ~offy).sum())}, offy only {int((~offx & offy).sum())}, both {int((offx & offy).sum())}")
        corner = (int((offx & ~offy).sum()), int((~offx & offy).sum()), int((offx & offy).sum()))
        assert values[rows].all() and corner == KINDS[case]["K.corner"] and corner[1] >= 2, (case, corner)
        if case == NEW:           # (every other R grid has spacing 2**-6 or 2**-7: each quotient is exact)
            assert corner[0] >= 2 and corner[2] >= 2
        else:
            assert not offx.any()
        # the profile knots: psiN of the states, as the host restatement has it, on each profile's own grid
        for prof in ("ne", "te"):
            rows = label == f"K.psi_knot.{prof}"
            if prof + "_grid" not in tab:
                assert not rows.any() and f"K.psi_knot.{prof}" not in KINDS[case]
                continue
            grid = tab[prof + "_grid"]
            psi = _psi(case, v[rows])
            off, low, counts = _kinds(grid, psi)
            cells = {rc.cell_estimate(grid, x)[1] for x in psi}
            print(f"{case}: K.psi_knot.{prof}: exact / down / up / knot in the lower cell = {counts}; cells {sorted(cells)}")
            assert values[rows].all(), (case, prof)
            assert counts == KINDS[case][f"K.psi_knot.{prof}"], (case, prof, counts)
            assert cells == set(range(1, len(grid))), (case, prof)          # every cell, the last one below psiN = 1 included
            for k in range(1, len(grid) - 1):                               # every interior knot from both sides
                near = np.abs(psi - grid[k]) < 1e-12
                assert (psi[near] < grid[k]).any() and (psi[near] >= grid[k]).any(), (case, prof, k)
            if prof == "ne":
                assert off.sum() >= 4, (case, counts)
        if load_golden(case)[2].axisym.magnetics_model == 2:      # the truncating index of GetPsi
            rows = np.isin(label, ["K.z_node", "K.r_node", "K.lin_cell"])
            for key, grid, x in (("lin_cell.Z", tab["z_grid"], v[:, 2]), ("lin_cell.R", tab["r_grid"], _R(v))):
                off, low, counts = _kinds(grid, x[rows], rc.lin_cell)
                print(f"{case}: GetPsi's index in {key[-1]}: the cell of the point / the one below / the one above = {counts[:3]}")
                assert counts == KINDS[case][key], (case, key, counts)
            assert (label == "K.lin_cell").sum() >= 5
        else:
            assert not (label == "K.lin_cell").any() and "lin_cell.Z" not in KINDS[case]
    assert 3 * compared >= 2 * n, f"{compared} of {n} states of class K are value-compared"
    # a trace kernel takes and keeps a step from two thirds of them too (k is rescaled onto the dispersion relation)
    steps = sum(int(((w == 0) & r & v1).sum()) for w, r, v1, z in (rc.expected_ode_step(rc.load_fixture(c, "K")) for c in rc.K_CASES))
    assert 3 * steps >= 2 * n, f"{steps} of {n} states of class K start a step that is kept"
    print(f"class K: {compared} of {n} states are value-compared")


_psi_cache = {}


def _psi(case, v):
    if case not in _psi_cache:
        _psi_cache[case] = rc._Case(case)
    c = _psi_cache[case]
    return np.array([c.psiN(x) for x in v])


@pytest.mark.parametrize("case", rc.K_CASES)
def test_oracle_equals_the_reference_at_every_knot_state(case):
    g, p, tab, f = _case(case, "K")
    got = [oracle_lib.probe(p, v) for v in f["v"]]
    got = {k: np.array([o[k] for o in got]) for k in ("eq", "cold", "num", "dvds", "resid", "codes")}
    rc.compare_probe(f, got, f"{case}: oracle_lib.probe")
    v1, resid, code, stopped = oracle_lib.step(p, f["v"], f["s"])
    rc.compare_step(f, v1, resid, np.where(stopped, code, 0), f"{case}: oracle_lib.step")


@pytest.mark.parametrize("case", rc.K_CASES)
def test_device_source_on_host_equals_the_reference_at_every_knot_state(case):
    _compare_emulated(case, classes="K")


@pytest.mark.parametrize("case", rc.K_CASES)
def test_trace_kernel_step_on_host_equals_the_reference_at_every_knot_state(case):
    g, p, tab, f = _case(case, "K")
    v1, resid, code = emul_lib.ode_step(p, f["v"], f["s"])
    want_code, code_rows, v1_rows, zero_rows = rc.expected_ode_step(f)
    what = f"{case}: emul_lib.ode_step"
    rc._check(f, what, "the stop code", code, want_code, code_rows)
    kept = v1_rows & (want_code == 0) & code_rows
    rc._check(f, what, "v1", v1, f["step"]["v1"], kept)
    rc._check(f, what, "the residual at v1", resid, f["step"]["resid1"], kept & f["ok"]["step_cs"])


@pytest.mark.parametrize("case", rc.K_CASES)
def test_emulated_diagnostics_at_the_knot_states(case):
    g, p, tab, f = _case(case, "K")
    dx.emul_set_tables(tab)
    ray_vec, residual, npoints, rows = rc.class_rays(f)
    got, bad = dx.emul_diagnostics(p, ray_vec, residual, npoints)
    for r, idx in enumerate(rows):
        want = dx.expected_at_points(p, tab, f["v"][idx], f["probe"]["resid"][idx])
        for name in dx.FIELDS:
            dx.assert_bits(got[name][r, :len(idx)], want[name], f"{case} class K {name}")
        for k, i in enumerate(idx):
            for name, val in dx.from_eq_record(p, f["v"][i], f["probe"]["eq"][i], f["probe"]["resid"][i]).items():
                dx.assert_bits(got[name][r, k], val, f"{case} state {i} {name} (reference eq record)")


@pytest.mark.parametrize("case", rc.K_CASES)
def test_one_step_trace_on_host_from_every_knot_state(case):
    """The recording RK4 trace kernel on the host, LAUNCHED at the states with nstep_max = 1 (the GPU tier runs the same
    launch through the kernels that read the tables from LDS and through those that read global memory)."""
    from rays_amd.params import copy_params
    g, p, tab, f = _case(case, "K")
    q = copy_params(p)
    q.nstep_max = 1
    out = emul_lib.trace(q, f["v"][:, :3], f["v"][:, 3:6] / p.k0)
    dx.assert_bits(out["ray_vec"][:, 0], f["v"], f"{case}: the launch point is the state")
    last = np.arange(len(f["v"])), out["npoints"] - 1
    rc.compare_one_step_trace(f, out["npoints"], out["stop_code"], out["ray_vec"][last], out["residual"][last], f"{case}: emul_lib.trace")
    started = ~rc.expected_ode_step(f)[3]       # (a ray whose own check_save refuses its launch point has no summary)
    dx.assert_bits(out["end_ray_vec"][started], out["ray_vec"][last][started], case)


def test_the_new_case_is_given_the_kernels_of_the_129_case_at_every_request():
    """The new case's host tables are a fixture under tests/golden/ (binary files are kept there), so its namelist is
    none of the configurations tests/golden/kernel_selection.json lists by loading configs/*.in.  Its rows are held here
    instead: for every request of that table (fan size x numerics x the two developer switches, all five kernels and
    the step loop) the answer for its parameters is the committed row of the 129 x 129 case, whose shape it shares."""
    import json
    import os
    from tests import kernel_selection_lib as ks
    from tests.common import ROOT
    with open(os.path.join(ROOT, "tests", "golden", "kernel_selection.json")) as fh:
        golden = json.load(fh)
    want = golden["configs"]["gold_axisym64_eqdsk129_tspline_damp_rk4.in"]
    assert NEW + ".in" not in golden["configs"] and len(want) == len(ks.CONFIG_REQUESTS)
    saved, numerics = {k: os.environ.get(k) for k in ks.ENV}, ks.hip.get_numerics()
    try:
        t = ks.Table()
        got = ks.requests(t, load_golden(NEW)[2], ks.CONFIG_REQUESTS)
    finally:
        ks.hip.set_numerics(numerics)
        for k, val in saved.items():
            os.environ.pop(k, None)
            if val is not None:
                os.environ[k] = val
    text = lambda strings, row: [strings[i] for i in row[:-1]] + [row[-1]] if len(row) > 1 else [strings[row[0]]]
    for req, w, g in zip(ks.CONFIG_REQUESTS, want, got):
        assert text(t.strings, g) == text(golden["strings"], w) and len(g) == 6, req
