"""GPU tier: the equilibrium's table lookups ON AND BESIDE THEIR KNOTS (class K of tests/rhs_state_cases.py, the reference's
records in tests/golden/eq_knot_states.npz): grid nodes of the R-Z tables and their neighbouring doubles, psiN on and beside
the knots of the profile splines, the truncating cell index of the bilinear model.  Only there does the cell search take
its rare branches (the estimate one cell off and the second fetch, the node that ends in the cell below it), and the
fetch exists twice: from the LDS copy of the tables that the one-wave-per-SIMD RK4 trace kernels make, and from global
memory (probe, diagnostics and Shampine-Gordon kernels).  Bit for bit under the exact numerics.  Reads tests/golden/,
configs/ and the library only."""
import re

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import diag_expect as dx, emul_build as eb, oracle_lib, rhs_state_cases as rc
from tests.common import host_libm_is_the_variant_the_fixtures_were_cut_with, load_golden
from tests.test_gpu_rhs_states import PER_STEP_TOL, _device_diagnostics, _numerics, _probe_params

pytestmark = pytest.mark.gpu
NEW = "gold_axisym16_eqdsk49x65_tspline_damp_rk4"
EQ_TAB_LDS_BYTES = 32768      # rays_trace.hpp: kEqTabBytes, what a kernel's LDS copy of the tables may take


def _case(case):
    g, nml, p = load_golden(case)
    return g, p, eb.axisym_tables_of(g), rc.load_fixture(case, "K")


def stages_tables_in_lds(kernel, tab):
    """rays_rk4.hpp / rays_rk4_body.inc: the one-wave-per-SIMD RK4 kernel of the axisym_toroid equilibrium (EQ & 3 == 2), in
    every variant (recording, summary-only, ...), copies the 1-D tables and the R and Z grids into LDS when they fit
    kEqTabBytes and looks them up there (DevParams::a_lds_tab, a_lds_rz); the two-waves-per-SIMD kernel and the
    Shampine-Gordon kernels read global memory, as the probe, diagnostics and launcher kernels do."""
    name, eq = re.match(r"(\w+)<(\d+),", kernel).groups()
    doubles = sum(5 * np.size(tab.get(k + "_grid", ())) for k in ("rb", "ne", "te", "ti")) + \
        np.size(tab.get("r_grid", ())) + np.size(tab.get("z_grid", ()))
    has_1d = any(np.size(tab.get(k + "_grid", ())) for k in ("rb", "ne", "te", "ti"))
    return name == "rk4_trace_kernel" and int(eq) & 3 == 2 and has_1d and 8 * doubles <= EQ_TAB_LDS_BYTES


@pytest.mark.parametrize("case", rc.K_CASES)
def test_device_probe_equals_the_reference_and_the_oracle_at_every_knot_state(case):
    """hip.probe (tables from global memory), one launch: against the reference's records, and at every state against
    oracle_lib.probe with the same nv = 7 parameters."""
    assert host_libm_is_the_variant_the_fixtures_were_cut_with()
    g, p, tab, f = _case(case)
    q = _probe_params(p)
    dev = hip.probe(q, f["v"][:, :7])
    numerical = rc.integrates_numerically(case)
    rc.compare_probe(f, dev, f"{case}: hip.probe", keys=("cold", "num", "resid") if numerical else ("cold", "num", "dvds", "resid"),
                     columns=7, rhs_flag_rows=f["eq_code"] != 0 if numerical else None, cs_flag_rows=f["cs_code"] != 42)
    ora = [oracle_lib.probe(q, np.ascontiguousarray(v[:7])) for v in f["v"]]
    np.testing.assert_array_equal(dev["codes"][:, [0, 2, 3]], np.array([o["codes"] for o in ora])[:, [0, 2, 3]])
    for key in ("cold", "num", "resid"):
        dx.assert_bits(dev[key], np.array([o[key] for o in ora]), f"{case} {key}")
    if not numerical:
        dx.assert_bits(dev["dvds"], np.array([o["dvds"] for o in ora]), f"{case} dvds")


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("case", rc.K_CASES)
def test_device_diagnostics_at_the_knot_states(case, packed):
    """The padded and the packed diagnostics entry on an array whose points are the states: all nineteen fields, Psi among
    them, equal diag_expect.expected_at_points (held to the reference's records at these states by the CPU tier) and the
    reference's eq record."""
    assert host_libm_is_the_variant_the_fixtures_were_cut_with()
    g, p, tab, f = _case(case)
    ray_vec, residual, npoints, rows = rc.class_rays(f)
    got = _device_diagnostics(p, ray_vec, residual, npoints, packed)
    pr = f["probe"]
    for r, idx in enumerate(rows):
        want = dx.expected_at_points(p, tab, f["v"][idx], pr["resid"][idx])
        for name in dx.FIELDS:
            dx.assert_bits(got[name][r, :len(idx)], want[name], f"{case} class K {name}")
        for k, i in enumerate(idx):
            for name, val in dx.from_eq_record(p, f["v"][i], pr["eq"][i], pr["resid"][i]).items():
                dx.assert_bits(got[name][r, k], val, f"{case} state {i} {name} (reference eq record)")


@pytest.mark.parametrize("case", rc.K_CASES)
def test_device_step_equals_the_reference_at_every_knot_state(case):
    """hip.ode_step under the exact numerics: stop code, v1 and the residual of a kept step equal the reference's."""
    g, p, tab, f = _case(case)
    with _numerics("exact"):
        v1, resid, code = hip.ode_step(p, f["v"], f["s"])
    want_code, code_rows, v1_rows, zero_rows = rc.expected_ode_step(f)
    rc._check(f, f"{case}: hip.ode_step", "the stop code", code, want_code, code_rows)
    rc.compare_step(f, v1, resid, code, f"{case}: hip.ode_step", v1_rows=v1_rows, resid_of_kept_steps_only=True,
                    code_rows=np.zeros(len(code), dtype=bool))
    assert not v1[zero_rows].any()


def _launch_one_step(p, v, summary_only):
    """A trace of nstep_max = 1 launched at the states through rays_hip_trace_device | rays_hip_trace_summary_device:
    (npoints, stop code, the last point, its residual or None, the first point)"""
    import torch
    q = copy_params(p)
    q.nstep_max = 1
    n, nv = len(v), p.nv
    r0 = torch.as_tensor(np.ascontiguousarray(v[:, :3])).cuda()
    n0 = torch.as_tensor(np.ascontiguousarray(v[:, 3:6] / p.k0)).cuda()
    npts = torch.zeros(n, dtype=torch.int32, device="cuda")
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    end = torch.zeros((n, nv), dtype=torch.float64, device="cuda")
    er, mr = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if summary_only:
        start = torch.zeros((n, nv), dtype=torch.float64, device="cuda")
        hip.trace_summary_device(q, n, r0.data_ptr(), n0.data_ptr(), npts.data_ptr(), sc.data_ptr(), start.data_ptr(),
                                 end.data_ptr(), er.data_ptr(), mr.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        return npts.cpu().numpy(), sc.cpu().numpy(), end.cpu().numpy(), None, start.cpu().numpy()
    rv = torch.zeros((n, 2, nv), dtype=torch.float64, device="cuda")
    res = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    hip.trace_device(q, n, r0.data_ptr(), n0.data_ptr(), rv.data_ptr(), res.data_ptr(), npts.data_ptr(), sc.data_ptr(),
                     end.data_ptr(), er.data_ptr(), mr.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    npoints, rv, res = npts.cpu().numpy(), rv.cpu().numpy(), res.cpu().numpy()
    last = np.arange(n), npoints - 1
    return npoints, sc.cpu().numpy(), rv[last], res[last], rv[:, 0]


@pytest.mark.parametrize("case", rc.K_CASES)
def test_one_recorded_step_through_the_lds_staged_tables(case):
    """One step of a trace LAUNCHED at every state (class K holds launch states) through rays_hip_trace_device and through
    rays_hip_trace_summary_device: the RK4 trace kernels, which look the tables up in their LDS copy -- the same states the
    probe and diagnostics kernels above take through global memory.  Both equal the reference's step record."""
    g, p, tab, f = _case(case)
    n = len(f["v"])
    with _numerics("exact"):
        recording, summary = hip.kernel_name(p, n), hip.summary_kernel_name(p, n)
        assert recording != summary and stages_tables_in_lds(recording, tab) and stages_tables_in_lds(summary, tab)
        npoints, code, v_end, resid_end, v_start = _launch_one_step(p, f["v"], False)
        dx.assert_bits(v_start, f["v"], f"{case}: the launch point is the state")
        kept = rc.compare_one_step_trace(f, npoints, code, v_end, resid_end, f"{case}: rays_hip_trace_device ({recording})")
        npoints, code, v_end, _, v_start = _launch_one_step(p, f["v"], True)
        rc.compare_one_step_trace(f, npoints, code, v_end, None, f"{case}: rays_hip_trace_summary_device ({summary})")
        dx.assert_bits(v_start[kept], f["v"][kept], f"{case}: start_ray_vec")


@pytest.mark.parametrize("case", ["gold_axisym64_eqdsk129_tspline_damp_rk4", NEW])
def test_one_output_interval_of_the_sg_kernel_from_the_knot_states(case):
    """The Shampine-Gordon integrator on the same tables, the trace kernel that reads them from global memory
    (stages_tables_in_lds is false for it): one output interval of a trace launched at the value-compared states equals the
    oracle's, which the CPU tier holds to the reference at these states.  The 129 x 129 case under its own `_damp_sg`
    configuration; the 49 x 65 case, the only one whose estimate is off in R, under its own parameters with the
    integrator of that configuration (its namelist carries the &SG_ode_list of the 129 x 129 one)."""
    assert host_libm_is_the_variant_the_fixtures_were_cut_with()
    p_sg = load_golden("gold_axisym64_eqdsk129_tspline_damp_sg")[2]
    g, p_rk4, tab, f = _case(case)          # (after the line above: the tables every library holds are this case's)
    p = copy_params(p_sg if case != NEW else p_rk4)
    p.ode_solver = p_sg.ode_solver
    p.nstep_max = 1
    v = f["v"][f["ok"]["values"]]
    assert not stages_tables_in_lds(hip.kernel_name(p, len(v)), tab)
    r0, n0 = np.ascontiguousarray(v[:, :3]), np.ascontiguousarray(v[:, 3:6] / p.k0)
    out = hip.trace_host(p, r0, n0, ngpu=1)
    ora = oracle_lib.trace(p, r0, n0)
    assert (ora["npoints"] == 2).sum() * 3 >= 2 * len(v)
    for k in ("stop_code", "npoints", "ray_vec", "residual", "end_ray_vec", "end_residuals", "max_residuals"):
        np.testing.assert_array_equal(out[k], ora[k], err_msg=k)


@pytest.mark.parametrize("case", rc.K_CASES)
def test_tolerance_step_at_the_knot_states(case):
    """The comparison of test_tolerance_step_at_the_interior_states at the states of class K from which the reference takes
    and keeps a step: equal stop codes, v1 within BASELINE's per-step bar of the reference's."""
    g, p, tab, f = _case(case)
    want_code, code_rows, v1_rows, zero_rows = rc.expected_ode_step(f)
    a = code_rows & v1_rows & (want_code == 0)
    assert 3 * a.sum() >= 2 * len(a)
    with _numerics("tolerance"):
        v1, resid, code = hip.ode_step(p, f["v"][a], f["s"][a])
    np.testing.assert_array_equal(code, want_code[a])
    want = f["step"]["v1"][a]
    for sl in (slice(0, 3), slice(3, 6)):
        err = np.linalg.norm(v1[:, sl] - want[:, sl], axis=1) / np.linalg.norm(want[:, sl], axis=1)
        worst = int(np.argmax(err))
        print(f"{case}: rows {sl.start}-{sl.stop - 1}: worst per-step relative error {err.max():.3e} "
              f"({f['label'][a][worst]}, side {int(f['side'][a][worst])})")
        assert err.max() <= PER_STEP_TOL
