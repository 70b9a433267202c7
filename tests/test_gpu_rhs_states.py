"""GPU tier: the device right-hand side at the threshold states of tests/golden/rhs_state_cases.npz (box bounds, the plasma
edge, the damping argument beside +-5 and beside the Z-function's knots, check_save's limits, RK4 stages that refuse)
against the reference's own records of the same states -- flags everywhere they are facts of the reference, values where
it defines them, bit for bit under the exact numerics.  Reads tests/golden/, configs/ and the library only."""
import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import diag_expect as dx, emul_build as eb, oracle_lib, rhs_state_cases as rc
from tests.common import host_libm_is_the_variant_the_fixtures_were_cut_with, load_golden

pytestmark = pytest.mark.gpu
PER_STEP_TOL = 1e-10   # BASELINE: the tolerance flavour's bar, relative, norm-wise on r and on k


def _case(case):
    g, nml, p = load_golden(case)
    return g, p, eb.axisym_tables_of(g), rc.load_fixture(case)


def _probe_params(p):
    """the rows probe_kernel evaluates: nv = 7 (rays_probe.hip)"""
    q = copy_params(p)
    q.nv, q.damping_model, q.multi_spec_damping, q.integrate_eq_gradients = 7, 0, 0, 0
    return q


@pytest.mark.parametrize("case", rc.CASES)
def test_device_probe_equals_the_reference_at_every_state(case):
    """hip.probe, one launch per case: the equilibrium and eqn_ray flags wherever they are reference facts; cold, num,
    dvds (rows 1-7; the probe's eqn_ray uses the cold derivatives, so not under ray_deriv_name = 'numerical') and resid
    where the reference defines values.  check_save's flag: not where the reference's is 'total_absorption', which the
    nv = 7 rows do not have."""
    g, p, tab, f = _case(case)
    dev = hip.probe(_probe_params(p), f["v"][:, :7])
    numerical = rc.integrates_numerically(case)
    rc.compare_probe(f, dev, f"{case}: hip.probe", keys=("cold", "num", "resid") if numerical else ("cold", "num", "dvds", "resid"),
                     columns=7, rhs_flag_rows=f["eq_code"] != 0 if numerical else None, cs_flag_rows=f["cs_code"] != 42)
    stopped = f["probe"]["rhs_stop"] == 1     # eqn_ray returns before it sets dvds: the zeros it was handed stay
    assert stopped.any() and not dev["dvds"][stopped].any()


@pytest.mark.parametrize("case", rc.CASES)
def test_device_probe_equals_the_oracle_at_every_state(case):
    """The same launch against oracle_lib.probe with the same nv = 7 parameters, at EVERY state: where the reference is
    undefined (a state outside the box, a flag decided on an unset variable) the device is defined as the oracle is."""
    assert host_libm_is_the_variant_the_fixtures_were_cut_with()
    g, p, tab, f = _case(case)
    q = _probe_params(p)
    dev = hip.probe(q, f["v"][:, :7])
    ora = [oracle_lib.probe(q, np.ascontiguousarray(v[:7])) for v in f["v"]]
    np.testing.assert_array_equal(dev["codes"][:, [0, 2, 3]], np.array([o["codes"] for o in ora])[:, [0, 2, 3]])
    for key in ("cold", "num", "resid"):
        dx.assert_bits(dev[key], np.array([o[key] for o in ora]), f"{case} {key}")
    if not rc.integrates_numerically(case):
        np.testing.assert_array_equal(dev["codes"][:, 1], np.array([o["codes"][1] for o in ora]))
        dx.assert_bits(dev["dvds"], np.array([o["dvds"] for o in ora]), f"{case} dvds")   # zeros where eqn_ray stops


def _device_diagnostics(p, ray_vec, residual, npoints, packed):
    import torch
    nray, npt = residual.shape
    q = copy_params(p)
    q.nstep_max = npt - 1
    rv, res = torch.as_tensor(ray_vec).cuda(), torch.as_tensor(residual).cuda()
    npd = torch.as_tensor(npoints).cuda()
    bad = torch.zeros(nray, dtype=torch.int32, device="cuda")
    nf = len(dx.FIELDS)
    if not packed:
        out = torch.full((nf, nray, npt), float("nan"), dtype=torch.float64, device="cuda")
        names = hip.ray_diagnostics_device(q, nray, rv.data_ptr(), res.data_ptr(), npd.data_ptr(), None, out.data_ptr(),
                                           bad.data_ptr())
        torch.cuda.synchronize()
        return {n: out[k].cpu().numpy() for k, n in enumerate(names)}
    off = hip.diag_offsets(npoints, npt - 1)
    total = int(off[-1])
    d_off = torch.as_tensor(off).cuda()
    out = torch.full((nf, total), float("nan"), dtype=torch.float64, device="cuda")
    names = hip.ray_diagnostics_packed_device(q, nray, rv.data_ptr(), res.data_ptr(), npd.data_ptr(), d_off.data_ptr(), total,
                                              None, out.data_ptr(), bad.data_ptr())
    torch.cuda.synchronize()
    return hip.diag_unpack({n: out[k].cpu().numpy() for k, n in enumerate(names)}, off, npt)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("case", rc.CASES)
def test_device_diagnostics_at_the_states(case, packed):
    """rays_hip_ray_diagnostics_device and the packed entry on arrays whose points are the states, one "ray" per class
    (npoints = the class size): all nineteen fields equal diag_expect.expected_at_points, which the CPU tier holds
    against the reference's records at these states; n_imag and xi_0..2 carry classes E and F."""
    assert host_libm_is_the_variant_the_fixtures_were_cut_with()      # (n_imag and Psi come through the oracle)
    g, p, tab, f = _case(case)
    ray_vec, residual, npoints, rows = rc.class_rays(f)
    got = _device_diagnostics(p, ray_vec, residual, npoints, packed)
    pr = f["probe"]
    for r, idx in enumerate(rows):
        want = dx.expected_at_points(p, tab, f["v"][idx], pr["resid"][idx])
        for name in dx.FIELDS:
            dx.assert_bits(got[name][r, :len(idx)], want[name], f"{case} class {f['cls'][idx[0]]} {name}")
        for k, i in enumerate(idx):      # and straight from the reference's eq record, for the fields it determines
            for name, val in dx.from_eq_record(p, f["v"][i], pr["eq"][i], pr["resid"][i]).items():
                dx.assert_bits(got[name][r, k], val, f"{case} state {i} {name} (reference eq record)")


def _numerics(mode):
    class _Ctx:
        def __enter__(self):
            self.prev = hip.set_numerics(mode)

        def __exit__(self, *a):
            hip.set_numerics(self.prev)
    return _Ctx()


@pytest.mark.parametrize("case", rc.CASES)
def test_device_step_equals_the_reference_at_every_state(case):
    """hip.ode_step under the exact numerics: stop code, v1 and the residual of a kept step equal the reference's step
    record at every state, class H (a later stage refuses: v untouched) included; a state whose own check_save sets
    stop_ode never starts (its flag, v1 = 0)."""
    g, p, tab, f = _case(case)
    with _numerics("exact"):
        v1, resid, code = hip.ode_step(p, f["v"], f["s"])
    want_code, code_rows, v1_rows, zero_rows = rc.expected_ode_step(f)
    rc._check(f, f"{case}: hip.ode_step", "the stop code", code, want_code, code_rows)
    rc.compare_step(f, v1, resid, code, f"{case}: hip.ode_step", v1_rows=v1_rows, resid_of_kept_steps_only=True,
                    code_rows=np.zeros(len(code), dtype=bool))
    assert not v1[zero_rows].any()
    h = (f["cls"] == "H") & code_rows
    if (want_code[h] == 0).any():      # (one case's class H lies off its rays: no trace starts there)
        assert (code[h] != 0).any() and (code[h] == 0).any()


@pytest.mark.parametrize("case", rc.CASES)
def test_tolerance_step_at_the_interior_states(case):
    """hip.ode_step under the tolerance numerics on class A only (threshold states are outside that flavour's contract:
    its bar on well-conditioned steps plus hand-over): equal stop codes, v1 within the per-step bar of the reference's."""
    g, p, tab, f = _case(case)
    a = f["cls"] == "A"
    with _numerics("tolerance"):
        v1, resid, code = hip.ode_step(p, f["v"][a], f["s"][a])
    want_code, code_rows, v1_rows, zero_rows = rc.expected_ode_step(f)
    assert code_rows[a].all() and v1_rows[a].all()
    np.testing.assert_array_equal(code, want_code[a])
    want = f["step"]["v1"][a]
    for sl in (slice(0, 3), slice(3, 6)):
        err = np.linalg.norm(v1[:, sl] - want[:, sl], axis=1) / np.linalg.norm(want[:, sl], axis=1)
        print(f"{case}: rows {sl.start}-{sl.stop - 1}: worst per-step relative error {err.max():.3e}")
        assert err.max() <= PER_STEP_TOL


def test_probe_refuses_the_shapes_its_kernel_does_not_evaluate():
    """rays_hip_probe returned 0 with uninitialised output for nv != 7 or a species count other than 2 or 3 (the kernel
    returns early): now an error that names the shape, and the caller's arrays are left as they were."""
    import ctypes as C
    g, nml, p = load_golden("gold_solovev64_damp_rk4")
    v = np.ascontiguousarray(g["ray_vec"][0, :2])
    out = [np.full((2, 7), -7.0), np.full((2, 7), -7.0), np.full((2, p.nv), -7.0), np.full(2, -7.0)]
    codes = np.full((2, 4), -7, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    rc_ = hip.load().rays_hip_probe(C.byref(p), 2, v.ctypes.data_as(dp), *[a.ctypes.data_as(dp) for a in out],
                                    codes.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc_ != 0 and all((a == -7.0).all() for a in out) and (codes == -7).all()
    with pytest.raises(hip.RaysHipError, match=r"rays_hip_probe: no kernel built for this configuration .*nv = 8"):
        hip.probe(p, g["ray_vec"][0, :2])
    g, nml, p = load_golden("gold_solovev64_4spec_rk4_num")
    with pytest.raises(hip.RaysHipError, match=r"rays_hip_probe: no kernel built for this configuration .*4 species"):
        hip.probe(p, g["ray_vec"][0, :2])
    g, nml, p = load_golden("gold_solovev64_pow_rk4")
    assert hip.probe(p, g["ray_vec"][0, :2])["codes"].shape == (2, 4)
