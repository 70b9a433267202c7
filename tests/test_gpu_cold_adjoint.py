"""GPU tier: the tolerance flavour's regrouped cold-plasma arithmetic (rays_device_arith.inc: deriv_cold's adjoint form
and factored gradient, check_save's residual from deriv_cold's own index components) against the reference's RECORDED
residuals -- the one output of the changed code that the per-step trajectory bars do not look at.

  * every flavour fixture (slab, Solovev, axisym; rays that leave the plasma or the box, that stop on the residual;
    one, two species): one step restarted with hip.ode_step from every recorded reference point that has a successor.
    No restarted step may stop, and the residual check_save returns at the new point is within the project's
    resid_atol = 1e-9 of the residual the reference recorded there (it is a cancellation remainder: absolute bar);
  * 64 rays of the cfg 2 Solovev fixture (the rays it records, filled up to one wave) traced under automatic selection
    (the lean step loop) and with the general loop forced, so that both copies of the step loop run the new arithmetic:
    counts exact, every recorded residual within the same bar."""
import numpy as np
import pytest

from rays_amd import hip
from tests.common import load_golden, stop_codes
from tests.test_gpu_tolerance_flavour import CASES

pytestmark = pytest.mark.gpu

RESID_ATOL = 1e-9   # the project's bar for the residual (tests/common.py: assert_matches_golden under the flavour)
LOOP_FIXTURE = "cfg2_solovev1024_rk4"   # the Solovev fixture whose models take the lean step loop (the headline's kernel)


@pytest.fixture(autouse=True)
def tolerance_numerics():
    prev = hip.set_numerics("tolerance")
    yield
    hip.set_numerics(prev)


@pytest.mark.parametrize("name", CASES)
def test_restarted_steps_return_the_recorded_residual(name):
    g, nml, p = load_golden(name)
    assert int(hip.kernel_name(p).split("<")[1].split(",")[0]) & 16, "not the tolerance flavour"
    ref, res, npts = g["ray_vec"], g["residual"], g["npoints"]
    v0, r1, s0 = [], [], []
    for r in range(len(npts)):
        n = int(npts[r])
        if n < 2:
            continue
        v0.append(ref[r, :n - 1])
        r1.append(res[r, 1:n])
        s0.append(np.concatenate([[0.0], np.cumsum(np.full(n - 1, float(p.ds)))])[:n - 1])
    if not v0:
        pytest.skip("no ray of this fixture takes a step")
    v0, r1, s0 = np.concatenate(v0), np.concatenate(r1), np.concatenate(s0)
    _, resid, code = hip.ode_step(p, v0, s0)
    worst = float(np.abs(resid - r1).max())
    print(f"{name}: {len(v0)} restarted steps, {int((code != 0).sum())} stopped, max |residual - recorded| {worst:.3e}, "
          f"largest recorded residual {float(np.abs(r1).max()):.3e}")
    assert (code == 0).all(), f"{(code != 0).sum()} of {len(code)} restarted steps stopped: {np.unique(code)}"
    assert worst <= RESID_ATOL, f"residual {worst:.3e} off the reference's"


@pytest.mark.parametrize("loop", ["automatic", "forced_general"])
def test_both_step_loops_record_the_references_residuals(loop, monkeypatch):
    g, nml, p = load_golden(LOOP_FIXTURE)
    # one wave: the rays whose trajectories the fixture records, filled up to 64 with their neighbours in the fan
    idx = np.asarray(g["ray_index"])
    sel = np.concatenate([idx, np.setdiff1d(np.arange(len(g["rvec0_full"])), idx)[:64 - len(idx)]])
    assert len(sel) == 64 and hip.kernel_name(p, 64) == "rk4_trace_kernel<21, 2, 0, 7>"
    if loop == "automatic":
        monkeypatch.delenv("RAYS_HIP_RK4_LOOP", raising=False)
        assert hip.rk4_loop(p, 64) == "lean"
    else:
        monkeypatch.setenv("RAYS_HIP_RK4_LOOP", "general")
        assert hip.rk4_loop(p, 64) == "general"
    out = hip.trace_host(p, g["rvec0_full"][sel], g["rindex_vec0_full"][sel], ngpu=1)
    np.testing.assert_array_equal(out["npoints"], g["npoints_full"][sel])
    np.testing.assert_array_equal(out["stop_code"], stop_codes(g["stop_flag_full"][sel]))
    keep = g["residual"].shape[1]
    got = out["residual"][:len(idx)]
    worst = float(np.abs(got[:, :keep] - g["residual"]).max())
    print(f"{loop}: {int(g['npoints'].sum())} recorded points, max |residual - recorded| {worst:.3e}")
    assert worst <= RESID_ATOL
    assert not got[:, keep:].any()
