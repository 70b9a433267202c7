"""GPU tier: the life cycle of the C ABI's device resources (rays_amd/csrc/rays_capi_resources.hpp).  rays_hip_finalize
gives everything back and the library then works as on first use -- lazy init, the tables uploaded again from their host
copies, the workspaces allocated again; the ode_step scratch block regrows on its stream without disturbing a result.
(The multi-device side of the same code runs in the CPU tier: tests/test_cpu_capi_emul.py, test_cpu_capi_resources.py.)"""
import numpy as np
import pytest

from rays_amd import hip
from tests.common import assert_matches_golden, load_golden

pytestmark = pytest.mark.gpu

CASES = ["gold_axisym64_eqdsk_damp_rk4",   # Z-function and eqdsk tables
         "gold_solovev64_sg_cold"]         # SG workspace


@pytest.mark.parametrize("name", CASES)
def test_trace_finalize_trace(name):
    g, nml, p = load_golden(name)
    try:
        out = hip.trace_host(p, g["rvec0"], g["rindex_vec0"], ngpu=1)
        assert_matches_golden(out, g, p, exact=True)
        hip.finalize()
        out = hip.trace_host(p, g["rvec0"], g["rindex_vec0"], ngpu=1)   # (no table is set again: hip.py set them once)
        assert_matches_golden(out, g, p, exact=True)
    finally:
        hip.finalize()


def test_ode_step_scratch_regrows_on_its_stream():
    """n = 3, then 700 (the block grows behind a stream synchronisation), then 3 again (the larger block is reused):
    each result equals that of the same states stepped in a call of their own on a library with no scratch yet."""
    g, nml, p = load_golden(CASES[0])
    ref, npts = g["ray_vec"], g["npoints"]
    v0 = np.concatenate([ref[r, :int(n) - 1] for r, n in enumerate(npts) if n >= 2])
    s0 = np.concatenate([float(p.ds) * np.arange(int(n) - 1) for n in npts if n >= 2])
    v0, s0 = np.resize(v0, (700, p.nv)), np.resize(s0, 700)     # (472 recorded points, repeated up to 700 states)
    try:
        alone = {}
        for n in (3, 700):
            hip.finalize()
            alone[n] = hip.ode_step(p, v0[:n], s0[:n])
        assert (alone[700][2] == 0).all() and not np.array_equal(alone[700][0], v0)   # every state was stepped
        hip.finalize()
        for n in (3, 700, 3):
            got = hip.ode_step(p, v0[:n], s0[:n])
            for a, b, what in zip(got, alone[n], ("v1", "resid", "stop_code")):
                np.testing.assert_array_equal(a, b, err_msg=f"n = {n}: {what}")
    finally:
        hip.finalize()


def test_no_kept_result_after_finalize():
    g, nml, p = load_golden(CASES[0])
    power, nb = g["dep_power"], int(g["dep_n_bins"])
    prev = hip.keep_last_result(True)
    try:
        out = hip.trace_host(p, g["rvec0_full"], g["rindex_vec0_full"], ngpu=1)
        np.testing.assert_array_equal(out["npoints"], g["npoints_full"])
        assert hip.deposition_last(p, "Ptotal_psi", nb, power) is not None   # held ...
        hip.finalize()
        assert hip.deposition_last(p, "Ptotal_psi", nb, power) is None       # ... RAYS_HIP_NO_KEPT_RESULT
        assert hip.keep_last_result(True) is True                            # (the switch itself survives finalize)
    finally:
        hip.keep_last_result(prev)
        hip.finalize()
