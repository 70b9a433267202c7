"""CPU tier: the stage of the RK4 trace kernels is a property of the WAVE (rays_rk4_body.inc: one scalar, advanced once per
trip, set to 3 by the pass that starts rays), not of a lane.  That rests on an invariant -- every lane under way is at its
wave's stage on every trip, with or without refills, in both loop structures -- which the wave emulator checks here: built
with -DRAYS_EMUL_CHECK_UNIFORM_STAGE every lane also keeps the stage it would have on its own, and every trip compares the
two (and the lanes' copies of the wave's stage with lane 0's).  The outputs are compared with the oracle bit for bit, as in
test_cpu_rk4_wave_emul.py, and the count of violations must stay zero."""
import ctypes as C

import numpy as np
import pytest

from tests import group_emul_lib as ge
from tests import oracle_lib
from tests.common import load_golden

ARRAYS = ("npoints", "stop_code", "ray_vec", "residual", "end_ray_vec", "end_residuals", "max_residuals")
CHECK = "-DRAYS_EMUL_CHECK_UNIFORM_STAGE"
# RAYS_REFILL_EVENT_COST (idle lane-trips that trigger a pass): the default and "at the next stage-3 trip"
VARIANTS = {"stagecheck": [CHECK], "stagecheck_cost0": [CHECK, "-DRAYS_REFILL_EVENT_COST=0"]}


def _lib(variant):
    library = ge.lib_variant(variant, VARIANTS[variant])
    library.rays_emul_uniform_stage_violations.restype = C.POINTER(C.c_int)  # only the checking build has it
    library.rays_emul_uniform_stage_violations.argtypes = []
    return library


def _violations(library):
    return int(library.rays_emul_uniform_stage_violations()[0])


def _check(out, ora):
    for k in ARRAYS:
        np.testing.assert_array_equal(out[k], ora[k], err_msg=k)


@pytest.mark.parametrize("stride,w2_body", [(0, False), (4, False), (16, False), (0, True)],
                         ids=["stride0", "stride4", "stride16", "w2_body"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_solovev_fan_with_refills(variant, stride, w2_body):
    """200 rays of the Solovev fan at their natural, ragged lengths (99..380 steps) on ONE wave: every lane is refilled
    two or three times and rays end on different trips and at different stages (ray 7 at its initial check).  The body of
    the two-waves-per-SIMD build hands rays out in index order whatever the stride, so it runs with stride 0 only."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::5][:200].copy(), g["rindex_vec0_full"][::5][:200].copy()
    n0[7] *= 3.0   # far off the dispersion surface: stops at its initial check
    ora = oracle_lib.trace(p, r0, n0)
    assert len(set(ora["npoints"].tolist())) > 20 and ora["npoints"][7] == 1
    library = _lib(variant)
    _check(ge.trace_rk4_waves(p, r0, n0, nwaves=1, library=library, stride=stride, w2_body=w2_body), ora)
    assert _violations(library) == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_slab_box_exits_two_waves(variant):
    """Rays that leave the box after a few steps (and one that starts outside it), tiled to 300 rays on two waves: stages
    refuse (a stop at stage 0, 1 or 2) next to lanes that go on."""
    g, nml, p = load_golden("gold_slab_box_exits_rk4")
    reps = -(-300 // len(g["rvec0_full"]))
    r0, n0 = np.tile(g["rvec0_full"], (reps, 1))[:300], np.tile(g["rindex_vec0_full"], (reps, 1))[:300]
    ora = oracle_lib.trace(p, r0, n0)
    assert len(set(ora["stop_code"].tolist())) > 1
    library = _lib(variant)
    _check(ge.trace_rk4_waves(p, r0, n0, nwaves=2, library=library), ora)
    _check(ge.trace_rk4_waves(p, r0, n0, nwaves=2, library=library, stride=4), ora)
    _check(ge.trace_rk4_waves(p, r0, n0, nwaves=2, library=library, w2_body=True), ora)
    assert _violations(library) == 0
