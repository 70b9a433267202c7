"""CPU tier: one iteration of the one-wave-per-SIMD RK4 trace kernel's wave loop is one STEP (rays_rk4_body.inc: a counted
loop over the evaluations of stage 3, 0, 1, 2; the pass over idle lanes is asked for once per step; a step whose lanes have
all stopped is left by a scalar branch); the two-waves build keeps one evaluation per iteration and runs the same cases.
The wave emulator (64 lanes as fibers) runs the sources built with -DRAYS_EMUL_CHECK_UNIFORM_STAGE: every lane under way
must be at the stage of the copy of the loop body it is in, the outputs are the oracle's bit for bit, and what the batching
threshold sees -- alive_sum per step, `occupied`, the running idle_acc -- equals what the trip-by-trip state machine this
loop replaced gave (recorded once from that build: tests/golden/rk4_step_loop_threshold_log.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

from rays_amd.params import copy_params
from tests import group_emul_lib as ge
from tests import oracle_lib
from tests.common import load_golden

ARRAYS = ("npoints", "stop_code", "ray_vec", "residual", "end_ray_vec", "end_residuals", "max_residuals")
CHECK = "-DRAYS_EMUL_CHECK_UNIFORM_STAGE"
# the libraries tests/test_cpu_rk4_uniform_stage.py builds (same tags, same switches: one compilation serves both files)
VARIANTS = {"stagecheck": [CHECK], "stagecheck_cost0": [CHECK, "-DRAYS_REFILL_EVENT_COST=0"]}


def _lib(variant="stagecheck"):
    library = ge.lib_variant(variant, VARIANTS[variant])
    for fn, args in (("rays_emul_uniform_stage_violations", []), ("rays_emul_early_step_exits", []),
                     ("rays_emul_threshold_log", [C.c_int])):
        getattr(library, fn).restype = C.POINTER(C.c_int)
        getattr(library, fn).argtypes = args
    return library


def _violations(library):
    return int(library.rays_emul_uniform_stage_violations()[0])


def _early_exits(library):
    return int(library.rays_emul_early_step_exits()[0])


def _check(out, ora):
    for k in ARRAYS:
        np.testing.assert_array_equal(out[k], ora[k], err_msg=k)


def _tiled(g, n):
    reps = -(-n // len(g["rvec0_full"]))
    return np.tile(g["rvec0_full"], (reps, 1))[:n].copy(), np.tile(g["rindex_vec0_full"], (reps, 1))[:n].copy()


@pytest.mark.parametrize("w2_body", [False, True], ids=["one_wave_body", "w2_body"])
@pytest.mark.parametrize("name", ["gold_slab_box_exits_rk4", "gold_solovev_evanescent_rk4", "gold_slab_negative_dens_rk4"])
def test_stages_refuse_next_to_lanes_that_go_on(name, w2_body):
    """Rays that a stage of a step refuses (box exit, evanescence, negative density: stage 0, 1 or 2 stops the lane, which
    parks with its code) in one wave with neighbours that go on, 70 rays on 64 lanes so that a pass also refills."""
    g, nml, p = load_golden(name)
    r0, n0 = _tiled(g, 70)
    ora = oracle_lib.trace(p, r0, n0)
    assert len(set(ora["npoints"].tolist())) > 1, "every ray of the wave ends on the same step"
    library = _lib()
    _check(ge.trace_rk4_waves(p, r0, n0, nwaves=1, library=library, w2_body=w2_body), ora)
    assert _violations(library) == 0


@pytest.mark.parametrize("w2_body", [False, True], ids=["one_wave_body", "w2_body"])
def test_the_last_lanes_stop_mid_step_and_the_wave_leaves_the_step(w2_body):
    """64 copies of ONE ray that a middle stage refuses: the wave's last lanes all stop on the same evaluation, which is
    not the step's last, and the scalar branch skips the rest of the step (the body of the two-waves build runs one
    evaluation per iteration and goes straight to its pass: same results, nothing to count)."""
    g, nml, p = load_golden("gold_slab_box_exits_rk4")
    ora_all = oracle_lib.trace(p, g["rvec0_full"], g["rindex_vec0_full"])
    library = _lib()
    found = 0
    for r in np.flatnonzero(ora_all["npoints"] > 1):
        r0, n0 = np.repeat(g["rvec0_full"][r:r + 1], 64, axis=0), np.repeat(g["rindex_vec0_full"][r:r + 1], 64, axis=0)
        before = _early_exits(library)
        out = ge.trace_rk4_waves(p, r0, n0, nwaves=1, library=library, w2_body=w2_body)
        _check(out, oracle_lib.trace(p, r0, n0))
        found += _early_exits(library) > before
    assert w2_body or found >= 1, "no ray of the fixture stops at stage 0, 1 or 2"
    assert _violations(library) == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("w2_body,stride", [(False, 0), (False, 4), (True, 0)], ids=["stride0", "stride4", "w2_body"])
def test_more_rays_than_lanes_join_lanes_under_way(variant, w2_body, stride):
    """130 rays of the Solovev fan on one 64-lane wave: passes start fresh rays (at stage 3, the first evaluation of a step)
    next to lanes that are under way; with RAYS_REFILL_EVENT_COST=0 at the first step that has an idle lane."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    q = copy_params(p)
    q.nstep_max = 120
    r0, n0 = g["rvec0_full"][::7][:130].copy(), g["rindex_vec0_full"][::7][:130].copy()
    n0[3] *= 3.0   # stops at its initial check
    ora = oracle_lib.trace(q, r0, n0)
    assert len(set(ora["npoints"].tolist())) > 5
    library = _lib(variant)
    _check(ge.trace_rk4_waves(q, r0, n0, nwaves=1, library=library, stride=stride, w2_body=w2_body), ora)
    assert _violations(library) == 0


@pytest.mark.parametrize("w2_body", [False, True], ids=["one_wave_body", "w2_body"])
def test_nstep_max_and_s_max_stop_on_the_step_they_fall_on(w2_body):
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::11][:70], g["rindex_vec0_full"][::11][:70]
    library = _lib()
    for nstep_max, s_max in ((7, None), (1, None), (1000, 5.5 * float(p.ds)), (1000, 0.5 * float(p.ds))):
        q = copy_params(p)
        q.nstep_max = nstep_max
        if s_max is not None:
            q.s_max = s_max
        ora = oracle_lib.trace(q, r0, n0)
        assert ora["npoints"].max() <= 8
        _check(ge.trace_rk4_waves(q, r0, n0, nwaves=1, library=library, w2_body=w2_body), ora)
    assert _violations(library) == 0


@pytest.mark.parametrize("case", ["stride0", "stride4", "w2_body"])
def test_the_batching_threshold_sees_the_sums_it_saw_trip_by_trip(case):
    """The ragged 200-ray Solovev fan of test_cpu_rk4_uniform_stage.py on one wave: every time a step asks the threshold,
    (alive_sum of the step, occupied, idle_acc) is what the per-trip state machine accumulated over the four trips."""
    want = np.load(os.path.join(os.path.dirname(__file__), "golden", "rk4_step_loop_threshold_log.npz"))[case]
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"][::5][:200].copy(), g["rindex_vec0_full"][::5][:200].copy()
    n0[7] *= 3.0
    library = _lib()
    library.rays_emul_threshold_log(1)
    kw = dict(w2_body=True) if case == "w2_body" else dict(stride=int(case[6:]))
    _check(ge.trace_rk4_waves(p, r0, n0, nwaves=1, library=library, **kw), oracle_lib.trace(p, r0, n0))
    log = library.rays_emul_threshold_log(0)
    n = int(log[0])
    assert n == len(want) and n <= 4096
    got = np.array([log[1 + i] for i in range(3 * n)], dtype=np.int32).reshape(n, 3)
    np.testing.assert_array_equal(got, want)
    assert _violations(library) == 0
