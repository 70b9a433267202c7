"""GPU tier: the RK4 trace kernels with one wave-loop iteration per STEP (rays_rk4_body.inc) and the resume kernel that
follows the tolerance kernels (rays_rk4.hpp: rk4_resume_kernel).

  * fans of 1, 63, 64, 65 and 257 rays (less than a wave, a whole wave, a wave and a lane, more than a block) of the slab
    and the Solovev equilibrium, and one of 65536 + 64 rays with nstep_max = 8 (more rays than resident lanes: the pass
    refills): the exact flavour is the oracle's bit for bit, the tolerance flavour has its ray counts and stop codes and
    its points within the bars of tests/test_gpu_tolerance_flavour.py;
  * resume: states whose step the tolerance kernel hands over, arranged so that waves hold 1, 8, 9 and 64 of them and a
    wave with none sits between two that have some: what the resumed rays write is the exact kernel's, what the other
    rays write is what they write when no ray of the launch is handed over (the resume kernel then does nothing)."""
import functools
import os

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.namelist import read_namelist
from rays_amd.params import params_from_namelist
from rays_amd.ray_init import fan_from_namelist
from tests import oracle_lib
from tests.common import ROOT, load_golden

pytestmark = pytest.mark.gpu

ARRAYS = ("npoints", "stop_code", "ray_vec", "residual", "end_ray_vec", "end_residuals", "max_residuals")
ACCUMULATED_TOL = 1e-6   # tests/test_gpu_tolerance_flavour.py: over a whole ray
RESID_ATOL = 1e-9        # likewise
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture
def numerics(request):
    prev = hip.set_numerics(request.param)
    yield request.param
    hip.set_numerics(prev)


@functools.lru_cache(maxsize=None)
def _small_fan(eq):
    """257 rays and their oracle, computed once; the smaller fans are its leading rays (rays do not interact)."""
    if eq == "solovev":
        g, nml, p = load_golden("cfg2_solovev1024_rk4")
        r0, n0 = g["rvec0_full"][::3][:257].copy(), g["rindex_vec0_full"][::3][:257].copy()
        n0[5] *= 3.0   # stops at its initial check
    else:
        g, nml, p = load_golden("gold_slab_box_exits_rk4")
        reps = -(-257 // len(g["rvec0_full"]))
        r0, n0 = np.tile(g["rvec0_full"], (reps, 1))[:257].copy(), np.tile(g["rindex_vec0_full"], (reps, 1))[:257].copy()
    ora = oracle_lib.trace(p, r0, n0, nthreads=0)
    for a in (r0, n0, *ora.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p, r0, n0, ora


def _assert_flavour(out, ora, flavour, n=None):
    sl = slice(0, n)
    if flavour == "exact":
        for k in ARRAYS:
            np.testing.assert_array_equal(out[k], ora[k][sl], err_msg=k)
        return
    np.testing.assert_array_equal(out["npoints"], ora["npoints"][sl])
    np.testing.assert_array_equal(out["stop_code"], ora["stop_code"][sl])
    worst = 0.0
    for key in ("ray_vec", "end_ray_vec"):
        rv, ref = out[key], ora[key][sl]
        for c in (slice(0, 3), slice(3, 6)):
            num, den = np.linalg.norm(rv[..., c] - ref[..., c], axis=-1), np.linalg.norm(ref[..., c], axis=-1)
            m = den > 0
            if m.any():
                worst = max(worst, float((num[m] / den[m]).max()))
        # the other rows (ray parameter, absorbed power): relative to the row's magnitude
        for c in range(6, rv.shape[-1]):
            scale = max(float(np.abs(ref[..., c]).max()), 1e-300)
            worst = max(worst, float(np.abs(rv[..., c] - ref[..., c]).max()) / scale)
    print(f"tolerance flavour: worst deviation of a point {worst:.3e}")
    assert worst <= ACCUMULATED_TOL
    for key in ("residual", "end_residuals", "max_residuals"):
        assert np.abs(out[key] - ora[key][sl]).max() <= RESID_ATOL, key


@pytest.mark.parametrize("numerics", ["exact", "tolerance"], indirect=True)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("eq", ["slab", "solovev"])
def test_small_fans(eq, n, numerics):
    p, r0, n0, ora = _small_fan(eq)
    _assert_flavour(hip.trace_host(p, r0[:n], n0[:n], ngpu=1), ora, numerics, n)


@functools.lru_cache(maxsize=None)
def _refill_fan():
    nml = read_namelist(os.path.join(ROOT, "configs", "cfg3b_solovev64k_rk4.in"))
    nml["ode_list"].update(nstep_max=8)
    p = params_from_namelist(nml, None)
    fan, nray_max = fan_from_namelist(nml)
    r0, n0, _ = hip.ray_init_host(p, fan, nray_max)
    assert len(r0) == 65536
    r0, n0 = np.concatenate([r0, r0[:64]]), np.concatenate([n0, n0[:64]])
    return p, r0, n0, oracle_lib.trace(p, r0, n0, nthreads=0)


@pytest.mark.parametrize("numerics", ["exact", "tolerance"], indirect=True)
def test_fan_with_more_rays_than_resident_lanes(numerics):
    """65536 + 64 rays, eight steps each: the last 64 rays are started by a pass, next to or after the first ones."""
    p, r0, n0, ora = _refill_fan()
    assert hip.kernel_name(p, len(r0)).startswith("rk4_trace_kernel<"), "not the one-wave-per-SIMD kernel"
    _assert_flavour(hip.trace_host(p, r0, n0, ngpu=1), ora, numerics)


def test_resume_kernel_with_1_8_9_and_64_handed_over_rays_in_a_wave():
    """ode_step restarts states under the tolerance flavour; a state one step before the end of a ray that runs into the
    mode coalescence is handed over to rk4_resume_kernel (tests/test_gpu_tolerance_flavour.py:
    test_handed_over_steps_are_the_references_bit_for_bit), a state in the middle of a ray is not.  The library launches
    the resume kernel right behind the trace kernel and shows no state in between, so "the rays that were not handed over
    are untouched by the resume launch" is checked against a launch of the same states in which NO ray is handed over
    (every wave of the resume kernel then leaves at once): a resume kernel that wrote to another ray would show."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    r0, n0 = g["rvec0_full"], g["rindex_vec0_full"]
    ora = oracle_lib.trace(p, r0, n0, nthreads=0)
    npts = ora["npoints"].astype(np.int64)
    rays = np.flatnonzero(npts >= 40)
    n = npts[rays]
    s_tab = np.concatenate([[0.0], np.cumsum(np.full(int(n.max()), float(p.ds)))])
    last_v, last_s = ora["ray_vec"][rays, n - 2], s_tab[n - 2]
    mid_v, mid_s = ora["ray_vec"][rays, n // 2], s_tab[n // 2]

    def step(flavour, v, s):
        prev = hip.set_numerics(flavour)
        try:
            return hip.ode_step(p, v, s)
        finally:
            hip.set_numerics(prev)

    # the last steps the tolerance flavour hands over come back as the exact kernel's (and the oracle's) bit for bit
    tol, ex = step("tolerance", last_v, last_s), step("exact", last_v, last_s)
    handed = np.flatnonzero((tol[0] == ex[0]).all(axis=1) & (ex[0] == ora["ray_vec"][rays, n - 1]).all(axis=1) & (tol[2] == 0))
    assert len(handed) >= 82, f"only {len(handed)} handed-over last steps in the fan"
    # lanes of the handed-over states: wave 0 one, wave 1 eight, wave 2 none, wave 3 nine, wave 4 all 64
    lanes = np.concatenate([[17], 64 + np.arange(8) * 7 + 3, 192 + np.arange(9) * 7, 256 + np.arange(64)])
    assert [int(((lanes // 64) == w).sum()) for w in range(5)] == [1, 8, 0, 9, 64]
    v, s = mid_v[:320].copy(), mid_s[:320].copy()
    plain = step("tolerance", v, s)             # no state of this launch is handed over
    assert any((a != b).any() for a, b in zip(plain, step("exact", v, s))), "the flavours do not differ on these states"
    v[lanes], s[lanes] = last_v[handed[:82]], last_s[handed[:82]]
    tol, ex = step("tolerance", v, s), step("exact", v, s)
    others = np.setdiff1d(np.arange(320), lanes)
    for a, b, c, what in zip(tol, ex, plain, ("v1", "resid", "stop_code")):
        np.testing.assert_array_equal(a[lanes], b[lanes], err_msg=f"{what} of the resumed rays")
        np.testing.assert_array_equal(a[others], c[others], err_msg=f"{what} of the rays that were not handed over")
    assert (tol[2] < 1000).all(), "the internal hand-over stop code reached the caller"
