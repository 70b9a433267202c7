"""CPU tier: the oracle (C restatement) against the golden vectors cut from the REFERENCE binary.
The oracle is pinned bit for bit: trajectories, residuals, counts and stop flags."""
import numpy as np
import pytest

from tests import oracle_lib
from tests.common import (GOLDEN_CASES, assert_matches_golden, host_libm_is_the_variant_the_fixtures_were_cut_with,
                          load_golden, stop_codes)

RK4_CASES = [n for n in GOLDEN_CASES if "_rk4" in n]
# stop flags that trace_rays decides between two steps (ray_tracing.f90:128-172), not inside one
OUTSIDE_THE_STEP = ("sout > s_max", " nstep > nstep_max")


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_bitwise_equals_reference(name):
    g, nml, p = load_golden(name)
    out = oracle_lib.trace(p, g["rvec0"], g["rindex_vec0"])
    assert_matches_golden(out, g, p, exact=True, calls_host_libm=True)


@pytest.mark.parametrize("name", ["cfg1_slab16_rk4", "cfg2_solovev1024_rk4", "gold_axisym64_eqdsk_damp_rk4"])
def test_oracle_rhs_pieces_equal_reference_probes(name):
    """equilibrium + deriv_cold + deriv_num + eqn_ray + check_save residual, state by state."""
    g, nml, p = load_golden(name)
    for rec in g["probes"][::4]:
        o = oracle_lib.probe(p, rec["v"])
        keys = ("eq", "cold", "num", "dvds") if p.nv == 7 else ("eq", "cold", "num")
        for key in keys:
            assert np.array_equal(o[key], rec[key], equal_nan=True), key
        assert o["resid"] == rec["resid"] or (np.isnan(o["resid"]) and np.isnan(rec["resid"]))


def _s_of_point(p, n):
    """s of recorded point k as trace_rays accumulates it: sout = sout + ds, k times (ray_tracing.f90:118-121)."""
    return np.concatenate([[0.0], np.cumsum(np.full(n, float(p.ds)))])


def test_the_rk4_fixtures_are_the_ones_named_so():
    for name in GOLDEN_CASES:
        g, nml, p = load_golden(name)
        assert (p.ode_solver == 0) == (name in RK4_CASES), name


@pytest.mark.parametrize("name", RK4_CASES)
def test_oracle_step_is_the_references_next_point(name):
    """oracle_lib.step (RK4_ode + check_save from an arbitrary state) pinned to the reference-generated fixtures:
    from EVERY recorded point k of every ray it returns point k + 1 and its residual bit for bit and does not stop;
    from a ray's last recorded point it stops with the ray's stop flag, for every ray whose end is decided inside a step."""
    g, nml, p = load_golden(name)
    ref, res, npts = g["ray_vec"], g["residual"], g["npoints"].astype(np.int64)
    nmax = ref.shape[1]
    s_tab = _s_of_point(p, nmax)
    has_next = np.arange(nmax - 1)[None, :] < (npts - 1)[:, None]          # [ray][k]: point k has a successor
    kk = np.broadcast_to(np.arange(nmax - 1)[None, :], has_next.shape)[has_next]
    assert has_next.sum() == (npts - 1).sum() > 0
    v1, resid, code, stopped = oracle_lib.step(p, ref[:, :-1][has_next], s_tab[kk])
    want, want_res = ref[:, 1:][has_next], res[:, 1:][has_next]
    assert not stopped.any(), f"{int(stopped.sum())} recorded steps come back stopped (codes {set(code[stopped])})"
    if host_libm_is_the_variant_the_fixtures_were_cut_with():
        np.testing.assert_array_equal(v1, want)
        np.testing.assert_array_equal(resid, want_res)
    else:   # the documented bars of tests.common.assert_matches_golden, per step
        for sl in (slice(0, 3), slice(3, 6)):
            num, den = np.linalg.norm(v1[:, sl] - want[:, sl], axis=-1), np.linalg.norm(want[:, sl], axis=-1)
            assert (num <= 1e-10 * den).all()
        np.testing.assert_allclose(resid, want_res, rtol=0, atol=1e-12)
    # ---- each ray's last recorded point ----
    rays = np.arange(len(npts))
    v1, resid, code, stopped = oracle_lib.step(p, ref[rays, npts - 1], s_tab[npts - 1])
    inside = np.array([str(f) not in OUTSIDE_THE_STEP for f in g["stop_flag"]])
    assert stopped[inside].all(), f"rays {rays[inside & ~stopped]} end inside a step in the fixture but not for step()"
    np.testing.assert_array_equal(code[inside], stop_codes(g["stop_flag"])[inside])


def test_oracle_step_edges():
    g, nml, p = load_golden("cfg1_slab16_rk4")
    v1, resid, code, stopped = oracle_lib.step(p, np.zeros((0, p.nv)))
    assert v1.shape == (0, p.nv) and resid.shape == code.shape == stopped.shape == (0,)
    # s0 = None is s = 0: the first step of every ray
    a = oracle_lib.step(p, g["ray_vec"][:, 0])
    b = oracle_lib.step(p, g["ray_vec"][:, 0], np.zeros(len(g["ray_vec"])))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[0], g["ray_vec"][:, 1])
    # the thread count does not enter the result
    c = oracle_lib.step(p, g["ray_vec"][:, 0], nthreads=1)
    np.testing.assert_array_equal(a[0], c[0])
    # Shampine-Gordon: a restarted output step is not the reference's next step -- refused, not approximated
    g, nml, p = load_golden("gold_solovev64_sg_cold")
    with pytest.raises(RuntimeError, match="RK4 only"):
        oracle_lib.step(p, g["ray_vec"][:, 0])


def test_oracle_full_counts():
    """All 1024 rays of cfg2: npoints and stop flags of every ray equal the reference's."""
    g, nml, p = load_golden("cfg2_solovev1024_rk4")
    out = oracle_lib.trace(p, g["rvec0_full"], g["rindex_vec0_full"])
    np.testing.assert_array_equal(out["npoints"], g["npoints_full"])
    np.testing.assert_array_equal(out["stop_code"], stop_codes(g["stop_flag_full"]))
    # summary conventions (ray_tracing.f90:255-256)
    r = 5
    n = out["npoints"][r]
    assert out["end_residuals"][r] == out["residual"][r, n - 2]
    assert out["max_residuals"][r] == np.abs(out["residual"][r, :n - 1]).max()


def test_oracle_edge_cases():
    g, nml, p = load_golden("cfg1_slab16_rk4")
    # empty fan
    out = oracle_lib.trace(p, np.zeros((0, 3)), np.zeros((0, 3)))
    assert out["npoints"].shape == (0,)
    # a ray launched outside the box never records a step.  (The reference's initial check_save
    # reads an undefined eq_point here; our defined behaviour evaluates the fields at the point,
    # which fails the dispersion-residual test -> 'dispersion_residual', npoints = 1.)
    r0 = g["rvec0"][:1].copy()
    r0[0, 0] = 10.0
    out = oracle_lib.trace(p, r0, g["rindex_vec0"][:1])
    assert out["npoints"][0] == 1 and out["stop_code"][0] in (10, 40, 41)
    assert not out["end_ray_vec"][0].any()  # summary fields stay zero (ray_tracing.f90:101-112)
    # nstep_max = 0: first trajectory trip stops with ' nstep > nstep_max'
    from rays_amd.params import copy_params
    q = copy_params(p)
    q.nstep_max = 0
    out = oracle_lib.trace(q, g["rvec0"][:2], g["rindex_vec0"][:2])
    assert (out["npoints"] == 1).all() and (out["stop_code"] == 2).all()
    # s_max smaller than one step
    q = copy_params(p)
    q.s_max = 0.5 * p.ds
    out = oracle_lib.trace(q, g["rvec0"][:2], g["rindex_vec0"][:2])
    assert (out["npoints"] == 1).all() and (out["stop_code"] == 1).all()
