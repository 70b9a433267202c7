"""CPU tier: the adjoint form of dD/dalpha_s and dD/dgamma_s that the tolerance flavour of deriv_cold evaluates
(rays_amd/csrc/rays_cold_adjoint.inc, compiled for the host by tests/hip_emul/emul_cold_adjoint.cpp) against the
reference-order expressions (deriv_cold.f90:104-112, :152-154) on the same intermediates p, t, u, q, du/da .. dq/dg.

Both forms sum the same monomials -- eleven for dD/dalpha_s, eight for dD/dgamma_s -- and every monomial passes through
fewer than 32 roundings on any path of either form, so

    |adjoint - reference| <= 32 * 2**-53 * (sum of the absolute values of the expanded monomials)

is a forward-error bound, not a measured figure.  Species counts 1, 2, 3, 4, 6; random physical inputs and the edge
inputs alpha = 0, a gamma within 1e-8 of 1, n1 = 0, n3 = 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(ROOT, "tests", "hip_emul")
_LIB = os.path.join(_DIR, "librays_emul_cold_adjoint.so")
BOUND = 32.0 * 2.0 ** -53
NS_LIST = (1, 2, 3, 4, 6)
N_RANDOM = 2000


@pytest.fixture(scope="module")
def adjoint():
    srcs = [os.path.join(_DIR, "emul_cold_adjoint.cpp"), os.path.join(ROOT, "rays_amd", "csrc", "rays_cold_adjoint.inc")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-w",
                               srcs[0], "-o", _LIB])
    lib = C.CDLL(_LIB)
    dp = C.POINTER(C.c_double)
    fn = lib.rays_emul_cold_adjoint
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] + [C.c_double] * 6 + [dp] * 7

    def call(I):
        """ddda, dddg [n][ns] of the adjoint form, sample by sample"""
        n, ns = I["duda"].shape
        ddda, dddg = np.zeros((n, ns)), np.zeros((n, ns))
        tabs = [np.ascontiguousarray(I[k]) for k in ("duda", "dqda", "dtdg", "dudg", "dqdg")]
        d = lambda a, i: a[i].ctypes.data_as(dp)
        for i in range(n):
            rc = fn(ns, I["p"][i], I["t"][i], I["u"][i], I["q"][i], I["n1_2"][i], I["n3_2"][i],
                    *(d(a, i) for a in tabs), d(ddda, i), d(dddg, i))
            assert rc == 0
        return ddda, dddg
    return call


def intermediates(alpha, gamma, n1, n3):
    """deriv_cold.f90:78-149 in the reference's order; alpha, gamma [n][ns], n1, n3 [n]"""
    n, ns = alpha.shape
    p = 1. - alpha.sum(axis=1)
    t = np.ones(n)
    for s in range(ns):
        t = t * (1. - gamma[:, s] ** 2)
    dq1da, dq2da = np.ones((n, ns)), np.ones((n, ns))
    for s1 in range(ns):
        for s in range(ns):
            if s != s1:
                dq1da[:, s1] = dq1da[:, s1] * (1. + gamma[:, s])
                dq2da[:, s1] = dq2da[:, s1] * (1. - gamma[:, s])
    q1 = (alpha * dq1da).sum(axis=1)
    q2 = (alpha * dq2da).sum(axis=1)
    u = t - (alpha * dq1da * dq2da).sum(axis=1)
    q = 2. * u - t + q1 * q2
    duda = -dq1da * dq2da
    dqda = 2. * duda + dq1da * q2[:, None] + q1[:, None] * dq2da
    gp, gm = np.ones((n, ns, ns)), np.ones((n, ns, ns))
    for s1 in range(ns):
        for s2 in range(ns):
            for s in range(ns):
                if s != s1 and s != s2:
                    gp[:, s1, s2] = gp[:, s1, s2] * (1. + gamma[:, s])
                    gm[:, s1, s2] = gm[:, s1, s2] * (1. - gamma[:, s])
    gpm = gp * gm
    dtdg = 2. * gamma * duda
    a = np.einsum("nj,njs->ns", alpha, gpm)
    b = np.einsum("nj,njs->ns", alpha, gp)
    c = np.einsum("nj,njs->ns", alpha, gm)
    dudg = dtdg + 2. * gamma * (a + alpha * duda)
    dq1dg = b - alpha * dq1da
    dq2dg = -c + alpha * dq2da
    dqdg = 2. * dudg - dtdg + dq1dg * q2[:, None] + q1[:, None] * dq2dg
    return dict(p=p, t=t, u=u, q=q, n1=n1, n3=n3, n1_2=n1 * n1, n3_2=n3 * n3, duda=duda, dqda=dqda, dtdg=dtdg, dudg=dudg,
                dqdg=dqdg)


def reference_order(I):
    """:104-112 and :152-154 as written (x**4 sequentially, as flang lowers it), and the sums of |monomial|"""
    col = lambda k: I[k][:, None]
    p, t, u, q, n1, n3 = (col(k) for k in ("p", "t", "u", "q", "n1", "n3"))
    duda, dqda, dtdg, dudg, dqdg = (I[k] for k in ("duda", "dqda", "dtdg", "dudg", "dqdg"))
    n3_2, n3_4, n1_2, n1_4 = n3 * n3, ((n3 * n3) * n3) * n3, n1 * n1, ((n1 * n1) * n1) * n1
    ddda = -t * n3_4 + (2. * (u - p * duda) + (-t + duda) * n1_2) * n3_2 - q + \
        p * dqda - (dqda - u + p * duda) * n1_2 + duda * n1_4
    dddg = dtdg * p * n3_4 + (-2. * p * dudg + (dtdg * p + dudg) * n1_2) * n3_2 + \
        p * dqdg - (dqdg + p * dudg) * n1_2 + dudg * n1_4
    mono_a = [t * n3_4, 2. * u * n3_2, 2. * p * duda * n3_2, t * n1_2 * n3_2, duda * n1_2 * n3_2, q + 0. * duda, p * dqda,
              dqda * n1_2, u * n1_2 + 0. * duda, p * duda * n1_2, duda * n1_4]
    mono_g = [dtdg * p * n3_4, 2. * p * dudg * n3_2, dtdg * p * n1_2 * n3_2, dudg * n1_2 * n3_2, p * dqdg, dqdg * n1_2,
              p * dudg * n1_2, dudg * n1_4]
    return ddda, dddg, sum(np.abs(m) for m in mono_a), sum(np.abs(m) for m in mono_g)


def physical_inputs(ns, n, seed):
    """electrons first: alpha_e up to past the cutoff, |gamma_e| round the resonance; ions lighter in both by the mass
    ratio; index components of a propagating wave"""
    rng = np.random.default_rng(seed)
    alpha, gamma = np.zeros((n, ns)), np.zeros((n, ns))
    alpha[:, 0] = rng.uniform(0., 1.5, n)
    gamma[:, 0] = -rng.uniform(0.2, 3.0, n)
    for s in range(1, ns):
        ratio = 1. / (1836. * rng.uniform(1., 4., n))
        alpha[:, s] = alpha[:, 0] * ratio * rng.uniform(0.1, 1., n)
        gamma[:, s] = -gamma[:, 0] * ratio
    return alpha, gamma, rng.uniform(0., 1.5, n), rng.uniform(-1.5, 1.5, n)


def check(adjoint, alpha, gamma, n1, n3):
    I = intermediates(alpha, gamma, n1, n3)
    ddda_r, dddg_r, sa, sg = reference_order(I)
    ddda, dddg = adjoint(I)
    assert np.isfinite(ddda_r).all() and np.isfinite(dddg_r).all()
    ra = np.abs(ddda - ddda_r) - BOUND * sa
    rg = np.abs(dddg - dddg_r) - BOUND * sg
    print(f"ns {alpha.shape[1]}: worst |difference| / sum|monomials| dD/dalpha {np.max(np.abs(ddda - ddda_r) / np.maximum(sa, 1e-300)):.2e}, "
          f"dD/dgamma {np.max(np.abs(dddg - dddg_r) / np.maximum(sg, 1e-300)):.2e} (bound {BOUND:.2e})")
    assert (ra <= 0.).all(), f"dD/dalpha: sample {np.argmax(ra.max(axis=1))} exceeds the bound by {ra.max():.3e}"
    assert (rg <= 0.).all(), f"dD/dgamma: sample {np.argmax(rg.max(axis=1))} exceeds the bound by {rg.max():.3e}"
    return ddda, dddg, ddda_r, dddg_r


@pytest.mark.parametrize("ns", NS_LIST)
def test_random_physical_inputs(adjoint, ns):
    check(adjoint, *physical_inputs(ns, N_RANDOM, seed=100 + ns))


@pytest.mark.parametrize("ns", NS_LIST)
def test_edge_inputs(adjoint, ns):
    """each edge alone on 64 random samples, then all four together"""
    n = 64
    alpha, gamma, n1, n3 = physical_inputs(ns, 5 * n, seed=200 + ns)
    near_one = 1. + np.random.default_rng(300 + ns).uniform(-1e-8, 1e-8, n)
    alpha[0 * n:1 * n] = 0.                 # no plasma: D_p, D_u, D_q do not vanish, the species' own tables do
    gamma[1 * n:2 * n, 0] = -near_one       # the electron cyclotron resonance: t -> 0
    n1[2 * n:3 * n] = 0.                    # parallel propagation
    n3[3 * n:4 * n] = 0.                    # perpendicular propagation
    alpha[4 * n:] = 0.
    gamma[4 * n:, 0] = -near_one
    n1[4 * n:] = 0.
    n3[4 * n:] = 0.
    ddda, dddg, ddda_r, dddg_r = check(adjoint, alpha, gamma, n1, n3)
    # alpha = 0, n = 0: D = t * 0 + p q with p = 1, q = t: dD/dalpha_s = dq/dalpha_s - q in both forms, to the bit
    np.testing.assert_array_equal(ddda[4 * n:], ddda_r[4 * n:])
    np.testing.assert_array_equal(dddg[4 * n:], dddg_r[4 * n:])


def test_the_two_forms_are_not_the_same_code(adjoint):
    """the comparison is not vacuous: on random inputs the two forms differ in the last places somewhere"""
    I = intermediates(*physical_inputs(2, 256, seed=7))
    ddda_r, dddg_r, _, _ = reference_order(I)
    ddda, dddg = adjoint(I)
    assert (ddda != ddda_r).any() or (dddg != dddg_r).any()
