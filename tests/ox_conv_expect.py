"""Cases and expected records of the O-X conversion analysis (include/rays_hip.h: rays_ox_result_t;
rays_amd/csrc/rays_oxconv.hpp) -- test infrastructure shared by the generator of tests/golden/ox_conv_cases.npz and
the CPU and GPU tiers.

The expected records follow the rule of tests/diag_expect.py: the reference's OWN eq_point records (oracle/_ref/ref_states
= oracle/ref_states_driver.f90 on the reference's objects, handed in as the callable `eq_at`) and the formulae of
post_process_lib/OX_conv_analysis_m.f90 restated here in the reference's written order, on Python floats (IEEE binary64,
one operation at a time), with Python's `math` for acos / sin / cos / exp / pow -- the host libm the reference calls --
and norm2 / minval / dot_product as the reference's compiler evaluates them (held against a program of ours by
tests/test_cpu_ox_conv.py).  Nothing here runs the code under test.

Cases are a configs/<base>.in plus namelist overrides, the way tests/launch_cases.py does it."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from tests import launch_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join("tests", "golden", "ox_conv_cases.npz")

FOUND_MAX, FOUND_CUTOFF, CONVERTED, EQ_REFUSED = 1, 2, 4, 8      # RAYS_OX_* of include/rays_hip.h
PI = float(np.float32(3.1415926535897932385))                     # constants_m.f90:39: a default-real literal
THRESHOLD = float(np.float32(0.0001))                             # OX_conv_analysis_m.f90:32, likewise
ALPHA_TOLERANCE = 1.0 / 10.0 ** 4                                 # :274
MAX_ITERATIONS = 10                                               # :275
CHUNK = 64                                                        # points per wave of the scan kernel

INT_FIELDS = ("status", "step_number", "iterations")
VEC_FIELDS = ("x_max", "k_max", "x_cut", "nvecx_c", "nvecy_c", "nvecz_c")
EXACT_FIELDS = ("alpha_max", "x_max", "k_max", "x_cut", "nvecx_c", "nvecy_c", "nvecz_c", "aux")   # bit-identical on the device
FLOAT_FIELDS = ("alpha_max", "conv_coeff") + VEC_FIELDS + ("aux",)
AUX = ("cos_theta", "gamma", "L", "ny_c", "nz_c")

# ---- cases -------------------------------------------------------------------------------------------------------------
SLAB_OX = {
    "species_list": dict(n0=1.2e20),
    "damping_list": dict(damping_model="no_damp"),
    "slab_eq_list": dict(bz_prof_model="constant", bz0=2.0, Ln_scale=0.5),
    "simple_slab_ray_init_list": dict(x_launch0=-0.45, n_ky_launch=3, delta_rindex_y0=0.02, n_kz_launch=16, rindex_z0=0.555,
                                      delta_rindex_z0=0.008),
    "ode_list": dict(nstep_max=600, ds=2e-11),
    "rf_list": dict(wave_mode="plus"),
}
SLAB_X = dict(SLAB_OX, rf_list=dict(wave_mode="minus"))

# T: traced fans (the reference's own trace, oracle/_ref/rays_ref_dump); S: hand-made rays on T.slab_ox's parameters
CASES = [
    lc.Case("T.slab_ox", "T", "gold_slab16_damp_rk4", SLAB_OX),
    lc.Case("T.slab_x", "T", "gold_slab16_damp_rk4", SLAB_X),
    # T.curved: an overdense plasma (alpha = 1.5 on the axis) and an O-mode fan around the optimal toroidal index, with
    # a step that puts the first decrease on both sides of point 64 -- the Solovev equilibrium, and axisym_toroid with the
    # eqdsk splines (the lookups from global memory)
    lc.Case("T.curved_solovev", "T", "cfg2_solovev1024_rk4", {
        "species_list": dict(n0=1.5e20), "rf_list": dict(wave_mode="plus"),
        "solovev_ray_init_nphi_ktheta_list": dict(n_rindex_theta=2, rindex_theta0=-0.01, delta_rindex_theta=0.02,
                                                  n_rindex_phi=6, rindex_phi0=0.30, delta_rindex_phi=0.02),
        "ode_list": dict(nstep_max=300, ds=1.4e-11)}),
    lc.Case("T.curved_axisym", "T", "gold_axisym64_eqdsk_damp_rk4", {
        "species_list": dict(n0=1.5e20), "rf_list": dict(wave_mode="plus"), "damping_list": dict(damping_model="no_damp"),
        "axisym_toroid_ray_init_R_Z_nphi_ntheta_list": dict(n_rindex_theta=2, rindex_theta0=-0.01, delta_rindex_theta=0.02,
                                                            n_rindex_phi=6, rindex_phi0=0.53, delta_rindex_phi=0.03),
        "ode_list": dict(nstep_max=400, ds=5.5e-12)}),
    lc.Case("S.synthetic", "S", "gold_slab16_damp_rk4", SLAB_OX),
    lc.Case("S.capped", "S", "gold_slab16_damp_rk4", dict(SLAB_OX, species_list=dict(n0=0.9e20))),   # see capped_rays
]
BY_NAME = {c.name: c for c in CASES}


def namelist_text(case):
    return lc.namelist_text(case)


def load_params(name):
    """(params, host tables or None) of a case, the tables attached to the libraries the tests use"""
    from rays_amd.namelist import parse_namelist
    from rays_amd.params import params_from_namelist
    case = BY_NAME[name]
    g = np.load(os.path.join(ROOT, "tests", "golden", case.base + ".npz"), allow_pickle=False)
    tab = {k[4:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("axi_")}
    if any(np.size(tab.get(k, ())) for k in ("r_grid", "ne_grid", "te_grid", "ti_grid")):
        # the base's host-built spline tables, for the C oracle and the library (the emulation of this analysis takes
        # them per call: emul_ox_conv(tab=...))
        from rays_amd import hip
        from tests import oracle_lib
        oracle_lib.set_axisym_tables(tab)
        hip.set_axisym_tables(tab)
    nml = parse_namelist(str(load_fixture(name)["namelist"]))     # the fixture's own parameters
    return params_from_namelist(nml, tab or None), (tab or None)


# ---- the intrinsics as the reference's compiler evaluates them -----------------------------------------------------------
def norm2(x):
    """flang's runtime Norm2: a running maximum m and the sum s of the squares of the other elements over m, rescaled
    when the maximum changes; m * sqrt(1 + s).  (Its compensated summation adds nothing for three elements or fewer.)"""
    m, s = 0.0, 0.0
    for t in x:
        a = abs(float(t))
        if m == 0.0:
            m = a
        elif a > m:
            q = m / a
            q2 = q * q
            s = s * q2
            s = s + q2
            m = a
        else:
            q = _div(a, m)
            s = s + q * q
    return m * math.sqrt(1.0 + s)


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)"""
    return float(np.float64(a) / np.float64(b))


def minval2(a, b):
    """minval((/a, b/)), inline: a unless b < a or (a is NaN and b is not)"""
    return b if (b < a or (a != a and b == b)) else a


def dot3(a, b):
    """dot_product, inline: ((0 + a1*b1) + a2*b2) + a3*b3"""
    return ((0.0 + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    """vectors3_m.f90:64-71"""
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


# ---- eq_point records (layout: oracle/ref_states_driver.f90 / rays_oracle_probe) -------------------------------------
def eq_fields(eq):
    eq = [float(t) for t in eq]
    return dict(bunit=eq[7:10], ns0=eq[28], gradns0=eq[29:32], alpha0=eq[38], gamma0=eq[39])


# ---- the module's three steps --------------------------------------------------------------------------------------------
def find_x_max(alpha, refused, npoints):
    """find_x_max_ray (:228-249) on a ray's alpha records: (status, step_number).  A refused point up to and including
    the one that shows the first decrease: EQ_REFUSED (defined here, not by the reference)."""
    if npoints >= 1 and refused[0]:
        return EQ_REFUSED, 0
    for j in range(1, npoints):                     # 0-based j = the reference's i - 1
        if refused[j]:
            return EQ_REFUSED, 0
        if alpha[j] < alpha[j - 1]:                 # :240
            return FOUND_MAX, j                     # :243 step_number = i - 1
    return 0, 0


def cutoff_step(x, e):
    """one iteration's step of find_x_cutoff_ray (:294-302) from x with the eq_point fields e at x"""
    with np.errstate(all="ignore"):
        gn = norm2(e["gradns0"])
        mod_grad_alpha = gn * _div(e["alpha0"], e["ns0"])                # :296
        r = norm2(x[:2])                                                  # :298
        delta = _div(1.0 - e["alpha0"], mod_grad_alpha)                   # :299
        step = minval2(delta, 0.25 * r)                                   # :301
        return [x[i] + _div(e["gradns0"][i], gn) * step for i in range(3)]   # :297, :301-302


def conv_value(cos_theta, gamma, L, ny_c, nz_c, k0):
    """conv_coeff from its ingredients (:363, :387-394), libm through Python's math"""
    try:
        theta = math.acos(cos_theta)
        st, ct = math.sin(theta), math.cos(theta)
        n_crit = st * math.sqrt(gamma / (1.0 + gamma))
        den = (1.0 + gamma) * (ct * ct) + (st * st) / 2.0
        F = 0.5 * (1.0 + gamma) * math.sqrt(gamma) / math.pow(den, 1.5)
        G = 0.5 * math.sqrt(gamma) / math.sqrt(den)
        dz, ay = abs(nz_c) - n_crit, abs(ny_c)
        expo = -(PI * k0 * L * (F * (dz * dz) + G * (ay * ay)))
        return math.exp(expo), expo
    except (ValueError, ZeroDivisionError, OverflowError):
        return float("nan"), float("nan")


def coeff(e, k, k0):
    """OX_conv_coeff (:357-394) with the eq_point fields e at x_cut: dict of nvec*_c, aux, conv_coeff, exponent"""
    with np.errstate(all="ignore"):
        g = e["gradns0"]
        gn = norm2(g)
        xc = [_div(g[i], gn) for i in range(3)]                 # :359
        v = cross(e["bunit"], xc)                               # :360
        vn = norm2(v)
        yc = [_div(v[i], vn) for i in range(3)]                 # :361
        zc = cross(xc, yc)                                      # :362
        cos_theta = dot3(xc, e["bunit"])                        # :363
        gamma = abs(e["gamma0"])                                # :364
        L = _div(e["ns0"], gn)                                  # :365
        n_vertical = _div(dot3(k, xc), k0)                      # :379
        nz_c = _div(dot3(k, zc), k0)                            # :380
        ny_c = _div(dot3(k, yc), k0)                            # :381
    c, expo = conv_value(cos_theta, gamma, L, ny_c, nz_c, k0)
    return dict(nvecx_c=[n_vertical * t for t in xc], nvecy_c=[ny_c * t for t in yc], nvecz_c=[nz_c * t for t in zc],
                aux=[cos_theta, gamma, L, ny_c, nz_c], conv_coeff=c, exponent=expo)


def blank(nray):
    out = {k: np.zeros(nray, dtype=np.int32) for k in INT_FIELDS}
    out.update(alpha_max=np.zeros(nray), conv_coeff=np.zeros(nray), aux=np.zeros((nray, len(AUX))), exponent=np.zeros(nray))
    out.update({k: np.zeros((nray, 3)) for k in VEC_FIELDS})
    return out


def expected_records(k0, ray_vec, npoints, alpha, refused, eq_at):
    """analyze_OX_conv (:114-165) on the rays ray_vec[nray][npt][nv] with the alpha records alpha[nray][npt] / refused
    [nray][npt] of their points.  eq_at(x[n][3], k[n][3]) -> (refused[n], eq[n][neq]): the eq_point records of n points,
    called once per ascent iteration for all rays still under way (k only fills the states' wave vector).
    Returns the result arrays plus `exponent` (the argument of exp, for the tolerance) and the converted list."""
    nray = len(npoints)
    out = blank(nray)
    x, k, it = {}, {}, {}
    for r in range(nray):
        status, step = find_x_max(alpha[r], refused[r], int(npoints[r]))
        out["status"][r] = status
        if status == FOUND_MAX:
            out["step_number"][r] = step
            out["alpha_max"][r] = alpha[r][step - 1]
            out["x_max"][r] = ray_vec[r, step - 1, 0:3]
            out["k_max"][r] = ray_vec[r, step - 1, 3:6]
            x[r], k[r], it[r] = [float(t) for t in ray_vec[r, step - 1, 0:3]], [float(t) for t in ray_vec[r, step - 1, 3:6]], 1

    def refuse(r):
        for key in out:
            out[key][r] = 0
        out["status"][r] = EQ_REFUSED
        del x[r]

    def finish(r, e):
        out["status"][r] |= FOUND_CUTOFF
        out["iterations"][r] = it[r]
        out["x_cut"][r] = x[r]
        c = coeff(e, k[r], k0)
        for key in ("nvecx_c", "nvecy_c", "nvecz_c", "aux", "conv_coeff", "exponent"):
            out[key][r] = c[key]
        if c["conv_coeff"] > THRESHOLD:             # :154
            out["status"][r] |= CONVERTED
        del x[r]

    at_cutoff = set()
    alpha_temp = {}
    while x:                                        # one evaluation per ray under way: x(0), x(1), ...
        rays = sorted(x)
        bad, eqs = eq_at(np.array([x[r] for r in rays]), np.array([k[r] for r in rays]))
        for n, r in enumerate(rays):
            if bad[n]:
                refuse(r)
                continue
            e = eq_fields(eqs[n])
            if it[r] == 1:
                assert np.float64(e["alpha0"]).tobytes() == np.float64(out["alpha_max"][r]).tobytes(), "alpha at x_max"
                if abs(e["alpha0"] - 1.0) <= ALPHA_TOLERANCE:      # :289, first iteration
                    at_cutoff.add(r)
            if r in at_cutoff:
                finish(r, e)
                continue
            alpha_temp[r] = e["alpha0"]             # :295
            x[r] = cutoff_step(x[r], e)
            it[r] += 1
            if it[r] > MAX_ITERATIONS:              # :287: iteration = 11 after the loop, nothing found
                out["iterations"][r] = it[r]
                del x[r]
            elif abs(alpha_temp[r] - 1.0) <= ALPHA_TOLERANCE:      # :289: leaves with x_cut = the point just stepped to
                at_cutoff.add(r)
    out["converted"] = (np.flatnonzero(out["status"] & CONVERTED) + 1).astype(np.int32)   # 1-based ray numbers, in order
    return out


# ---- S.synthetic ------------------------------------------------------------------------------------------------------
def synthetic_rays(p, k_row):
    """About two dozen hand-made rays in T.slab_ox's plasma.  The density is linear in x, so alpha is monotone in x: a
    ray is a sequence of x values (y = 0.01, z = 0.1 j), every point carrying the wave vector k_row.
    Returns (names, ray_vec[nray][npt][nv], npoints)."""
    xmin, xmax = float(p.slab.xmin), float(p.slab.xmax)
    lo, hi = -0.30, -0.20                            # alpha about 0.52 .. 0.78: well below the cutoff

    def rise(n, a=lo, b=hi):                        # n strictly increasing values
        return [a + (b - a) * i / max(n - 1, 1) for i in range(n)]

    def fall(x0, n):
        return [x0 - 1e-3 * (i + 1) for i in range(n)]

    rays = []

    def add(name, xs):
        rays.append((name, [float(t) for t in xs]))

    for n in (1, 2, 63, 64, 65, 128):               # the first decrease between points (n | n + 1), 1-based
        up = rise(n)
        add(f"decrease_{n}_{n + 1}", up + fall(up[-1], 3))
    up = rise(129)
    add("decrease_at_the_end_of_130", up + fall(up[-1], 1))
    for n in (64, 65, 200):
        add(f"no_decrease_{n}", rise(n))
    add("npoints_0", [])
    add("npoints_1", [lo])
    add("npoints_2_rising", [lo, hi])
    up = rise(40)
    add("plateau_then_decrease", up + [up[-1]] * 30 + fall(up[-1], 3))         # equal is not `<`
    up = rise(63)
    add("plateau_across_the_chunk_edge", up + [up[-1]] * 4 + fall(up[-1], 2))
    # (near x = -0.45, where 1 + x/Ln is computed without rounding: two adjacent x give two different alpha)
    up = rise(30, -0.48, -0.45)
    add("adjacent_doubles_descending", up + [math.nextafter(up[-1], -1.0)] + rise(5))
    up = rise(20, lo, -0.28)
    add("second_larger_maximum", up + fall(up[-1], 3) + rise(30, -0.27, -0.10) + fall(-0.10, 3))   # the first wins
    up = rise(20)
    add("refused_after_the_decrease", up + fall(up[-1], 2) + [xmax + 0.25] + rise(4))             # outside the box
    add("refused_before_the_decrease", rise(10) + [xmin - 0.25] + rise(10, -0.19, -0.15) + fall(-0.15, 2))
    add("refused_first_point", [xmax + 0.25] + rise(10) + fall(hi, 2))
    up = rise(20)
    add("nan_before_the_decrease", up[:10] + [float("nan")] + up[10:] + fall(up[-1], 2))
    return rays


def capped_rays():
    """S.capped: the ascent that needs the cap on every step and is not done after 10 iterations.  The cap is a quarter
    of r = sqrt(x**2 + y**2) and the density rises along x, so a capped step shrinks |x| by a quarter where x < 0: in
    T.slab_ox's plasma (cutoff at x = -0.08, no plasma beyond x = -0.5) at most six steps are capped, whatever the
    start.  S.capped is that plasma with n0 = 0.9e20: the cutoff lies at x = +0.058, and from (1e-3, 0, z) every step
    is r/4 and GROWS by a quarter -- ten of them reach 1e-3 * 1.25**10 < 0.01.  The second ray starts at 2.5e-2, where
    the cap no longer binds after a few steps: the contrast."""
    return [("capped_ascent_not_found", [-2e-3, 0.0, 1e-3, 5e-4]), ("uncapped_contrast", [1e-2, 2.5e-2, 2e-2])]


def build_synthetic(p, k_row, x_cutoff, capped=False):
    """The rays of synthetic_rays plus the one that needs the cutoff's position x_cutoff (alpha(x_cutoff) = 1), or the
    rays of S.capped."""
    special_y = {}
    if capped:
        rays = capped_rays()
        special_y = {n: 0.0 for n, _ in rays}
    else:
        rays = synthetic_rays(p, k_row)
        near = x_cutoff - 2e-5 * abs(x_cutoff) - 1e-6   # |alpha - 1| of about 1e-5: inside the tolerance
        rays.append(("maximum_within_the_tolerance", [near - 0.05, near - 0.02, near, near - 0.01]))
    names = [n for n, _ in rays]
    npts = np.array([len(xs) for _, xs in rays], dtype=np.int32)
    npt = p.nstep_max + 1
    rv = np.zeros((len(rays), npt, p.nv))
    for r, (name, xs) in enumerate(rays):
        n = len(xs)
        rv[r, :n, 0] = xs
        rv[r, :n, 1] = special_y.get(name, 0.01)
        rv[r, :n, 2] = 0.1 * np.arange(n) / max(n, 1)
        rv[r, :n, 3:6] = k_row
        rv[r, :n, 6] = 1e-11 * np.arange(n)
    return names, rv, npts


# ---- the fixture ---------------------------------------------------------------------------------------------------------
_fixture = None


def load_fixture(name):
    """{key: array} of one case of tests/golden/ox_conv_cases.npz: ray_vec (clipped), npoints, alpha, refused, the
    expected result arrays, exponent, converted; S.synthetic also `names`"""
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, FIXTURE), allow_pickle=False)
    pre = name + ":"
    return {k[len(pre):]: _fixture[k] for k in _fixture.files if k.startswith(pre)}


def case_names():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, FIXTURE), allow_pickle=False)
    return [str(c) for c in _fixture["cases"]]


def padded(p, fx):
    """(params with nstep_max = the fixture's clipped length - 1, ray_vec[nray][npt][nv], npoints) -- what the tests feed"""
    from rays_amd.params import copy_params
    q = copy_params(p)
    q.nstep_max = fx["ray_vec"].shape[1] - 1
    return q, np.ascontiguousarray(fx["ray_vec"], dtype=np.float64), np.ascontiguousarray(fx["npoints"], dtype=np.int32)


def packed(ray_vec, npoints):
    """(ray_vec[total][nv], offsets[nray + 1]) of the padded arrays"""
    off = np.zeros(len(npoints) + 1, dtype=np.int64)
    off[1:] = np.cumsum(npoints)
    rows = [ray_vec[r, :n] for r, n in enumerate(npoints)]
    flat = np.concatenate(rows) if rows else np.zeros((0, ray_vec.shape[2]))
    return np.ascontiguousarray(flat, dtype=np.float64).reshape(-1, ray_vec.shape[2]), off


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def assert_records(got, fx, what, fields=None, conv="exact"):
    """An implementation's result arrays against a case's expected records.  Integers exact; the float fields bit for
    bit (NaN matching NaN); conv = "exact" | None (not compared).  Rays the fixture marks EQ_REFUSED are compared in
    their status alone."""
    want_status = fx["status"]
    refused = (want_status & EQ_REFUSED) != 0
    st = np.asarray(got["status"])
    if conv is None:                                 # CONVERTED follows conv_coeff
        st, want_status = st & ~CONVERTED, want_status & ~CONVERTED
    bad = np.flatnonzero(st != want_status)
    assert not len(bad), f"{what}: status differs on rays {bad[:8].tolist()}: got {st[bad[:8]].tolist()}, " \
                         f"want {want_status[bad[:8]].tolist()}"
    keep = ~refused
    for k in fields or (INT_FIELDS[1:] + EXACT_FIELDS + (("conv_coeff",) if conv == "exact" else ())):
        if k not in got or got[k] is None:
            continue
        g, w = np.asarray(got[k])[keep], fx[k][keep]
        if k in INT_FIELDS:
            ok = g == w
        else:
            g, w = g.astype(np.float64), w.astype(np.float64)
            ok = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
        if not ok.all():
            i = np.argwhere(~ok)[0]
            ray = int(np.flatnonzero(keep)[i[0]])
            raise AssertionError(f"{what}: {k} differs on {int((~ok).sum())} values; first at ray {ray} {tuple(i[1:])}: "
                                 f"got {g[tuple(i)]!r}, want {w[tuple(i)]!r}")


# ---- the emulated kernels (tests/hip_emul/emul_oxconv.cpp) -----------------------------------------------------------
class OxResult(C.Structure):
    """rays_ox_result_t (include/rays_hip.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("status", "step_number", "iterations", "alpha_max", "x_max", "k_max", "x_cut",
                                          "conv_coeff", "nvecx_c", "nvecy_c", "nvecz_c", "aux")]


def result_arrays(nray, sentinel=True):
    """host arrays of every field, sentinel-filled"""
    out = {k: np.full(nray, -77, dtype=np.int32) for k in INT_FIELDS}
    fill = np.nan if sentinel else 0.0
    out.update(alpha_max=np.full(nray, fill), conv_coeff=np.full(nray, fill), aux=np.full((nray, len(AUX)), fill))
    out.update({k: np.full((nray, 3), fill) for k in VEC_FIELDS})
    return out


def result_struct(arrays):
    return OxResult(**{k: (arrays[k].ctypes.data if arrays.get(k) is not None else None) for k, _ in OxResult._fields_})


_emul = {}


def emul_lib(path=None, directory=None):
    from rays_amd.params import AxisymTables, RaysParams
    from tests import emul_build as eb
    out = path or os.path.join(eb.DIR, "librays_emul_oxconv.so")
    if out not in _emul:
        eb.build("emul_oxconv.cpp", out, directory=directory or eb.DIR)
        lib = C.CDLL(out)
        vp = C.c_void_p
        lib.rays_emul_ox_conv.restype = C.c_int
        lib.rays_emul_ox_conv.argtypes = [C.POINTER(RaysParams), C.c_int, C.c_int, vp, vp, vp, C.POINTER(OxResult), C.c_int, vp, vp]
        lib.rays_emul_ox_set_axisym_tables.argtypes = [C.POINTER(AxisymTables), C.c_int, C.c_double, C.c_double]
        _emul[out] = lib
    return _emul[out]


def emul_set_tables(lib, tab):
    from rays_amd.params import axisym_tables_struct
    if tab and any(np.size(tab.get(k, ())) for k in ("r_grid", "ne_grid", "te_grid", "ti_grid")):
        t, keep = axisym_tables_struct(tab)
        lin = "lin_psi" in tab
        lib.rays_emul_ox_set_axisym_tables(C.byref(t), int(lin), float(tab["lin_dR"]) if lin else 0.0,
                                           float(tab["lin_dZ"]) if lin else 0.0)


def emul_ox_conv(p, ray_vec, npoints, host_finish=True, use_packed=False, lib=None, tab=None):
    """The two kernels on the host (scan on the wave emulator) and, host_finish, what rays_hip_ox_conv does behind them.
    Returns the result arrays plus `converted`."""
    lib = lib or emul_lib()
    emul_set_tables(lib, tab)
    nray = len(npoints)
    out = result_arrays(nray)
    res = result_struct(out)
    off = None
    rv = np.ascontiguousarray(ray_vec, dtype=np.float64)
    if use_packed:
        rv, off = packed(rv, npoints)
    npoints = np.ascontiguousarray(npoints, dtype=np.int32)
    n_conv = C.c_int32(0)
    conv = np.zeros(max(nray, 1), dtype=np.int32)
    rc = lib.rays_emul_ox_conv(C.byref(p), nray, 1 if use_packed else 0, rv.ctypes.data, npoints.ctypes.data,
                               off.ctypes.data if off is not None else None, C.byref(res), int(host_finish),
                               C.addressof(n_conv), conv.ctypes.data)
    assert rc == 0, f"rays_emul_ox_conv rc={rc}"
    out["converted"] = conv[:n_conv.value].copy()
    return out
