"""Synthetic rays for the uniform grid binner under the deposition profiles (rays_amd/csrc/rays_deposition.hpp:
deposit_ray = the reference's bin_a_ray + binner_real, math_functions_lib/bin_to_uniform_grid_m.f90).

Deterministic: the pseudo-random numbers come from the integer generator below, not from a library, so
tests/golden/make_golden.py reproduces tests/golden/deposition_binner_cases.npz bit for bit anywhere.  The tests read
the fixture (inputs and the reference's rows); this module is what made the inputs.

A ray is a list of grid values x(1:np) and cumulative absorbed power Q(1:np), np <= NPT.  Every ray is generated for
every (grid, n_bins) of GRIDS x N_BINS: its x depend on the grid (bin edges, clipping), its Q do not.  Families:

  a  random walks inside the grid, steps of 0 to 6 bin widths in both directions (middle-bin fill, descending x)
  b  points exactly on the bin edges xmin + k*x_bin_width and one ulp to either side of them
  c  segments entering across xmin, leaving across xmax, and crossing both at once
  d  segments wholly outside the grid, and the ones that touch it: x_high == xmin, x_low == xmax, x_low == x_high == xmax
  e  repeated points (delta_ix == 0) with and without a power change
  f  power steps below 4*tiny (subnormal, zero) next to ordinary ones
  g  power that decreases, power that is negative
  h  rays of 0, 1 and 2 points

Families a, b and e stay inside [xmin, xmax] and every segment of theirs is either a repeated point or at least
2**-8 bin widths long (the high-precision check of tests/test_cpu_deposition_binner.py needs |delta_ix| >= 2**-10).

UNDEFINED IN THE REFERENCE, kept out of the reference-cut set: a segment with x_high < xmax whose quotient
(x_high - xmin)/x_bin_width rounds up to n_bins makes binner_real update binned_Q(n_bins + 1), one element past the
array.  `cases()` moves every point off such a value and asserts that none is left;
`edge_cases()` is the second list, made of exactly those segments, whose expected rows come from
tests/deposition_ref.py with the guard.
"""
from __future__ import annotations

import math

import numpy as np

GRIDS = ((-0.5, 0.5), (0.0, 1.0), (0.1, 0.7), (1000.0, 1000.3))   # dyadic | dyadic | non-dyadic width | x - xmin cancels
N_BINS = (1, 2, 3, 7, 100, 320)
NPT = 12
TINY = 2.2250738585072014e-308   # tiny(1.0d0)
FAMILIES = "aaaaaa" "bbbbbb" "cccccc" "ddddd" "eeee" "ffff" "gggg" "hhh"
NRAY = len(FAMILIES)


class Lcg:
    """Knuth's 64-bit linear congruential generator; the top 53 bits make a double in [0, 1)."""

    def __init__(self, seed):
        self.s = (int(seed) * 0x9E3779B97F4A7C15 + 0x1234567) & 0xFFFFFFFFFFFFFFFF
        for _ in range(4):
            self.u()

    def u(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 11) / 9007199254740992.0

    def uniform(self, a, b):
        return a + (b - a) * self.u()

    def below(self, n):
        return min(int(self.u() * n), n - 1)


def up(x, n=1):
    for _ in range(n):
        x = float(np.nextafter(x, np.inf))
    return x


def down(x, n=1):
    for _ in range(n):
        x = float(np.nextafter(x, -np.inf))
    return x


def past_last_bin(x, xmin, xmax, n_bins):
    """x below xmax whose real-number index reaches n_bins: as a segment's upper end, undefined in the reference"""
    w = (xmax - xmin) / n_bins
    return x < xmax and math.floor((x - xmin) / w) >= n_bins


def has_undefined_segment(x, xmin, xmax, n_bins):
    return any(past_last_bin(max(x[i - 1], x[i]), xmin, xmax, n_bins) for i in range(1, len(x)))


def _fold(t, n_bins):
    """reflect a position in bin units back into [0, n_bins - 2**-8]"""
    L = float(n_bins)
    t = math.fmod(abs(t), 2 * L)
    if t > L:
        t = 2 * L - t
    return min(t, L - 2.0 ** -8)


def _x_of_ray(iray, xmin, xmax, n_bins):
    fam = FAMILIES[iray]
    k_in_family = iray - FAMILIES.index(fam)
    r = Lcg(1000 + iray)
    w = (xmax - xmin) / n_bins
    n = float(n_bins)
    at = lambda t: xmin + t * w          # noqa: E731  (t in bin widths from xmin)
    if fam == "a":
        t = r.uniform(0.0, n - 2.0 ** -8)
        ts = [t]
        for _ in range(NPT - 1):
            step = r.uniform(0.0, 6.0) * (1.0 if r.u() < 0.5 else -1.0)
            if k_in_family == 1:
                step = abs(step) * 0.5            # one ray climbs only,
            if k_in_family == 2:
                step = -abs(step) * 0.5           # one descends only (both fold back at the ends)
            t2 = _fold(t + step, n_bins)
            if abs(t2 - t) < 2.0 ** -8:
                t2 = t
            ts.append(t2)
            t = t2
        return [min(at(t), xmax) for t in ts]
    if fam == "b":
        xs, k_prev = [], -1
        for i in range(NPT):
            k = r.below(n_bins + 1)
            if k == k_prev:
                k = (k + 1) % (n_bins + 1)
            k_prev = k
            off = (i + k_in_family) % 3 - 1       # -1, 0, +1 ulp in turn
            e = xmax if k == n_bins else at(float(k))
            if k == 0:
                off = max(off, 0)                  # stay inside the grid
            if k == n_bins:
                off = min(off, 0)
            xs.append(up(e) if off > 0 else down(e) if off < 0 else e)
        return [min(max(x, xmin), xmax) for x in xs]
    if fam == "c":
        f = lambda a, b=0.0: at(a * n + b)   # noqa: E731  (fraction of the grid + bins)
        return [
            [f(0, -1.3), f(0.3), f(0.8), f(0, -0.4), f(0.55), f(0, -2.5), f(0.1), f(0.1)],               # in and out across xmin
            [f(0.6), f(1, 0.4), f(0.2), f(1, 2.5), f(0.9), f(1, 0.01), f(0.95)],                         # ... across xmax
            [f(0, -0.7), f(1, 0.3), f(0, -3.2), f(1, 1.5), f(0.5), f(1, 0.6), f(0, -0.1), f(1, 0.05)],   # both in one segment
            [down(xmin), f(0.4), up(xmax), f(0.7), down(xmin), up(xmax)],                                # one ulp outside
            [f(0, -1.1), xmax, f(0.5), xmin, f(1, 0.8), xmin, f(0, -0.5), xmax],                         # ends exactly on the limits
            [r.uniform(-0.3 * n - 1.0, 1.3 * n + 1.0) * w + xmin for _ in range(NPT)],
        ][k_in_family]
    if fam == "d":
        f = lambda a, b=0.0: at(a * n + b)   # noqa: E731
        return [
            [f(0, -3.0), f(0, -0.2), f(0, -1.5), down(xmin), f(0, -0.01)],            # wholly below
            [f(1, 0.2), f(1, 4.0), up(xmax), f(1, 0.7), f(1, 0.7)],                   # wholly above
            [f(0, -1.0), xmin, f(0, -0.5), xmin, xmin, f(0.5)],                       # x_high == xmin (then a point inside)
            [f(1, 1.0), xmax, f(1, 0.5), xmax, xmax, xmax, f(0.5)],                   # x_low == xmax, x_low == x_high == xmax
            [f(0.5), xmax, xmax, f(0.25), xmin, xmin, f(0.75)],                       # the same, reached from inside
        ][k_in_family]
    if fam == "e":
        t = []
        for _ in range(5):   # strictly inside a bin: a repeated point ON an edge belongs to either neighbour
            v = r.uniform(0.0, n)
            k = min(math.floor(v), n_bins - 1)
            t.append(k + min(max(v - k, 0.05), 0.95))
        return [
            [at(t[0])] * 3 + [at(t[1])] * 2 + [at(t[2])] * 4 + [at(t[3])],
            [at(t[4])] * NPT,
            [xmin, xmin, at(t[0]), at(t[0]), xmin, xmin, at(t[2])],
            [at(t[1]), at(t[3]), at(t[3]), at(t[1]), at(t[1]), at(t[3])],
        ][k_in_family]
    if fam in "fg":
        t = r.uniform(0.0, n - 2.0 ** -8)
        ts = [t]
        for _ in range(NPT - 1):
            t = _fold(t + r.uniform(-2.5, 2.5), n_bins)
            ts.append(t)
        return [min(at(t), xmax) for t in ts]
    if fam == "h":
        return [at(0.3 * n), at(0.8 * n)][:k_in_family]
    raise AssertionError(fam)


def _q_of_ray(iray, npts):
    fam = FAMILIES[iray]
    k_in_family = iray - FAMILIES.index(fam)
    r = Lcg(5000 + iray)
    if fam == "f":
        sub = 4.9406564584124654e-324
        q = [
            [0.0, sub, 1e-310, 1e-310, 3e-308, 3e-308 + 4 * TINY, 0.25, 0.25, 0.25 + 1e-300, 0.5, 0.5, 0.75],
            [0.0, 4 * TINY, 4 * TINY + down(4 * TINY), 2e-307, 2e-307, 2e-307 - sub, 0.0, -0.0, 0.0, 1e-3, 1e-3, 1e-3],
            [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5],                    # no power at all
            [1e-300, 1e-300 + 7e-308, 1e-300 + 7e-308 + 9e-308, 0.1, 0.1 + 2.0 ** -55, 0.2, 0.2, -0.0, 0.0, sub, -sub, 0.3],
        ][k_in_family]
        return q[:npts]
    if fam == "g":
        if k_in_family == 0:      # decreasing from 1
            q, v = [], 1.0
            for _ in range(npts):
                q.append(v)
                v = v - r.uniform(0.0, 0.12)
        elif k_in_family == 1:    # negative throughout, down to -1.35
            q = [-1.35 * (i + 1) / npts for i in range(npts)]
        elif k_in_family == 2:    # up and down through zero
            q = [r.uniform(-1.0, 1.0) for _ in range(npts)]
        else:                     # negative and rising
            q = [-0.9 + 0.07 * i * r.uniform(0.5, 1.0) for i in range(npts)]
        return q
    if fam == "e":
        # a repeated point with a power change, then one without, in turn
        q, v = [], 0.0
        for i in range(npts):
            q.append(v)
            if (i + k_in_family) % 2 == 0:
                v = v + r.uniform(0.01, 0.1)
        return q
    # absorbed power fraction: 0 at the launch point, rising
    q, v = [], 0.0
    for _ in range(npts):
        q.append(v)
        v = v + r.uniform(0.0, 0.09)
    return q


def _off_undefined(x, xmin, xmax, n_bins):
    while past_last_bin(x, xmin, xmax, n_bins):
        x = down(x)
    return x


def cases(xmin, xmax, n_bins):
    """The reference-cut set for one (grid, n_bins): (x[NRAY][NPT], Q[NRAY][NPT], npoints[NRAY]); slots past npoints are 0."""
    x, q, npts = np.zeros((NRAY, NPT)), np.zeros((NRAY, NPT)), np.zeros(NRAY, dtype=np.int32)
    for i in range(NRAY):
        xs = [_off_undefined(float(v), xmin, xmax, n_bins) for v in _x_of_ray(i, xmin, xmax, n_bins)]
        assert len(xs) <= NPT and all(math.isfinite(v) for v in xs)
        assert not has_undefined_segment(xs, xmin, xmax, n_bins), (i, xmin, xmax, n_bins)
        if FAMILIES[i] in "abe":
            assert all(xmin <= v <= xmax for v in xs), (i, xmin, xmax, n_bins)
        qs = _q_of_ray(i, len(xs))
        assert len(qs) == len(xs)
        npts[i] = len(xs)
        x[i, :len(xs)], q[i, :len(xs)] = xs, qs
    return x, q, npts


def edge_cases():
    """The second list: rays whose segments end on an x_high < xmax with floor((x_high - xmin)/x_bin_width) >= n_bins
    (one and two ulps below xmax, wherever that happens among GRIDS x N_BINS).  Flat:
    (grid index[n], n_bins[n], x[n][NPT], Q[n][NPT], npoints[n])."""
    gi, nb, xs, qs, npts = [], [], [], [], []
    for ig, (xmin, xmax) in enumerate(GRIDS):
        for n_bins in N_BINS:
            w = (xmax - xmin) / n_bins
            n = float(n_bins)
            at = lambda t: xmin + t * w   # noqa: E731
            for ulps in (1, 2):
                xh = down(xmax, ulps)
                if not past_last_bin(xh, xmin, xmax, n_bins):
                    continue
                rays = [
                    [at(n - 0.5), xh],                                                     # the plain case: two neighbouring "bins"
                    [at(n - 0.5), xh, at(max(n - 3.5, 0.25)), xh, xh, at(n + 1.2), xh, at(-0.6), xh, xmax, xh],
                ]
                for ray in rays:
                    assert has_undefined_segment(ray, xmin, xmax, n_bins)
                    row_x, row_q = np.zeros(NPT), np.zeros(NPT)
                    row_x[:len(ray)] = ray
                    row_q[:len(ray)] = [0.125 * i + 0.01 * i * i for i in range(len(ray))]
                    gi.append(ig), nb.append(n_bins), xs.append(row_x), qs.append(row_q), npts.append(len(ray))
    assert len(gi) >= 8
    return (np.array(gi, dtype=np.int32), np.array(nb, dtype=np.int32), np.array(xs), np.array(qs),
            np.array(npts, dtype=np.int32))


def write_case_file(path, case_list):
    """The stream file oracle/ref_binner_driver.f90 and tests/hip_emul/emul_deposition_main.cpp read:
    int32 ncase, then per case float64 xmin, xmax; int32 n_bins, nx; float64 xQ[nx], Q[nx]."""
    with open(path, "wb") as f:
        f.write(np.int32(len(case_list)).tobytes())
        for xmin, xmax, n_bins, x, q in case_list:
            assert len(x) == len(q)
            f.write(np.array([xmin, xmax], dtype="<f8").tobytes())
            f.write(np.array([n_bins, len(x)], dtype="<i4").tobytes())
            f.write(np.asarray(x, dtype="<f8").tobytes())
            f.write(np.asarray(q, dtype="<f8").tobytes())


def read_result_file(path, case_list):
    """per case int32 ierr; float64 binned_Q[n_bins] -> ([rows], [ierr])"""
    rows, ierr = [], []
    with open(path, "rb") as f:
        for _, _, n_bins, _, _ in case_list:
            ierr.append(int(np.frombuffer(f.read(4), dtype="<i4")[0]))
            rows.append(np.frombuffer(f.read(8 * n_bins), dtype="<f8").copy())
        assert f.read() == b""
    return rows, ierr


def key(ig, n_bins):
    return f"g{ig}_n{n_bins}"


def case_list_of_fixture(z):
    """every (grid, n_bins, ray) of the fixture as one flat list of (xmin, xmax, n_bins, x, Q), in GRIDS x N_BINS x ray order"""
    out = []
    for ig, (xmin, xmax) in enumerate(z["grids"]):
        for n_bins in z["n_bins"]:
            x = z["x_" + key(ig, int(n_bins))]
            for i, npt in enumerate(z["npoints"]):
                out.append((float(xmin), float(xmax), int(n_bins), x[i, :npt], z["Q"][i, :npt]))
    return out


def edge_list_of_fixture(z):
    return [(float(z["grids"][g][0]), float(z["grids"][g][1]), int(n), z["edge_x"][i, :m], z["edge_Q"][i, :m])
            for i, (g, n, m) in enumerate(zip(z["edge_grid"], z["edge_n_bins"], z["edge_npoints"]))]


# ---- fans for the kernels: the fixture's rays tiled to any number of rays ----------------------------------------

def fan_powers(nray):
    """initial_ray_power of a tiled fan: +-2**k, k over -27..26 (sixteen decades), signs mixed.  Powers of two, so a
    ray's row is the fixture's row times its power exactly (no subnormal involved: every family but f)."""
    k = (np.arange(nray) * 37 + 11) % 54 - 27
    sign = np.where((np.arange(nray) * 7 + 3) % 5 < 2, -1.0, 1.0)
    return sign * np.ldexp(1.0, k)


def ray_vec_of(x, Q, nv):
    """ray_vec[nray][npt][nv] with the grid value in row 0 (Ptotal_x reads x) and the power fraction in row 7"""
    rv = np.zeros(x.shape + (nv,))
    rv[..., 0], rv[..., 7] = x, Q
    return rv


def tiled_fan(z, ig, n_bins, nray):
    """(x[nray][NPT], Q[nray][NPT], npoints[nray], power[nray]): ray i = the fixture's ray i mod its ray count"""
    idx = np.arange(nray) % len(z["npoints"])
    return z["x_" + key(ig, n_bins)][idx], z["Q"][idx], z["npoints"][idx], fan_powers(nray)


def slab_params(lo, hi):
    """The parameters of the slab fixture with damping ('Ptotal_x' bins ray_vec(1) on [slab.xmin, slab.xmax]), the grid
    set to [lo, hi] and room for NPT points per ray"""
    from rays_amd.params import copy_params
    from tests.common import load_golden
    g, nml, p = load_golden("gold_slab16_damp_rk4")
    q = copy_params(p)
    q.slab.xmin, q.slab.xmax, q.nstep_max = float(lo), float(hi), NPT - 1
    return q
