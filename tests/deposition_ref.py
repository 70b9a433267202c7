"""Plain restatement of the reference's uniform grid binner and profile sum, for the deposition tests.

Written from the statements of binner_real (math_functions_lib/bin_to_uniform_grid_m.f90) and of
calculate_deposition_profiles (post_process_lib/deposition_profiles_m.f90: profile = sum(work, 2)), NOT from
rays_amd/csrc/rays_deposition.hpp: the tests compare two independent readings of the reference.  Scalar Python floats
(IEEE binary64, one rounding per operation), in the reference's order of operations.
"""
from __future__ import annotations

import math

import numpy as np

TINY = 2.2250738585072014e-308   # tiny(delta_Q), real(rkind)


def bin_ray(x, Q, xmin, xmax, n_bins, guard=True):
    """binner_real(Q, xQ, xmin, xmax, binned_Q, ierr) -> (binned_Q[n_bins], ierr).

    guard: the update of binned_Q(index_high) is not executed when index_high = n_bins + 1 (x_high < xmax whose
    real-number index rounds up to n_bins): the reference writes one element past binned_Q there, which is undefined.
    With guard=False that case raises IndexError instead."""
    x = [float(v) for v in x]
    Q = [float(v) for v in Q]
    assert len(x) == len(Q)
    xmin, xmax = float(xmin), float(xmax)
    binned_Q = [0.0] * n_bins           # indices 1..n_bins below are binned_Q[index - 1]
    ierr = 0
    x_range = xmax - xmin
    x_bin_width = x_range / float(n_bins)

    def add(index, value):
        if not 1 <= index <= n_bins:
            raise IndexError(f"binned_Q({index}) of {n_bins}")
        binned_Q[index - 1] = binned_Q[index - 1] + value

    for i_s in range(1, len(x)):
        x_low = min(x[i_s - 1], x[i_s])
        x_high = max(x[i_s - 1], x[i_s])
        ix_low = (x_low - xmin) / x_bin_width
        ix_high = (x_high - xmin) / x_bin_width
        delta_ix = ix_high - ix_low
        index_low = math.floor(ix_low) + 1
        index_high = math.floor(ix_high) + 1
        if x_high >= xmax:
            index_high = n_bins
        delta_i = index_high - index_low
        delta_Q = Q[i_s] - Q[i_s - 1]
        # Q_density = delta_Q/delta_ix is formed here in the reference (Inf or NaN for a repeated point, never used then)
        if abs(delta_Q) < 4.0 * TINY:
            continue
        if x_high < xmin or x_low > xmax:
            continue
        if x_low < xmin:
            fraction_in = ix_high / delta_ix
            delta_Q = delta_Q * fraction_in
            ix_low = 0.0
            index_low = 1
            delta_i = index_high - index_low
            ierr = 1
        if x_high > xmax:
            fraction_in = (float(n_bins) - ix_low) / delta_ix
            delta_Q = delta_Q * fraction_in
            ix_high = float(n_bins)
            index_high = n_bins
            delta_i = index_high - index_low
            ierr = 2
        if delta_i == 0:
            if guard and index_low == n_bins + 1:
                continue                 # (the same element past the end, reached with both ends in "bin n_bins + 1")
            add(index_low, delta_Q)
        elif delta_i > 0:
            fraction_low = (float(index_low) - ix_low) / delta_ix
            Q_incrL = delta_Q * fraction_low
            add(index_low, Q_incrL)
            fraction_high = (ix_high - float(index_high - 1)) / delta_ix
            Q_incrH = delta_Q * fraction_high
            if not (guard and index_high == n_bins + 1):
                add(index_high, Q_incrH)
            if delta_i > 1:
                Q_density = (Q[i_s] - Q[i_s - 1]) / delta_ix     # from the unclipped delta_Q and delta_ix
                for i in range(index_low + 1, index_high):
                    add(i, Q_density)
    return np.array(binned_Q, dtype=np.float64), ierr


def profile_sum(work, carry=None):
    """profile(b) = carry(b) + work(1, b) + work(2, b) + ... one ray after the other (the reference's sum(work, 2)
    as its compiler evaluates it: a sequential loop; np.sum adds pairwise and is NOT this).  work[nray][n_bins]."""
    work = np.asarray(work, dtype=np.float64)
    prof = [0.0] * work.shape[1] if carry is None else [float(c) for c in carry]
    for row in work:
        for b, v in enumerate(row):
            prof[b] = prof[b] + float(v)
    return np.array(prof, dtype=np.float64)


def exact_bins(x, Q, xmin, xmax, n_bins):
    """What the binner approximates, in exact rational arithmetic from the same float inputs, for rays inside
    [xmin, xmax]: each segment's delta_Q times the exact fraction of the segment lying in each bin; a repeated point gives
    all of its delta_Q to the bin that holds it (bins are [edge_k, edge_k+1), the last one closed at xmax).
    Returns (exact[n_bins] as Fractions, sum |delta_Q| over the segments touching each bin)."""
    from fractions import Fraction as F
    xmin, xmax = F(float(xmin)), F(float(xmax))
    W = (xmax - xmin) / n_bins
    edge = [xmin + k * W for k in range(n_bins + 1)]
    exact = [F(0)] * n_bins
    touched = [F(0)] * n_bins
    for i in range(1, len(x)):
        a, b = sorted((F(float(x[i - 1])), F(float(x[i]))))
        assert xmin <= a and b <= xmax
        dQ = F(float(Q[i])) - F(float(Q[i - 1]))
        k_first = max(0, math.floor((a - xmin) / W) - 1)
        k_last = min(n_bins - 1, math.floor((b - xmin) / W) + 1)
        for k in range(k_first, k_last + 1):
            lo, hi = edge[k], edge[k + 1]
            if a == b:
                inside = (lo <= a < hi) or (k == n_bins - 1 and a == hi)
                frac = F(1) if inside else F(0)
                touch = inside
            else:
                ov = min(b, hi) - max(a, lo)
                frac = ov / (b - a) if ov > 0 else F(0)
                touch = min(b, hi) >= max(a, lo)     # closed intervals meet
            exact[k] += dQ * frac
            if touch:
                touched[k] += abs(dQ)
    return exact, touched
