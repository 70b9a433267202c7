"""TEST INFRASTRUCTURE ONLY: what the segmented-deposition tests share (rays_hip_profile_sum_segments_device,
rays_hip_scan_profiles_device, rays_hip_trace_profiles_segments_device) -- the numpy restatement of the sum per segment
and the synthetic work it is tested on."""
from __future__ import annotations

import numpy as np

from tests import deposition_ref as dr


def profile_sum_segments(work, offsets, carry=None, reverse=False):
    """profile[s][b] = carry[s][b] + work[off[s]][b] + work[off[s] + 1][b] + ... + work[off[s + 1] - 1][b]: sequential
    float64 adds in ray order (dr.profile_sum per slice), nothing else added -- an empty segment gives its carry, or
    +0.0.  work[nray][n_bins] (the reference's layout); offsets: n_seg + 1 ray indices, each clamped to 0..nray, an end
    before its start counting as empty; carry[n_seg][n_bins] or None.  reverse=True: each segment summed from its last
    ray to its first (what the product must NOT compute)."""
    work = np.asarray(work, dtype=np.float64)
    nray, n_bins = work.shape
    off = np.clip(np.asarray(offsets, dtype=np.int64), 0, nray)
    out = np.zeros((len(off) - 1, n_bins))
    for s in range(len(off) - 1):
        r0, r1 = int(off[s]), max(int(off[s + 1]), int(off[s]))
        rows = work[r0:r1]
        out[s] = dr.profile_sum(rows[::-1] if reverse else rows, None if carry is None else carry[s])
    return out


def uniform_offsets(n_seg: int, rays_per_seg: int):
    return np.arange(n_seg + 1, dtype=np.int64) * rays_per_seg


def synthetic_work(nray: int, n_bins: int):
    """work[nray][n_bins]: entries +-m * 2**k, m in [1, 2) with a full mantissa, k over -27..26 (sixteen decades), signs
    mixed -- a sum of them depends on the order of its adds in nearly every bin."""
    r = np.arange(nray, dtype=np.int64)[:, None]
    b = np.arange(n_bins, dtype=np.int64)[None, :]
    k = (r * 37 + b * 13 + 11) % 54 - 27
    sign = np.where((r * 7 + b * 3 + 3) % 5 < 2, -1.0, 1.0)
    mant = 1.0 + ((r * 2654435761 + b * 40503 + 12345) % 1000003) / 1000003.0
    return np.ascontiguousarray(sign * np.ldexp(mant, k.astype(np.int32)))


def synthetic_carry(n_seg: int, n_bins: int):
    s = np.arange(n_seg, dtype=np.int64)[:, None]
    b = np.arange(n_bins, dtype=np.int64)[None, :]
    return np.ascontiguousarray(np.where((s + b) % 3 == 0, -1.0, 1.0) * (0.375 + ((s * 31 + b * 17) % 97) / 7.0))
