"""GPU tier: the ray-ordered profile sum per segment of rays (rays_amd/csrc/rays_deposition.hip:
profile_sum_segments_kernel) on its own, through rays_hip_profile_sum_segments_device, on synthetic work whose entries
span sixteen decades and both signs.  Expected values: the numpy restatement (tests/scan_profiles_lib.py: sequential
float64 adds per segment).  Every comparison is on bit patterns; no tolerance appears.

The ragged case: segments of 0, 1, 63, 64, 65, 0, 511, 512 and 513 rays from off[0] = 3, then a remainder that stops
short of the last ray.  Those lengths add up to 1729 -- more than the 1700 rays first planned for this case -- so the fan
here has 1800 rays and the remainder ends at ray 1772; no length was dropped."""
import functools

import numpy as np
import pytest

from rays_amd import hip
from tests import scan_profiles_lib as spl
from tests.test_gpu_deposition_binner import assert_same_bits

pytestmark = pytest.mark.gpu

NRAY = 1800
LENGTHS = [0, 1, 63, 64, 65, 0, 511, 512, 513, 40]
OFFSETS = np.concatenate([[3], 3 + np.cumsum(LENGTHS)]).astype(np.int32)   # ... 1732, 1772
UNIFORM = {1: 70, 64: 27, 65: 27, 513: 3}   # rays_per_seg -> n_seg, n_seg * rays_per_seg < NRAY
SENTINEL = 7.25
assert OFFSETS[-1] == 1772 < NRAY and all(k * n < NRAY for k, n in UNIFORM.items())


@functools.lru_cache(maxsize=None)
def work_of(n_bins):
    w = spl.synthetic_work(NRAY, n_bins)   # [nray][n_bins]
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def expected(n_bins, seg, with_carry):
    """(offsets, carry, profile) of the restatement; seg: "ragged" or a uniform rays_per_seg"""
    off = OFFSETS.astype(np.int64) if seg == "ragged" else spl.uniform_offsets(UNIFORM[seg], seg)
    carry = spl.synthetic_carry(len(off) - 1, n_bins) if with_carry else None
    want = spl.profile_sum_segments(work_of(n_bins), off, carry)
    want.setflags(write=False)
    return off, carry, want


def device_sum(n_bins, seg, carry, in_place=False):
    """-> (profile[n_seg][n_bins], the two sentinel rows behind it, work as the device holds it after the call)"""
    import torch
    d_work = torch.as_tensor(np.array(work_of(n_bins).T, order="C"), device="cuda")   # bin-major (a writable copy)
    if seg == "ragged":
        n_seg, segments = len(OFFSETS) - 1, torch.as_tensor(OFFSETS, device="cuda")
    else:
        n_seg, segments = UNIFORM[seg], (UNIFORM[seg], seg)
    buf = torch.full((n_seg + 2, n_bins), SENTINEL, dtype=torch.float64, device="cuda")
    out = buf[:n_seg]
    d_in = None if carry is None else torch.as_tensor(carry, device="cuda")
    if in_place:
        out.copy_(d_in)
        d_in = out
    got = hip.profile_sum_segments(d_work, segments, profile_in=d_in, profile_out=out,
                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy(), buf[n_seg:].cpu().numpy(), d_work.cpu().numpy()


@pytest.mark.parametrize("with_carry", [False, True], ids=["from_zero", "carry"])
@pytest.mark.parametrize("seg", ["ragged", 1, 64, 65, 513])
@pytest.mark.parametrize("n_bins", [1, 7, 320])
def test_segment_sums_equal_the_restatement(n_bins, seg, with_carry):
    """Segments that start off a multiple of 64, empty ones, one ray, a ragged and a full wave, a second chunk, a second
    pass of eight chunks with one ray / none / one ray more; rays before the first offset and behind the last belong to
    no profile.  Rows of profile_out beyond n_seg and every byte of work keep what they held."""
    off, carry, want = expected(n_bins, seg, with_carry)
    got, behind, work_after = device_sum(n_bins, seg, carry)
    assert_same_bits(got, want, f"n_bins {n_bins} segments {seg}")
    assert (behind == SENTINEL).all()
    assert work_after.tobytes() == np.ascontiguousarray(work_of(n_bins).T).tobytes()
    empty = np.flatnonzero(np.diff(off) == 0)
    for s in empty:   # an empty segment: its carry, or +0.0
        assert_same_bits(got[s], carry[s] if with_carry else np.zeros(n_bins))


@pytest.mark.parametrize("seg", ["ragged", 65])
@pytest.mark.parametrize("n_bins", [7, 320])
def test_in_place_carry(n_bins, seg):
    off, carry, want = expected(n_bins, seg, True)
    got, behind, _ = device_sum(n_bins, seg, carry, in_place=True)
    assert_same_bits(got, want)
    assert (behind == SENTINEL).all()


def test_the_sum_depends_on_the_ray_order():
    """The restatement summed from each segment's last ray to its first differs in some bin of some segment: a kernel
    that adds in another order cannot pass the comparisons above."""
    for seg in ("ragged", 64):
        off, carry, want = expected(7, seg, False)
        back = spl.profile_sum_segments(work_of(7), off, None, reverse=True)
        assert (back != want).any()


def test_one_segment_over_all_rays_equals_the_single_sum():
    """One segment [0, nray] on the work rays_hip_deposition_device wrote equals that entry's own profile (the single
    sum, profile_sum_kernel), from zero and from a carry that holds no -0.0."""
    import torch
    from tests import deposition_cases as dc
    from tests.test_gpu_deposition_binner import FAN_BINS, FAN_GRID, device_deposition, fan, fixture
    z = fixture()
    x, q, npts, pw, want_work = fan()
    nray = len(npts)
    lo, hi = z["grids"][FAN_GRID]
    p = dc.slab_params(lo, hi)
    carry = spl.synthetic_carry(1, FAN_BINS)
    for c in (None, carry):
        work, prof = device_deposition(p, FAN_BINS, x, q, npts, pw, carry=None if c is None else c[0])
        assert_same_bits(work, want_work)
        d_work = torch.as_tensor(np.ascontiguousarray(work.T), device="cuda")
        d_in = None if c is None else torch.as_tensor(c, device="cuda")
        for segments in (torch.as_tensor(np.array([0, nray], dtype=np.int32), device="cuda"), (1, nray)):
            got = hip.profile_sum_segments(d_work, segments, profile_in=d_in)
            torch.cuda.synchronize()
            assert_same_bits(got.cpu().numpy()[0], prof)


def test_offsets_are_clamped_and_refusals_are_named():
    """Offsets outside 0..nray are clamped and an end before its start is an empty segment: nothing outside work is read
    (the expected values are the restatement's, which clamps the same way).  The entry's refusals, by name; nothing is
    written by a refused call."""
    import torch
    n_bins = 7
    off = np.array([-5, 10, 4, NRAY + 7, 2_000_000_000, -2_000_000_000], dtype=np.int32)
    want = spl.profile_sum_segments(work_of(n_bins), off.astype(np.int64), None)
    d_work = torch.as_tensor(np.array(work_of(n_bins).T, order="C"), device="cuda")
    got = hip.profile_sum_segments(d_work, torch.as_tensor(off, device="cuda"))
    torch.cuda.synchronize()
    assert_same_bits(got.cpu().numpy(), want)
    assert not want[1].any() and not want[3].any() and not want[4].any() and want[0].any() and want[2].any()
    lib = hip.load()
    out = torch.full((4, n_bins), SENTINEL, dtype=torch.float64, device="cuda")
    W, O = d_work.data_ptr(), out.data_ptr()

    def refused(rc, text):
        assert rc != 0 and text in hip.last_error(), hip.last_error()
    who = "rays_hip_profile_sum_segments_device"
    refused(lib.rays_hip_profile_sum_segments_device(n_bins, NRAY, -1, None, 5, W, None, O, None), who + ": n_seg < 0")
    refused(lib.rays_hip_profile_sum_segments_device(n_bins, NRAY, 4, None, 0, W, None, O, None),
            who + ": neither segment offsets nor a positive rays_per_seg")
    refused(lib.rays_hip_profile_sum_segments_device(0, NRAY, 4, None, 5, W, None, O, None), who + ": n_bins < 1")
    refused(lib.rays_hip_profile_sum_segments_device(n_bins, -1, 4, None, 5, W, None, O, None), who + ": nray < 0")
    refused(lib.rays_hip_profile_sum_segments_device(n_bins, NRAY, 4, None, 5, None, None, O, None), who + ": null work or profile")
    refused(lib.rays_hip_profile_sum_segments_device(n_bins, NRAY, 4, None, 5, W, None, None, None), who + ": null work or profile")
    assert lib.rays_hip_profile_sum_segments_device(n_bins, NRAY, 0, None, 0, W, None, O, None) == 0   # no segment: nothing
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
