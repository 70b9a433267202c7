"""GPU tier of the deposition kernels (rays_amd/csrc/rays_deposition.hip: deposit_rays_kernel, profile_sum_kernel)
through rays_hip_deposition_device / rays_hip_deposition, on synthetic ray_vec arrays -- row 0 the grid value, row 7 the
power fraction, 'Ptotal_x' on the slab fixture's parameters with the grid and nstep_max set -- so no trace is needed.

Expected values: the rows the REFERENCE's binner_real made of the same rays (tests/golden/deposition_binner_cases.npz),
the plain restatement of tests/deposition_ref.py where the reference has no row (powers, the undefined-edge list), and
its sequential ray-ordered sum.  Everything is compared with assert_array_equal: there is no tolerance in this file.
The CPU tier (tests/test_cpu_deposition_binner.py) shows that the restatement equals the reference on every case and
that the fans' profiles depend on the order of the sum."""
import functools
import os

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.params import copy_params
from tests import deposition_cases as dc
from tests import deposition_ref as dr
from tests.common import ROOT, load_golden

pytestmark = pytest.mark.gpu

FAN_GRID, FAN_BINS = 2, 100   # the non-dyadic grid at the reference's default bin count
SENTINEL = 7.25               # what the output buffers hold before a call: every element must be written


@functools.lru_cache(maxsize=None)
def fixture():
    f = np.load(os.path.join(ROOT, "tests", "golden", "deposition_binner_cases.npz"), allow_pickle=False)
    return {k: f[k] for k in f.files}


def device_deposition(p, nb, x, q, npts, power, carry=None):
    """rays_hip_deposition_device on x[nray][NPT], Q[nray][NPT] -> (work[nray][n_bins], profile[n_bins])"""
    import torch
    nray = len(npts)
    assert nray >= 1
    rv = torch.as_tensor(dc.ray_vec_of(np.asarray(x), np.asarray(q), p.nv).reshape(nray, p.nstep_max + 1, p.nv), device="cuda")
    d_np = torch.as_tensor(np.ascontiguousarray(npts, dtype=np.int32), device="cuda")
    d_pw = torch.as_tensor(np.ascontiguousarray(power, dtype=np.float64), device="cuda")
    work = torch.full((nb, nray), SENTINEL, dtype=torch.float64, device="cuda")   # bin-major
    prof = torch.full((nb,), SENTINEL, dtype=torch.float64, device="cuda")
    d_in = None if carry is None else torch.as_tensor(np.ascontiguousarray(carry, dtype=np.float64), device="cuda")
    hip.deposition_device(p, "Ptotal_x", nb, nray, rv.data_ptr(), d_np.data_ptr(), d_pw.data_ptr(), work.data_ptr(),
                          None if d_in is None else d_in.data_ptr(), prof.data_ptr())
    torch.cuda.synchronize()
    return work.cpu().numpy().T, prof.cpu().numpy()


def assert_same_bits(a, b, msg=""):
    np.testing.assert_array_equal(a, b, err_msg=msg)
    np.testing.assert_array_equal(np.signbit(a), np.signbit(b), err_msg=msg + " (sign of zero)")


@pytest.mark.parametrize("ig", range(len(dc.GRIDS)))
def test_every_fixture_case_equals_the_reference_binner(ig):
    """38 rays x 6 bin counts (1 .. 320: the whole LDS of a CU) on one grid: work = the reference's rows, the profile
    their ray-ordered sum"""
    z = fixture()
    lo, hi = z["grids"][ig]
    p = dc.slab_params(lo, hi)
    for nb in z["n_bins"]:
        nb = int(nb)
        work, prof = device_deposition(p, nb, z["x_" + dc.key(ig, nb)], z["Q"], z["npoints"], np.ones(dc.NRAY))
        assert_same_bits(work, z["rows_" + dc.key(ig, nb)], f"grid {ig} n_bins {nb}")
        assert_same_bits(prof, dr.profile_sum(z["rows_" + dc.key(ig, nb)]), f"grid {ig} n_bins {nb}: profile")


def test_undefined_edge_cases_equal_the_guarded_restatement():
    """x_high just below xmax whose index rounds up to n_bins: bins 1..n_bins as the reference's statements give them,
    the update of bin n_bins + 1 not made; one launch per (grid, n_bins)"""
    z = fixture()
    combos = sorted(set(zip(z["edge_grid"].tolist(), z["edge_n_bins"].tolist())))
    assert len(combos) >= 4
    for ig, nb in combos:
        sel = np.flatnonzero((z["edge_grid"] == ig) & (z["edge_n_bins"] == nb))
        lo, hi = z["grids"][ig]
        x, q, npts = z["edge_x"][sel], z["edge_Q"][sel], z["edge_npoints"][sel]
        assert all(dc.has_undefined_segment(x[i, :n], lo, hi, nb) for i, n in enumerate(npts))
        work, prof = device_deposition(dc.slab_params(lo, hi), nb, x, q, npts, np.ones(len(sel)))
        want = np.stack([dr.bin_ray(x[i, :n], q[i, :n], lo, hi, nb)[0] for i, n in enumerate(npts)])
        assert_same_bits(work, want, f"grid {ig} n_bins {nb}")
        assert_same_bits(prof, dr.profile_sum(want))


@functools.lru_cache(maxsize=None)
def fan(nray_max=1100):
    """the fixture's rays tiled (ray i = case i mod 38) with powers +-2**k over sixteen decades, and the expected work"""
    z = fixture()
    x, q, npts, pw = dc.tiled_fan(z, FAN_GRID, FAN_BINS, nray_max)
    lo, hi = z["grids"][FAN_GRID]
    work = np.stack([dr.bin_ray(x[i, :n], q[i, :n] * pw[i], lo, hi, FAN_BINS)[0] for i, n in enumerate(npts)])
    for a in (x, q, npts, pw, work):
        a.setflags(write=False)
    return x, q, npts, pw, work


@pytest.mark.parametrize("nray", [1, 63, 64, 65, 513, 1100])
def test_fan_sizes_work_rows_and_ray_ordered_profile(nray):
    """one lane, a ragged and a full wave, a second block; 513 = a second pass of profile_sum_kernel with a one-ray chunk,
    1100 = three passes, the last one ragged inside its second chunk.  The profile must be the SEQUENTIAL sum."""
    z = fixture()
    x, q, npts, pw, want = (a[:nray] for a in fan())
    lo, hi = z["grids"][FAN_GRID]
    work, prof = device_deposition(dc.slab_params(lo, hi), FAN_BINS, x, q, npts, pw)
    assert_same_bits(work, want)
    rows = z["rows_" + dc.key(FAN_GRID, FAN_BINS)]
    for i in range(nray):   # ... which are the reference's rows times the power (family f apart: subnormal steps)
        if dc.FAMILIES[i % dc.NRAY] != "f":
            assert_same_bits(work[i], rows[i % dc.NRAY] * pw[i] + 0.0)
    assert_same_bits(prof, dr.profile_sum(want))


def test_full_chunks_only():
    """1024 rays = two passes of eight full 64-ray chunks"""
    z = fixture()
    x, q, npts, pw, want = (a[:1024] for a in fan())
    lo, hi = z["grids"][FAN_GRID]
    work, prof = device_deposition(dc.slab_params(lo, hi), FAN_BINS, x, q, npts, pw)
    assert_same_bits(work, want)
    assert_same_bits(prof, dr.profile_sum(want))


@pytest.mark.parametrize("cut", [1, 512, 513, 1099])
def test_chained_blocks_give_the_unsplit_profile(cut):
    z = fixture()
    x, q, npts, pw, want = fan()
    lo, hi = z["grids"][FAN_GRID]
    p = dc.slab_params(lo, hi)
    w1, part = device_deposition(p, FAN_BINS, x[:cut], q[:cut], npts[:cut], pw[:cut])
    w2, prof = device_deposition(p, FAN_BINS, x[cut:], q[cut:], npts[cut:], pw[cut:], carry=part)
    assert_same_bits(np.concatenate([w1, w2]), want)
    assert_same_bits(part, dr.profile_sum(want[:cut]))
    assert_same_bits(prof, dr.profile_sum(want))


@pytest.mark.parametrize("case", ["fewer points than nstep_max + 1", "nstep_max + 1 points", "no points at all"])
def test_host_form_equals_device_form(case):
    z = fixture()
    x, q, npts, pw, want = (a[:130] for a in fan())
    lo, hi = z["grids"][FAN_GRID]
    p = dc.slab_params(lo, hi)
    assert npts.max() == dc.NPT == p.nstep_max + 1
    if case == "no points at all":
        npts = np.zeros_like(npts)
        want = np.zeros_like(want)
    w_dev, prof_dev = device_deposition(p, FAN_BINS, x, q, npts, pw)
    ph = copy_params(p)
    if case == "fewer points than nstep_max + 1":
        ph.nstep_max = dc.NPT + 3      # the host arrays carry four more (zero) points per ray than any ray has
    rv = np.zeros((130, ph.nstep_max + 1, p.nv))
    rv[:, :dc.NPT] = dc.ray_vec_of(x, q, p.nv)
    w_host, prof_host = hip.deposition_host(ph, "Ptotal_x", FAN_BINS, rv, npts, pw)
    assert_same_bits(w_host, w_dev)
    assert_same_bits(prof_host, prof_dev)
    assert_same_bits(w_dev, want)
    assert_same_bits(prof_dev, dr.profile_sum(want))


def test_no_rays_give_a_zero_profile():
    z = fixture()
    lo, hi = z["grids"][FAN_GRID]
    p = dc.slab_params(lo, hi)
    work, prof = hip.deposition_host(p, "Ptotal_x", FAN_BINS, np.zeros((0, dc.NPT, p.nv)), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert work.shape == (0, FAN_BINS)
    assert_same_bits(prof, np.zeros(FAN_BINS))


def test_bin_limit():
    """320 bins work (every fixture case above runs them); 321 are refused by name before any launch"""
    import torch
    z = fixture()
    lo, hi = z["grids"][FAN_GRID]
    p = dc.slab_params(lo, hi)
    x, q, npts = z["x_" + dc.key(FAN_GRID, 320)], z["Q"], z["npoints"]
    work, prof = device_deposition(p, 320, x, q, npts, np.ones(dc.NRAY))
    assert_same_bits(work, z["rows_" + dc.key(FAN_GRID, 320)])
    with pytest.raises(hip.RaysHipError, match="limit of 320 bins"):
        device_deposition(p, 321, x, q, npts, np.ones(dc.NRAY))
    torch.cuda.synchronize()
    with pytest.raises(hip.RaysHipError, match="limit of 320 bins"):
        hip.deposition_host(p, "Ptotal_x", 321, dc.ray_vec_of(x, q, p.nv), npts, np.ones(dc.NRAY))
    # ... and the device is as usable as before
    work, _ = device_deposition(p, 320, x, q, npts, np.ones(dc.NRAY))
    assert_same_bits(work, z["rows_" + dc.key(FAN_GRID, 320)])


def test_axisym_profiles_with_more_than_one_block():
    """'Ptotal_psi' and 'Ptotal_rho' (the psi evaluator and the rho spline per point) on the device trace of the eqdsk
    fixture tiled to 613 rays: ten blocks, a second pass of the sum with a ragged chunk.  work rows = the reference
    post-processor's, the profile = their sequential sum."""
    import torch
    from rays_amd.trace import DeviceTrace
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    tr = DeviceTrace(p, g["rvec0_full"], g["rindex_vec0_full"])
    tr.launch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tr.npoints.cpu().numpy(), g["npoints_full"])
    nray, nb = 613, int(g["dep_n_bins"])
    idx = np.arange(nray) % tr.nray
    t_idx = torch.as_tensor(idx, device="cuda")
    rv, npts = tr.ray_vec[t_idx].contiguous(), tr.npoints[t_idx].contiguous()
    power = torch.as_tensor(g["dep_power"][idx], device="cuda")
    hip.set_rho_table(g["dep_rho_grid"], g["dep_rho_fspl"])
    for which, name in enumerate(("Ptotal_psi", "Ptotal_rho")):
        work = torch.full((nb, nray), SENTINEL, dtype=torch.float64, device="cuda")
        prof = torch.full((nb,), SENTINEL, dtype=torch.float64, device="cuda")
        hip.deposition_device(p, name, nb, nray, rv.data_ptr(), npts.data_ptr(), power.data_ptr(), work.data_ptr(), None,
                              prof.data_ptr())
        torch.cuda.synchronize()
        want = g["dep_work"][which][idx]
        assert_same_bits(work.cpu().numpy().T, want, name)
        assert_same_bits(prof.cpu().numpy(), dr.profile_sum(want), name)
