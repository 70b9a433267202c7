"""GPU tier of the packed ray diagnostics (include/rays_hip.h: rays_hip_point_offsets_device,
rays_hip_ray_diagnostics_packed_device): the recorded points alone, one wave per 64 consecutive packed points.  The
arithmetic is the padded entry's diag_point, so every comparison is on the bit patterns (tests/diag_expect.py:
assert_bits) against the padded entry's output at the recorded points."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from rays_amd import hip
from rays_amd.trace import DeviceTrace, RayResults, RaysRun
from tests import diag_expect as dx
from tests.common import GOLDEN_CASES, ROOT, load_golden

pytestmark = pytest.mark.gpu

PREFILL = 0x7FF8DEADBEEF0123   # a NaN no kernel produces: an untouched slot is recognised by its bits
EDGE_NPOINTS = [0, 1, 63, 64, 65, 127, 128, 129, 0, 0, 145, 2, 64]


def _prefilled(torch, n):
    return torch.full((int(n),), PREFILL, dtype=torch.int64, device="cuda").view(torch.float64)


def _untouched(a):
    return np.ascontiguousarray(a).view(np.uint64) == np.uint64(PREFILL)


def _traced(name):
    g, nml, p = load_golden(name)
    tr = DeviceTrace(p, g["rvec0"], g["rindex_vec0"])
    tr.launch()
    return g, p, tr


def _offsets(tr, npoints=None):
    import torch

    npoints = tr.npoints if npoints is None else npoints
    off = torch.empty(tr.nray + 1, dtype=torch.int64, device="cuda")
    hip.point_offsets_device(tr.nray, tr.params.nstep_max, npoints.data_ptr(), off.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    return off


def _pack(tr, npoints, off, total):
    """the packed trajectory arrays, made by rays_hip_pack_device"""
    import torch

    p = tr.params
    pv = torch.empty((max(total, 1), p.nv), dtype=torch.float64, device="cuda")   # (never a null pointer)
    pr = torch.empty(max(total, 1), dtype=torch.float64, device="cuda")
    hip.pack_device(tr.nray, p.nv, p.nstep_max, npoints.data_ptr(), off.data_ptr(), tr.ray_vec.data_ptr(),
                    tr.residual.data_ptr(), pv.data_ptr(), pr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return pv, pr


def _packed_run(tr, fields=None, npoints=None, packed_input=False, out_stride=None, buffer_len=None):
    """The raw entry on a prefilled buffer: (buffer as numpy [buffer_len], offsets, first_bad_point, total, names)."""
    import torch

    p = tr.params
    npoints = tr.npoints if npoints is None else npoints
    off = _offsets(tr, npoints)
    total = int(off[-1].item())
    _, names = hip.diag_field_mask(fields)
    out_stride = total if out_stride is None else out_stride
    n = len(names) * max(out_stride, 0) if buffer_len is None else buffer_len
    buf = _prefilled(torch, n + 1)   # one slot behind the buffer proper: never a null pointer (total = 0), never written
    bad = torch.full((tr.nray,), -7, dtype=torch.int32, device="cuda")
    rv, res = _pack(tr, npoints, off, total) if packed_input else (tr.ray_vec, tr.residual)
    hip.ray_diagnostics_packed_device(p, tr.nray, rv.data_ptr(), res.data_ptr(), npoints.data_ptr(), off.data_ptr(),
                                      out_stride, fields, buf.data_ptr(), bad.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream, packed_input=packed_input)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert _untouched(h[n:]).all(), "a store behind the buffer"
    return h[:n], off.cpu().numpy(), bad.cpu().numpy(), total, names


def _padded_run(tr, fields=None, npoints=None):
    """the padded entry on the same arrays: ({name: [nray][npt]}, first_bad_point)"""
    import torch

    p = tr.params
    npoints = tr.npoints if npoints is None else npoints
    _, names = hip.diag_field_mask(fields)
    out = torch.empty((len(names), tr.nray, p.nstep_max + 1), dtype=torch.float64, device="cuda")
    bad = torch.empty(tr.nray, dtype=torch.int32, device="cuda")
    hip.ray_diagnostics_device(p, tr.nray, tr.ray_vec.data_ptr(), tr.residual.data_ptr(), npoints.data_ptr(), fields,
                               out.data_ptr(), bad.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    return {n: h[k] for k, n in enumerate(names)}, bad.cpu().numpy()


def _live(npoints, npt):
    return np.arange(npt)[None, :] < np.clip(np.asarray(npoints), 0, npt)[:, None]


def _check_against_padded(what, tr, npoints_host, npoints_dev=None, layouts=(False, True)):
    """both input layouts of the packed entry against the padded entry at the recorded points, every field"""
    npt = tr.params.nstep_max + 1
    want, want_bad = _padded_run(tr, None, npoints_dev)
    live = _live(npoints_host, npt)
    want_off = np.concatenate([[0], np.cumsum(np.clip(npoints_host, 0, npt), dtype=np.int64)])
    for packed_input in layouts:
        buf, off, bad, total, names = _packed_run(tr, None, npoints_dev, packed_input)
        np.testing.assert_array_equal(off, want_off)
        assert total == off[-1] == int(np.clip(npoints_host, 0, npt).sum())
        got = buf.reshape(len(names), total)
        for k, name in enumerate(names):
            dx.assert_bits(got[k], want[name][live], f"{what} {name} packed_input={packed_input}")
        np.testing.assert_array_equal(bad, want_bad)
    return total


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_packed_equals_padded_at_the_recorded_points(name):
    """(a) every fixture, all nineteen fields, both input layouts (the packed input made by rays_hip_pack_device);
    offsets = numpy's exclusive cumsum with the total in offsets[nray]; first_bad_point = the padded run's.  Then
    DeviceTrace.diagnostics(packed=True): the same values in tensors of exactly `total` elements."""
    g, p, tr = _traced(name)
    npts = tr.npoints.cpu().numpy()
    np.testing.assert_array_equal(npts, g["npoints"])
    total = _check_against_padded(name, tr, npts)
    assert total == int(npts.sum()) > 0
    want, want_bad = _padded_run(tr)
    d = tr.diagnostics(packed=True)
    assert set(d) == set(hip.DIAG_FIELDS) | {"offsets", "first_bad_point"}
    live = _live(npts, p.nstep_max + 1)
    for k in hip.DIAG_FIELDS:
        assert tuple(d[k].shape) == (total,)
        dx.assert_bits(d[k].cpu().numpy(), want[k][live], f"{name} {k} DeviceTrace.diagnostics(packed=True)")
    np.testing.assert_array_equal(d["offsets"].cpu().numpy(), hip.diag_offsets(npts))
    np.testing.assert_array_equal(d["first_bad_point"].cpu().numpy(), want_bad)


def test_chunk_and_ray_edges():
    """(b) 1: npoints overwritten on the device -- runs of empty rays, rays that end on, before and after a wave
    boundary, a wave that spans four rays.  The points are independent, so the truncated arrays are valid input."""
    import torch

    g, p, tr = _traced("gold_solovev64_damp_rk4")
    npts = tr.npoints.cpu().numpy()
    assert tr.nray == 13 == len(EDGE_NPOINTS) and p.nv == 8 and npts.min() >= 145
    dev = torch.as_tensor(np.array(EDGE_NPOINTS, dtype=np.int32)).cuda()
    total = _check_against_padded("edges", tr, np.array(EDGE_NPOINTS), dev)
    assert total == sum(EDGE_NPOINTS)
    # a negative count is an empty ray, as in the padded entry (the padded input only: rays_hip_pack_device takes
    # npoints as it is; the upper clamp is an integer matter: test_point_offsets_over_several_tiles)
    wild = np.array(EDGE_NPOINTS, dtype=np.int32)
    wild[8] = -5
    _check_against_padded("clamped", tr, wild, torch.as_tensor(wild).cuda(), layouts=(False,))


@pytest.mark.parametrize("packed_input", [False, True])
def test_all_zero_npoints_write_nothing(packed_input):
    """(b) 2"""
    import torch

    g, p, tr = _traced("gold_solovev64_damp_rk4")
    zero = torch.zeros(tr.nray, dtype=torch.int32, device="cuda")
    buf, off, bad, total, names = _packed_run(tr, None, zero, packed_input, out_stride=500, buffer_len=19 * 500)
    assert total == 0 and not off.any() and len(off) == tr.nray + 1
    assert _untouched(buf).all()
    assert not bad.any()
    # the Python layers on a fan without a recorded point: empty fields, no bad point
    res = tr.results()
    res.npoints[:] = 0
    tr.npoints.zero_()
    d = res.diagnostics(p, ("s",), packed=True) if packed_input else tr.diagnostics(("s",), packed=True)
    assert tuple(d["s"].shape) == (0,) and len(d["offsets"]) == tr.nray + 1
    assert not np.asarray(d["offsets"].cpu() if not packed_input else d["offsets"]).any()
    assert not np.asarray(d["first_bad_point"].cpu() if not packed_input else d["first_bad_point"]).any()


@pytest.mark.parametrize("name", ["gold_slab_one_ray_rk4", "gold_solovev64_damp_grad_rk4",
                                  "gold_slab16_damp_multi_grad_rk4"])
def test_one_ray_and_other_row_widths(name):
    """(b) 3, 4: one ray of 501 points; nv = 13 and nv = 15 for the LDS row pad.  With the edge counts as far as the
    fixture's rays reach, so that waves span rays at these widths too."""
    import torch

    g, p, tr = _traced(name)
    npts = tr.npoints.cpu().numpy()
    if name == "gold_slab_one_ray_rk4":
        assert tr.nray == 1 and npts[0] == 501
    else:
        assert p.nv == (13 if "solovev" in name else 15)
    _check_against_padded(name, tr, npts)
    # (the list forwards gives the single ray no point at all -- a fan without a recorded point --, backwards 64)
    for edge in (EDGE_NPOINTS, EDGE_NPOINTS[::-1]):
        cut = np.minimum(npts, np.resize(np.array(edge, dtype=np.int32), tr.nray)).astype(np.int32)
        _check_against_padded(name + " cut", tr, cut, torch.as_tensor(cut).cuda())


@pytest.mark.parametrize("packed_input", [False, True])
def test_capacity_guard(packed_input):
    """(c) no store at or beyond out_stride of a field.  The buffers are large enough throughout: this checks the
    bound on the stores, it provokes nothing."""
    g, p, tr = _traced("gold_solovev64_damp_rk4")
    full, off, _, total, names = _packed_run(tr, None, None, packed_input)
    full = full.reshape(19, total)
    assert not _untouched(full).any()
    # larger: the tail [total, out_stride) of every field is intact
    big = total + 333
    buf = _packed_run(tr, None, None, packed_input, out_stride=big)[0].reshape(19, big)
    assert _untouched(buf[:, total:]).all()
    for k, name in enumerate(names):
        dx.assert_bits(buf[k, :total], full[k], f"{name} out_stride = total + 333")
    # smaller, in a buffer of the full size: field k is [k * small, (k + 1) * small), cut at `small` points; behind
    # the nineteenth field nothing is written
    small = total - 70
    buf = _packed_run(tr, None, None, packed_input, out_stride=small, buffer_len=19 * total)[0]
    assert _untouched(buf[19 * small:]).all()
    rows = buf[:19 * small].reshape(19, small)
    for k, name in enumerate(names):
        dx.assert_bits(rows[k], full[k, :small], f"{name} out_stride = total - 70")
    # out_stride = 0: nothing at all
    buf = _packed_run(tr, None, None, packed_input, out_stride=0, buffer_len=64)[0]
    assert _untouched(buf).all()


@pytest.mark.parametrize("name", ["gold_axisym64_eqdsk_damp_rk4", "gold_slab16_fast_rk4"])
def test_field_subsets_equal_the_full_run(name):
    """(d), and RayResults.diagnostics(packed=True) on the host arrays"""
    g, p, tr = _traced(name)
    full, off, bad, total, names = _packed_run(tr)
    full = dict(zip(names, full.reshape(19, total)))
    for sel in (("n_imag", "Psi", "s"), ("residual",)):
        for packed_input in (False, True):
            buf, _, sub_bad, _, sub_names = _packed_run(tr, sel, None, packed_input, buffer_len=(len(sel) + 1) * total)
            assert _untouched(buf[len(sel) * total:]).all(), f"{name} {sel}: stores behind the selected fields"
            assert set(sub_names) == set(sel)
            for k, key in enumerate(sub_names):
                dx.assert_bits(buf[k * total:(k + 1) * total], full[key], f"{name} {key} selected as {sel}")
            np.testing.assert_array_equal(sub_bad, bad)
    res = tr.results()
    host = res.diagnostics(p, ("xi_1", "s"), packed=True)
    assert set(host) == {"xi_1", "s", "offsets", "first_bad_point"}
    dx.assert_bits(host["xi_1"], full["xi_1"], "RayResults.diagnostics(packed=True)")
    dx.assert_bits(host["s"], full["s"], "RayResults.diagnostics(packed=True)")
    np.testing.assert_array_equal(host["offsets"], off)
    np.testing.assert_array_equal(host["first_bad_point"], bad)
    padded = hip.diag_unpack(host, host["offsets"], p.nstep_max + 1)
    dx.assert_bits(padded["xi_1"], res.diagnostics(p, ("xi_1",))["xi_1"], "scattered back to the padded layout")


def test_bad_arguments_are_refused():
    """(e) the padded entry's texts, plus a negative out_stride and an unknown input layout"""
    g, nml, p = load_golden("gold_axisym64_eqdsk_damp_rk4")
    lib = hip.load()
    f = lib.rays_hip_ray_diagnostics_packed_device
    with pytest.raises(hip.RaysHipError, match="selects no field"):
        hip._check(f(C.byref(p), 0, 0, None, None, None, None, 0, 0, None, None, None), "diag")
    with pytest.raises(hip.RaysHipError, match="selects no field"):
        hip._check(f(C.byref(p), 0, 0, None, None, None, None, 0, 1 << 19, None, None, None), "diag")
    with pytest.raises(hip.RaysHipError, match="null device pointer"):
        hip._check(f(C.byref(p), 4, 0, None, None, None, None, 8, 1, None, None, None), "diag")
    with pytest.raises(hip.RaysHipError, match="out_stride < 0"):
        hip._check(f(C.byref(p), 0, 0, None, None, None, None, -1, 1, None, None, None), "diag")
    with pytest.raises(hip.RaysHipError, match="in_layout"):
        hip._check(f(C.byref(p), 0, 2, None, None, None, None, 0, 1, None, None, None), "diag")
    with pytest.raises(hip.RaysHipError, match="bad nray"):
        hip._check(f(C.byref(p), -1, 0, None, None, None, None, 0, 1, None, None, None), "diag")
    with pytest.raises(hip.RaysHipError, match="null device pointer"):
        hip.point_offsets_device(4, 10, 0, 0)
    with pytest.raises(hip.RaysHipError, match="bad nray"):
        hip.point_offsets_device(-1, 10, 0, 0)
    g, nml, p = load_golden("cfg1_slab16_rk4")
    assert f(C.byref(p), 0, 0, None, None, None, None, 0, 1, None, None, None) == 0   # no rays: nothing to do


def test_point_offsets_over_several_tiles():
    """The prefix sum where its three passes all run: 5000 rays are three tiles of 2048, the last one partial; counts
    outside 0 .. nstep_max + 1 are clamped; nray = 0 writes the single 0; nray = 2048 and 2049 sit on a tile edge."""
    import torch

    rng = np.random.default_rng(7)
    n = rng.integers(-3, 260, size=5000).astype(np.int32)
    n[rng.random(5000) < 0.3] = 0
    for nray in (0, 1, 2047, 2048, 2049, 4096, 5000):
        dev = torch.as_tensor(n[:nray]).cuda()
        off = torch.full((nray + 2,), -1, dtype=torch.int64, device="cuda")
        hip.point_offsets_device(nray, 200, dev.data_ptr(), off.data_ptr(), torch.cuda.current_stream().cuda_stream)
        got = off.cpu().numpy()
        np.testing.assert_array_equal(got[:-1], hip.diag_offsets(n[:nray], 200), err_msg=f"nray = {nray}")
        assert got[-1] == -1


def test_fortran_driver_reproduces_the_python_path(tmp_path):
    """(f) tests/fortran/ray_diagnostics_packed_driver.f90 (our own source) + the binding, built with amdflang and
    linked against librays_hip.so and the HIP runtime, fed one fixture's arrays in both input layouts: offsets, the
    nineteen packed fields and first_bad_point equal the Python packed path's bit for bit."""
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    libdir = os.path.join(ROOT, "rays_amd", "lib")
    hipdir = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    srcs = [os.path.join(ROOT, "fortran", "rays_hip_m.f90"),
            os.path.join(ROOT, "tests", "fortran", "ray_diagnostics_packed_driver.f90")]
    exe = str(tmp_path / "ray_diagnostics_packed_driver")
    subprocess.check_call([fc, "-O2", "-ffp-contract=off", "-w", "-o", exe] + srcs +
                          ["-L" + libdir, "-lrays_hip", "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath," + hipdir], cwd=str(tmp_path))
    name = "gold_solovev64_damp_rk4"
    g, p, tr = _traced(name)
    want, want_off, want_bad, total, names = _packed_run(tr)
    want = want.reshape(19, total)
    res = tr.results()
    nray, npt, nv = res.ray_vec.shape
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    fspl = np.ascontiguousarray(z["fspl_re"], dtype=np.float64)
    nx = len(fspl) if p.damping_model else 0
    for layout in (hip.DIAG_IN_PADDED, hip.DIAG_IN_PACKED):
        fin, fout = str(tmp_path / f"in{layout}.bin"), str(tmp_path / f"out{layout}.bin")
        with open(fin, "wb") as f:
            f.write(np.array([nray, npt, nv, layout, nx], dtype=np.int32).tobytes())
            f.write(bytes(p))
            if nx:
                f.write(np.array([float(z["x_min"]), float(z["x_max"])]).tobytes())
                f.write(fspl.tobytes())
            f.write(np.ascontiguousarray(res.ray_vec).tobytes())
            f.write(np.ascontiguousarray(res.residual).tobytes())
            f.write(res.npoints.astype(np.int32).tobytes())
        r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        raw = np.fromfile(fout, dtype=np.uint8)
        n_off, n_out = 8 * (nray + 1), 8 * 19 * total
        assert raw.size == n_off + n_out + 4 * nray
        np.testing.assert_array_equal(raw[:n_off].view(np.int64), want_off)
        got = raw[n_off:n_off + n_out].view(np.float64).reshape(19, total)
        for k, key in enumerate(names):
            dx.assert_bits(got[k], want[k], f"{name} Fortran, in_layout {layout}, field {key}")
        np.testing.assert_array_equal(raw[n_off + n_out:].view(np.int32), want_bad)


def test_full_size_fan():
    """(g) cfg 5b, 262144 rays: the packed form on the padded trace arrays equals the padded entry gathered at the
    recorded points on every 64th ray, and exactly npoints.sum() slots of every field are written."""
    import torch

    path = os.path.join(ROOT, "configs", "cfg5b_axisym256k_rk4_damp.in")
    run = RaysRun.from_namelist(path)
    assert run.nray == 262144
    p = run.params
    tr = DeviceTrace(p, run.rvec0, run.rindex_vec0)
    tr.launch()
    npts = tr.npoints.cpu().numpy().astype(np.int64)
    total, npt = int(npts.sum()), p.nstep_max + 1
    off = _offsets(tr)
    want_off = np.concatenate([[0], np.cumsum(npts)])
    np.testing.assert_array_equal(off.cpu().numpy(), want_off)
    stride = total + 4096
    buf = _prefilled(torch, 19 * stride)
    bad = torch.empty(tr.nray, dtype=torch.int32, device="cuda")
    hip.ray_diagnostics_packed_device(p, tr.nray, tr.ray_vec.data_ptr(), tr.residual.data_ptr(), tr.npoints.data_ptr(),
                                      off.data_ptr(), stride, None, buf.data_ptr(), bad.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows = buf.view(torch.int64).view(19, stride)
    written = (rows != PREFILL).sum(dim=1).cpu().numpy()
    np.testing.assert_array_equal(written, np.full(19, total))
    assert bool((rows[:, total:] == PREFILL).all().item())
    assert not bad.any().item()
    padded = tr.diagnostics()
    sel = np.arange(0, tr.nray, 64)
    live = _live(npts[sel], npt)
    flat = np.concatenate([want_off[r] + np.arange(npts[r]) for r in sel])   # ray by ray, point by point: live's order
    d_sel, d_flat = torch.as_tensor(sel, device="cuda"), torch.as_tensor(flat, device="cuda")
    got = buf.view(19, stride)
    for k, name in enumerate(hip.DIAG_FIELDS):
        dx.assert_bits(got[k][d_flat].cpu().numpy(), padded[name][d_sel].cpu().numpy()[live], f"cfg 5b {name}")
    assert len(flat) == int(npts[sel].sum()) > 0
