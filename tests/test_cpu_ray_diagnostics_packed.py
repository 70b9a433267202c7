"""CPU tier of the packed ray diagnostics (include/rays_hip.h: rays_hip_ray_diagnostics_packed_device): the locator of
rays_amd/csrc/rays_diag.hpp compiled for the host (tests/hip_emul/emul_diag_locate.cpp) against numpy's searchsorted
at every flat index, the host scatter helpers, and the NetCDF writer fed the packed dictionary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rays_amd import hip, results
from tests.common import ROOT

_DIR = os.path.join(ROOT, "tests", "hip_emul")
_lib = None

# the npoints of the GPU tier's chunk-and-ray-edge case: runs of empty rays, rays ending on, before and after a wave
# boundary, a wave that spans four rays
EDGE_NPOINTS = [0, 1, 63, 64, 65, 127, 128, 129, 0, 0, 145, 2, 64]


def _locator():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _DIR, "-f", "Makefile.diag_locate"])
        lib = C.CDLL(os.path.join(_DIR, "librays_emul_diag_locate.so"))
        lp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
        lib.rays_emul_diag_locate.argtypes = [lp, C.c_int, ip]
        lib.rays_emul_diag_locate.restype = None
        lib.rays_emul_diag_locate_wave.argtypes = [lp, C.c_int, C.c_int, ip]
        lib.rays_emul_diag_locate_wave.restype = None
        _lib = lib
    return _lib


def _random_rays():
    rng = np.random.default_rng(20261017)
    n = rng.integers(1, 200, size=1000)
    n[rng.random(1000) < 0.3] = 0
    return [int(x) for x in n]


LOCATOR_CASES = {
    "edges": EDGE_NPOINTS,
    "empty_prefix": [0, 0, 0, 0, 5, 64, 1],
    "empty_suffix": [5, 64, 1, 0, 0, 0, 0],
    "empty_both": [0, 0, 7, 0, 0],
    "one_ray": [501],
    "one_point_rays": [1] * 200 + [0] * 70 + [1] * 3,   # waves that span 64 rays and a long run of empties
    "random_1000": _random_rays(),
}


@pytest.mark.parametrize("case", list(LOCATOR_CASES))
def test_locator_equals_searchsorted_at_every_flat_index(case):
    npoints = np.array(LOCATOR_CASES[case], dtype=np.int64)
    if case == "random_1000":
        assert len(npoints) == 1000 and 0.2 < (npoints == 0).mean() < 0.4
    offsets = hip.diag_offsets(npoints)
    nray, total = len(npoints), int(offsets[-1])
    assert total == npoints.sum() > 0
    want = (np.searchsorted(offsets, np.arange(total), side="right") - 1).astype(np.int32)
    assert (npoints[want] > 0).all()   # an empty ray is never the answer
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    lp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
    got = np.full(total, -1, dtype=np.int32)
    _locator().rays_emul_diag_locate(off.ctypes.data_as(lp), nray, got.ctypes.data_as(ip))
    np.testing.assert_array_equal(got, want)
    for wave in (64, 1, 7):
        got = np.full(total, -1, dtype=np.int32)
        _locator().rays_emul_diag_locate_wave(off.ctypes.data_as(lp), nray, wave, got.ctypes.data_as(ip))
        np.testing.assert_array_equal(got, want, err_msg=f"from the first ray of runs of {wave}")


def test_diag_offsets_clamps_like_the_device_entry():
    np.testing.assert_array_equal(hip.diag_offsets([3, -2, 9, 0, 4], nstep_max=4), [0, 3, 3, 8, 8, 12])
    np.testing.assert_array_equal(hip.diag_offsets([]), [0])
    assert hip.diag_offsets([1, 2]).dtype == np.int64


def _synthetic(npoints, npt, seed=5):
    """a padded dictionary as RayResults.diagnostics returns it: values at the recorded points, +0.0 elsewhere"""
    rng = np.random.default_rng(seed)
    npoints = np.asarray(npoints, dtype=np.int32)
    live = np.arange(npt)[None, :] < npoints[:, None]
    diag = {}
    for k in hip.DIAG_FIELDS:
        a = np.zeros((len(npoints), npt))
        a[live] = rng.standard_normal(int(live.sum()))
        diag[k] = a
    diag["Psi"][live] = -0.0   # a sign bit the scatter must keep
    diag["first_bad_point"] = np.arange(len(npoints), dtype=np.int32) % 3
    return diag, live


def test_scatter_helpers_round_trip():
    npt = 150
    diag, live = _synthetic(EDGE_NPOINTS, npt)
    packed = hip.diag_pack(diag, EDGE_NPOINTS)
    np.testing.assert_array_equal(packed["offsets"], hip.diag_offsets(EDGE_NPOINTS))
    assert set(packed) == set(diag) | {"offsets"}
    for k in hip.DIAG_FIELDS:
        assert packed[k].shape == (int(np.sum(EDGE_NPOINTS)),)
        np.testing.assert_array_equal(packed[k].view(np.uint64), diag[k][live].view(np.uint64))
    back = hip.diag_unpack(packed, packed["offsets"], npt)
    assert set(back) == set(diag)
    for k in hip.DIAG_FIELDS:
        np.testing.assert_array_equal(back[k].view(np.uint64), diag[k].view(np.uint64), err_msg=k)
    np.testing.assert_array_equal(back["first_bad_point"], diag["first_bad_point"])
    again = hip.diag_pack(back, EDGE_NPOINTS)
    for k in hip.DIAG_FIELDS:
        np.testing.assert_array_equal(again[k].view(np.uint64), packed[k].view(np.uint64))
    # a packed array with spare capacity behind the total (out_stride > total) unpacks the same
    roomy = dict(packed, s=np.concatenate([packed["s"], np.full(9, np.nan)]))
    np.testing.assert_array_equal(hip.diag_unpack(roomy, packed["offsets"], npt)["s"], diag["s"])
    with pytest.raises(ValueError, match="offsets"):
        hip.diag_unpack(packed, packed["offsets"], 100)   # a ray of 145 points does not fit 100 slots
    with pytest.raises(ValueError, match="shape"):
        hip.diag_unpack(dict(packed, s=packed["s"][:-1]), packed["offsets"], npt)


@pytest.mark.parametrize("slab", [False, True])
def test_netcdf_file_from_the_packed_dictionary_is_byte_identical(tmp_path, slab):
    npt = 150
    diag, _ = _synthetic(EDGE_NPOINTS, npt)
    packed = hip.diag_pack(diag, EDGE_NPOINTS)
    date = [2026, 10, 17, 0, 12, 0, 0, 0]
    a, b = str(tmp_path / "padded.nc"), str(tmp_path / "packed.nc")
    results.write_ray_diagnostics_NC(a, diag, EDGE_NPOINTS, 8, run_label="lbl", date_vector=date, slab=slab)
    results.write_ray_diagnostics_NC(b, packed, EDGE_NPOINTS, 8, run_label="lbl", date_vector=date, slab=slab)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        da, db = fa.read(), fb.read()
    assert len(da) > 17 * 13 * 145 * 8 and da == db
    with pytest.raises(ValueError, match="offsets"):
        results.write_ray_diagnostics_NC(b, packed, EDGE_NPOINTS[::-1], 8, date_vector=date, slab=slab)


def test_fortran_binding_and_packed_driver_compile(tmp_path):
    """amdflang -c fortran/rays_hip_m.f90 tests/fortran/ray_diagnostics_packed_driver.f90"""
    import shutil

    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    subprocess.check_call([fc, "-c", "-w", os.path.join(ROOT, "fortran", "rays_hip_m.f90"),
                           os.path.join(ROOT, "tests", "fortran", "ray_diagnostics_packed_driver.f90")], cwd=str(tmp_path))
