"""ctypes wrapper around tests/hip_emul/librays_emul.so: the PRODUCT kernel source compiled for the
host (one lane per wave) -- test infrastructure for the CPU tier and for sanitizer runs."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from rays_amd.params import RaysFan, RaysParams
from tests import emul_build as eb
from tests.emul_build import d as _d, i as _i

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(_ROOT, "tests", "hip_emul")
_LIB = os.path.join(_DIR, "librays_emul.so")
_lib = None
# second build of the same sources with the SG kernel's fast storage tiers shrunk (rays_sg.hpp:
# coefficient entries <= 2 and 2 + 1 phi rows instead of <= 8 and 4 + 4), so that ordinary rays
# cross every tier boundary
_TIERS_LIB = os.path.join(_DIR, "librays_emul_tiers.so")
_TIERS_DEFS = ["-DRAYS_SG_TIER=2", "-DRAYS_SG_REG_ROWS=2", "-DRAYS_SG_LDS_ROWS=1"]
_tiers_lib = None


def build(sanitize: bool = False, out: str = None, defs=()):
    eb.build("emul_trace.cpp", _LIB if out is None else out, defs, sanitize)


def _load(path):
    lib = eb.load(path)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.rays_emul_trace.restype = C.c_int
    lib.rays_emul_trace.argtypes = [C.POINTER(RaysParams), C.c_int, dp, dp, dp, dp, ip, ip, dp, dp, dp]
    lib.rays_emul_trace_ex.restype = C.c_int
    lib.rays_emul_trace_ex.argtypes = [C.POINTER(RaysParams), C.c_int, dp, dp, dp, dp, ip, ip, dp, dp, dp,
                                       dp, dp, dp, C.c_int]
    lib.rays_emul_ray_init.restype = C.c_int
    lib.rays_emul_ray_init.argtypes = [C.POINTER(RaysParams), C.POINTER(RaysFan), C.c_int, dp, dp, ip]
    lib.rays_emul_deposition.restype = C.c_int
    lib.rays_emul_deposition.argtypes = [C.POINTER(RaysParams), C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, dp, C.c_int, dp, dp]
    return lib


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = _load(_LIB)
    return _lib


def tiers_lib():
    global _tiers_lib
    if _tiers_lib is None:
        build(out=_TIERS_LIB, defs=_TIERS_DEFS)
        _tiers_lib = _load(_TIERS_LIB)
    return _tiers_lib


def set_axisym_tables(tab: dict, small_tiers: bool = False):
    eb.set_axisym_tables(tiers_lib() if small_tiers else lib(), tab)


def _offset_zeros(shape, offset):
    """zeros of `shape` whose first element sits `offset` doubles past a 64-byte boundary"""
    n = int(np.prod(shape))
    raw = np.zeros(n + 16)
    skew = (-(raw.ctypes.data // 8) + offset) % 8
    return raw[skew:skew + n].reshape(shape)


def trace(p: RaysParams, rvec0, rindex_vec0, small_tiers: bool = False, vec_offset: int = 0, res_offset: int = 0) -> dict:
    """vec_offset / res_offset: position of the two trajectory arrays within a 64-byte sector, in doubles
    (the RK4 kernel's PointWindow writes whole sectors of the global address)."""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    nray, nv, npt = len(rvec0), p.nv, p.nstep_max + 1
    out = eb.trace_outputs(nray, nv, npt)
    out["ray_vec"], out["residual"] = _offset_zeros((nray, npt, nv), vec_offset), _offset_zeros((nray, npt), res_offset)
    rc = (tiers_lib() if small_tiers else lib()).rays_emul_trace(C.byref(p), nray, _d(rvec0), _d(rindex_vec0),
                                                                 *eb.trace_args(out))
    if rc:
        raise RuntimeError(f"rays_emul_trace rc={rc}")
    return out


def _trace_ex(p, nray, rvec0, rindex_vec0, out, v0=None, s0=None, ds_run=None, rays_per_run=0):
    rc = lib().rays_emul_trace_ex(C.byref(p), nray, _d(rvec0), _d(rindex_vec0), *eb.trace_args(out), _d(v0), _d(s0),
                                  _d(ds_run), int(rays_per_run))
    if rc:
        raise RuntimeError(f"rays_emul_trace_ex rc={rc}")


def scan(p: RaysParams, rvec0, rindex_vec0, ds_values) -> dict:
    """The fused scan's launch (rays_hip_scan_device: run = ray // nray, ds per run) through the kernel source on
    the host; arrays carry a leading run dimension."""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    ds = np.ascontiguousarray(ds_values, dtype=np.float64)
    nray, R = len(rvec0), len(ds)
    out = eb.trace_outputs(R * nray, p.nv, p.nstep_max + 1)
    _trace_ex(p, R * nray, rvec0, rindex_vec0, out, ds_run=ds, rays_per_run=nray)
    return {k: v.reshape((R, nray) + v.shape[1:]) for k, v in out.items()}


def ode_step(p: RaysParams, v0, s0=None):
    """rays_hip_ode_step_device's launch (nstep_max = 1 from the caller's states) on the host:
    (v1, resid, stop_code) with stop_code 0 where the step was taken and kept."""
    from rays_amd.params import copy_params
    v0 = np.ascontiguousarray(v0, dtype=np.float64).reshape(-1, p.nv)
    s0 = None if s0 is None else np.ascontiguousarray(s0, dtype=np.float64)
    q = copy_params(p)
    q.nstep_max = 1
    q.s_max = 1.7976931348623157e308
    n = len(v0)
    out = eb.trace_outputs(n, p.nv, 2)
    _trace_ex(q, n, v0, v0, out, v0=v0, s0=s0)
    ok = out["npoints"] == 2
    return (np.where(ok[:, None], out["ray_vec"][:, 1], 0.0), np.where(ok, out["residual"][:, 1], 0.0),
            np.where(ok, 0, out["stop_code"]).astype(np.int32))


def ray_init(p: RaysParams, fan: RaysFan, nray_max: int):
    """The device launcher's per-member function (rays_ray_init.hpp: fan_member) run on the host."""
    n = int(nray_max)
    rvec0, rindex_vec0 = np.zeros((n, 3)), np.zeros((n, 3))
    nray = C.c_int32(0)
    rc = lib().rays_emul_ray_init(C.byref(p), C.byref(fan), n, _d(rvec0), _d(rindex_vec0), C.byref(nray))
    if rc:
        raise RuntimeError(f"rays_emul_ray_init rc={rc}")
    return rvec0[:nray.value].copy(), rindex_vec0[:nray.value].copy()


def deposition(p: RaysParams, which: int, n_bins: int, ray_vec, npoints, power, rho_grid, rho_fspl):
    """rays_deposition.hpp: deposit_ray + the ray-ordered profile sum, run on the host.
    ray_vec[nray][nstep_max+1][nv] (padded reference layout)."""
    nray = len(npoints)
    ray_vec = np.ascontiguousarray(ray_vec, dtype=np.float64)
    npoints = np.ascontiguousarray(npoints, dtype=np.int32)
    power = np.ascontiguousarray(power, dtype=np.float64)
    rho_grid = np.ascontiguousarray(rho_grid, dtype=np.float64)
    rho_fspl = np.ascontiguousarray(rho_fspl, dtype=np.float64)
    work, profile = np.zeros((nray, n_bins)), np.zeros(n_bins)
    rc = lib().rays_emul_deposition(C.byref(p), which, n_bins, nray, _d(ray_vec), _i(npoints), _d(power), _d(rho_grid),
                                    _d(rho_fspl), len(rho_grid), _d(work), _d(profile))
    if rc:
        raise RuntimeError(f"rays_emul_deposition rc={rc}")
    return work, profile
