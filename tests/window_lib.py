"""TEST INFRASTRUCTURE ONLY: what the windowed-tracing tests share -- the saved ray state as numpy arrays, the ctypes
wrappers around the host emulation of the continuation kernels (tests/hip_emul/emul_window.cpp), and the assembly of a
full trace from point 1 and the windows' new points."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from rays_amd.params import RaysParams
from tests.common import ROOT
from tests.summary_lib import set_axisym_tables  # noqa: F401  (the same entry of the emulation libraries)

_DIR = os.path.join(ROOT, "tests", "hip_emul")
_CSRC = os.path.join(ROOT, "rays_amd", "csrc")
STATE_KEYS = ("v", "s", "nstep", "stop_code", "resid", "sg_err", "flags")
SUMMARY_KEYS = ("npoints", "stop_code", "end_ray_vec", "end_residuals", "max_residuals")
REFUSED = 1   # include/rays_hip.h: RAYS_STATE_REFUSED

_libs = {}
_SRCS = ["emul_window.cpp", "emul_trace.cpp", "emul_group.cpp", "hip/hip_runtime.h", "hip/hip_wave_emul.h"]
_PRODUCT = ["rays_libm.hpp", "rays_libm_tables.inc", "rays_device.hpp", "rays_device_arith.inc", "rays_trace.hpp",
            "rays_rk4.hpp", "rays_rk4_body.inc", "rays_rk4_pass.inc", "rays_rk4_take.inc", "rays_sg.hpp", "rays_sg_group.hpp",
            "rays_dev_params.inc"]


def emul_lib(wave: bool = False, tag: str = "", defs=()):
    """librays_emul_window[_wave][_<tag>].so, built on first use (extra -D switches get a library of their own)."""
    key = (wave, tag)
    if key in _libs:
        return _libs[key]
    path = os.path.join(_DIR, "librays_emul_window" + ("_wave" if wave else "") + (f"_{tag}" if tag else "") + ".so")
    srcs = [os.path.join(_DIR, f) for f in _SRCS] + [os.path.join(_CSRC, f) for f in _PRODUCT]
    if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-extern-tls-init",
                               "-fPIC", "-shared", "-w", "-DRAYS_RK4_NO_HANDOVER",
                               *(["-DRAYS_EMUL_WINDOW_WAVE=1"] if wave else []), *defs, "-I", _DIR, srcs[0], "-o", path])
    lib = C.CDLL(path)
    dp, ip, pp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(RaysParams)
    state = [dp, dp, ip, ip, dp, dp, ip]
    if wave:
        lib.rays_emul_window_waves.restype = C.c_int
        lib.rays_emul_window_waves.argtypes = [pp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, *state, C.c_int, dp, dp, ip]
    else:
        lib.rays_emul_window.restype = C.c_int
        lib.rays_emul_window.argtypes = [pp, C.c_int, C.c_int, dp, dp, *state, C.c_int, dp, dp, ip, dp]
    lib.rays_emul_set_zfun_table.restype = C.c_int
    lib.rays_emul_set_zfun_table.argtypes = [dp, C.c_int, C.c_double, C.c_double]
    from tests.emul_lib import _set_zfun
    _set_zfun(lib.rays_emul_set_zfun_table)
    _libs[key] = lib
    return lib


def _d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def new_state(nray: int, nv: int) -> dict:
    """Poisoned, not zeroed: state_init has to write every element."""
    return dict(v=np.full((nray, nv), np.nan), s=np.full(nray, np.nan), nstep=np.full(nray, -7, dtype=np.int32),
                stop_code=np.full(nray, -7, dtype=np.int32), resid=np.full((nray, 3), np.nan),
                sg_err=np.full((nray, 2), np.nan), flags=np.full(nray, -7, dtype=np.int32))


def _state_args(st):
    return [_d(st["v"]), _d(st["s"]), _i(st["nstep"]), _i(st["stop_code"]), _d(st["resid"]), _d(st["sg_err"]),
            _i(st["flags"])]


def state_bytes(st) -> bytes:
    return b"".join(np.ascontiguousarray(st[k]).tobytes() for k in STATE_KEYS)


def state_init(p: RaysParams, rvec0, rindex_vec0, lib=None):
    """rays_hip_state_init_device's launch on the host: (state, start_ray_vec)."""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    n = len(rvec0)
    st, start = new_state(n, p.nv), np.full((n, p.nv), np.nan)
    rc = (lib or emul_lib()).rays_emul_window(C.byref(p), 0, n, _d(rvec0), _d(rindex_vec0), *_state_args(st), 1, None,
                                              None, None, _d(start))
    if rc:
        raise RuntimeError(f"rays_emul_window (state_init) rc={rc}")
    return st, start


def window(p: RaysParams, st: dict, n_steps: int, recording: bool = True, lib=None, waves=None):
    """rays_hip_trace_window_device's launch on the host; the state is updated in place.  Returns (ray_vec_win,
    residual_win, npoints_win); the first two are None for a summary window.  waves = (kind, blocks, stride): whole
    emulated waves (kind 'rk4' | 'sg') of the wave library `lib` instead of one lane."""
    n, nv = len(st["s"]), st["v"].shape[1]
    rv = np.full((n, n_steps, nv), np.nan) if recording else None   # poisoned: nothing past npoints_win is compared
    res = np.full((n, n_steps), np.nan) if recording else None
    npw = np.full(n, -7, dtype=np.int32)
    mode = 1 if recording else 2
    if waves is None:
        rc = (lib or emul_lib()).rays_emul_window(C.byref(p), mode, n, None, None, *_state_args(st), int(n_steps), _d(rv),
                                                  _d(res), _i(npw), None)
    else:
        kind, blocks, stride = waves
        rc = (lib or emul_lib(wave=True)).rays_emul_window_waves(
            C.byref(p), mode, {"rk4": 0, "sg": 2}[kind], int(blocks), int(stride), n, *_state_args(st), int(n_steps),
            _d(rv), _d(res), _i(npw))
    if rc:
        raise RuntimeError(f"rays_emul_window rc={rc}")
    return rv, res, npw


def state_summaries(st: dict) -> dict:
    """The five summary arrays from a state, as rays_hip_state_summary_device's kernel forms them."""
    refused = (st["flags"] & REFUSED) != 0
    nstep = st["nstep"]
    return dict(npoints=(nstep + 1).astype(np.int32), stop_code=st["stop_code"].copy(),
                end_ray_vec=np.where(refused[:, None], 0.0, st["v"]),
                end_residuals=np.where(~refused & (nstep >= 1), st["resid"][:, 1], 0.0),
                max_residuals=np.where(refused, 0.0, st["resid"][:, 2]))


def trace_windowed(p: RaysParams, rvec0, rindex_vec0, sizes, policy="record", lib=None, waves=None, wave_lib=None,
                   max_windows=100000):
    """A whole trace in windows.  sizes: the n_steps values, cycled.  policy: 'record' (every window records),
    'summary' (none does) or 'mixed' (recording and summary windows alternate, recording first).  Returns the full
    arrays (nan where no recording window covered a point, `covered` says which points one did), the state's
    summaries, the state and start_ray_vec.  The state is initialised on one lane; waves / wave_lib as in window()."""
    st, start = state_init(p, rvec0, rindex_vec0, lib=lib)
    n, nv, npt = len(start), p.nv, p.nstep_max + 1
    ray_vec, residual = np.full((n, npt, nv), np.nan), np.full((n, npt), np.nan)
    covered = np.zeros((n, npt), dtype=bool)
    ray_vec[:, 0], residual[:, 0], covered[:, 0] = start, 0.0, True
    have = np.ones(n, dtype=np.int64)
    for k, w in enumerate(itertools.cycle(sizes)):
        assert k < max_windows
        if not (st["stop_code"] == 0).any():
            break
        rec = policy == "record" or (policy == "mixed" and k % 2 == 0)
        rv, res, npw = window(p, st, w, rec, lib=wave_lib if waves else lib, waves=waves)
        assert (npw >= 0).all() and (npw <= w).all()
        if rec:
            for r in np.nonzero(npw)[0]:
                a, m = have[r], npw[r]
                ray_vec[r, a:a + m], residual[r, a:a + m], covered[r, a:a + m] = rv[r, :m], res[r, :m], True
        have += npw
    out = state_summaries(st)
    assert np.array_equal(have, out["npoints"])
    out.update(ray_vec=ray_vec, residual=residual, covered=covered, state=st, start_ray_vec=start)
    return out
