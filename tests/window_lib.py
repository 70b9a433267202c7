"""TEST INFRASTRUCTURE ONLY: what the windowed-tracing tests share -- the saved ray state as numpy arrays, the ctypes
wrappers around the host emulation of the continuation kernels (tests/hip_emul/emul_window.cpp), and the assembly of a
full trace from point 1 and the windows' new points."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from rays_amd.params import RaysParams
from tests import emul_build as eb
from tests.emul_build import d as _d, i as _i
from tests.summary_lib import set_axisym_tables  # noqa: F401  (the same entry of the emulation libraries)

STATE_KEYS = ("v", "s", "nstep", "stop_code", "resid", "sg_err", "flags")
SUMMARY_KEYS = ("npoints", "stop_code", "end_ray_vec", "end_residuals", "max_residuals")
REFUSED = 1   # include/rays_hip.h: RAYS_STATE_REFUSED

def _declare(lib, wave):
    dp, ip, pp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(RaysParams)
    state = [dp, dp, ip, ip, dp, dp, ip]
    if wave:
        lib.rays_emul_window_waves.restype = C.c_int
        lib.rays_emul_window_waves.argtypes = [pp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, *state, C.c_int, dp, dp, ip]
    else:
        lib.rays_emul_window.restype = C.c_int
        lib.rays_emul_window.argtypes = [pp, C.c_int, C.c_int, dp, dp, *state, C.c_int, dp, dp, ip, dp]


def emul_lib(wave: bool = False, tag: str = "", defs=()):
    """librays_emul_window[_wave][_<tag>].so, built on first use (extra -D switches get a library of their own)."""
    return eb.variant_lib("emul_window.cpp", "window", ["-DRAYS_RK4_NO_HANDOVER"], "-DRAYS_EMUL_WINDOW_WAVE=1", wave, tag,
                          defs, _declare)


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
