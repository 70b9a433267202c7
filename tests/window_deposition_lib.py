"""TEST INFRASTRUCTURE ONLY: what the deposition-window tests share -- the ctypes wrappers around the host emulation of
the continuation variant of the fused deposition kernels (tests/hip_emul/emul_window_deposition.cpp: the saved state in
the TraceArgs slots of windowed tracing, the DepTraceArgs / Dep2TraceArgs block in the ray_vec slot, work rows that no
launch zeroes), and a whole run in windows.  The library also holds the one-shot fused entries, so fl.emul_fused(...,
lib=emul_lib()) and pl.emul_profiles(..., lib=emul_lib()) compare both paths on one set of tables."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from rays_amd.params import RaysParams
from tests import emul_build as eb
from tests import fused_deposition_lib as fl
from tests import fused_profiles_lib as pl
from tests import summary_lib as sl
from tests import window_lib as wl

SRC = "emul_window_deposition.cpp"


def declare(lib, wave):
    pl.declare(lib, wave)
    dp, ip, pp, cp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(RaysParams), C.POINTER(C.c_int)
    state = [dp, dp, ip, ip, dp, dp, ip]
    tail = [C.c_int, dp, C.c_int, cp, cp, dp, dp, C.c_int, dp, dp, ip]
    if wave:
        lib.rays_emul_window_deposition_waves.restype = C.c_int
        lib.rays_emul_window_deposition_waves.argtypes = [pp, C.c_int, C.c_int, C.c_int, C.c_int, *state, *tail]
    else:
        lib.rays_emul_window_deposition.restype = C.c_int
        lib.rays_emul_window_deposition.argtypes = [pp, C.c_int, C.c_int, dp, dp, *state, *tail, dp]


def emul_lib(wave: bool = False):
    """librays_emul_windep[_wave].so, built on first use."""
    return eb.variant_lib(SRC, "windep", pl.BASE_DEFS, pl.WAVE_DEF, wave, "", (), declare)


def state_init(p: RaysParams, rvec0, rindex_vec0, lib=None):
    """rays_hip_state_init_device's launch on one emulated lane: (state, start_ray_vec), both poisoned beforehand."""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    n = len(rvec0)
    st, start = wl.new_state(n, p.nv), np.full((n, p.nv), np.nan)
    rc = (lib or emul_lib()).rays_emul_window_deposition(
        C.byref(p), 0, n, eb.d(rvec0), eb.d(rindex_vec0), *wl._state_args(st), 1, None, 0, None, None, None, None, 0, None,
        None, None, eb.d(start))
    if rc:
        raise RuntimeError(f"rays_emul_window_deposition (state_init) rc={rc}")
    return st, start


def new_works(specs, nray):
    """The accumulators, bin-major as on the device, zeroed once -- when the state is initialised."""
    return [np.zeros((int(nb), nray)) for _, nb in specs]


def window(p: RaysParams, st: dict, n_steps: int, power, specs, works, rho=None, lib=None, waves=None):
    """One deposition window; the state and the works are updated in place.  Returns npoints_win.  waves = (kind,
    blocks, stride): whole emulated waves of the wave library `lib` instead of one lane."""
    n = len(st["s"])
    power = np.ascontiguousarray(power, dtype=np.float64)
    which = (C.c_int * 2)(*[fl.WHICH[w] for w, _ in specs], *([0] * (2 - len(specs))))
    bins = (C.c_int * 2)(*[int(nb) for _, nb in specs], *([0] * (2 - len(specs))))
    grid, fspl = rho if rho is not None else (None, None)
    npw = np.full(n, -7, dtype=np.int32)
    tail = [int(n_steps), eb.d(power), len(specs), which, bins, eb.d(grid), eb.d(fspl), 0 if grid is None else len(grid),
            eb.d(works[0]), eb.d(works[1]) if len(works) > 1 else None, eb.i(npw)]
    if waves is None:
        rc = (lib or emul_lib()).rays_emul_window_deposition(C.byref(p), 1, n, None, None, *wl._state_args(st), *tail, None)
    else:
        kind, blocks, stride = waves
        rc = (lib or emul_lib(wave=True)).rays_emul_window_deposition_waves(
            C.byref(p), sl.WAVE_KINDS[kind], int(blocks), int(stride), n, *wl._state_args(st), *tail)
    if rc:
        raise RuntimeError(f"rays_emul_window_deposition rc={rc}")
    return npw


def profile_sum(work, carry=None):
    """profile(b) = carry(b) + work(b, 1) + work(b, 2) + ... in ray order (rays_deposition.hip: profile_sum_kernel);
    work bin-major."""
    s = np.zeros(work.shape[0]) if carry is None else np.array(carry, dtype=np.float64)
    for r in range(work.shape[1]):
        s = s + work[:, r]
    return s


def run_windowed(p: RaysParams, rvec0, rindex_vec0, power, specs, sizes, rho=None, lib=None, waves=None, wave_lib=None,
                 after_window=None, extra_windows=0, max_windows=100000):
    """A whole run in deposition windows.  sizes: the n_steps values, cycled.  Returns the state's summaries with
    start_ray_vec, `works` (each [nray][n_bins], the reference's layout), `profiles`, `state` and `windows` (their
    number).  after_window(k, state, works_bin_major): called behind every window.  extra_windows: calls made after
    every ray has ended, which have to change no byte and return npoints_win = 0."""
    st, start = state_init(p, rvec0, rindex_vec0, lib=lib)
    n = len(start)
    works = new_works(specs, n)
    have = np.ones(n, dtype=np.int64)
    k = 0
    for k, w in enumerate(itertools.cycle(sizes)):
        assert k < max_windows
        if not (st["stop_code"] == 0).any():
            break
        npw = window(p, st, w, power, specs, works, rho=rho, lib=wave_lib if waves else lib, waves=waves)
        assert (npw >= 0).all() and (npw <= w).all()
        have += npw
        if after_window:
            after_window(k, st, works)
    before = wl.state_bytes(st) + b"".join(w.tobytes() for w in works)
    for _ in range(extra_windows):
        npw = window(p, st, 5, power, specs, works, rho=rho, lib=wave_lib if waves else lib, waves=waves)
        assert not npw.any()
        assert wl.state_bytes(st) + b"".join(w.tobytes() for w in works) == before
    out = wl.state_summaries(st)
    assert np.array_equal(have, out["npoints"])
    out.update(start_ray_vec=start, state=st, windows=k, works=[np.ascontiguousarray(w.T) for w in works],
               profiles=[profile_sum(w) for w in works])
    return out
