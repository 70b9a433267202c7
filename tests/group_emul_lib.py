"""ctypes wrapper around tests/hip_emul/librays_emul_group.so: the lane-group SG kernel (rays_sg_group.hpp) compiled
for the host wave emulator (64 lanes per wave as fibers) -- test infrastructure."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from rays_amd.params import RaysParams
from tests import emul_build as eb
from tests.emul_build import d as _d

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(_ROOT, "tests", "hip_emul")
_LIB = os.path.join(_DIR, "librays_emul_group.so")
# second build with only two register rows of phi: ordinary rays then use the workspace rows all the time
_LIB_KR2 = os.path.join(_DIR, "librays_emul_group_kr2.so")
_lib = None
_lib_kr2 = None
_variants = {}


def build(out=None, defs=()):
    eb.build("emul_group.cpp", _LIB if out is None else out, defs)


def _load(path):
    l = eb.load(path)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    l.rays_emul_trace_group.restype = C.c_int
    l.rays_emul_trace_group.argtypes = [C.POINTER(RaysParams), C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, ip, ip, dp, dp, dp]
    l.rays_emul_trace_rk4_waves.restype = C.c_int
    l.rays_emul_trace_sg_waves.restype = C.c_int
    l.rays_emul_trace_sg_waves.argtypes = [C.POINTER(RaysParams), C.c_int, C.c_int, dp, dp, dp, dp, ip, ip, dp, dp, dp]
    l.rays_emul_trace_rk4_waves.argtypes = [C.POINTER(RaysParams), C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, ip, ip, dp, dp, dp]
    return l


def lib_variant(tag: str, defs):
    """The library compiled with extra -D switches (its own .so per tag)."""
    if tag not in _variants:
        path = os.path.join(_DIR, f"librays_emul_group_{tag}.so")
        build(out=path, defs=list(defs))
        _variants[tag] = _load(path)
    return _variants[tag]


def lib(small_tier=False):
    global _lib, _lib_kr2
    if small_tier:
        if _lib_kr2 is None:
            build(out=_LIB_KR2, defs=["-DRAYS_SG_GROUP_KR=2"])
            _lib_kr2 = _load(_LIB_KR2)
        return _lib_kr2
    if _lib is None:
        build()
        _lib = _load(_LIB)
    return _lib


def set_axisym_tables(tab: dict, library=None):
    eb.set_axisym_tables(library or lib(), tab)


def _run(entry, name, p, head, rvec0, rindex_vec0):
    """entry(p, *head, nray, rvec0, rindex_vec0, <the seven output arrays>) into zeroed outputs"""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    out = eb.trace_outputs(len(rvec0), p.nv, p.nstep_max + 1)
    rc = entry(C.byref(p), *head, len(rvec0), _d(rvec0), _d(rindex_vec0), *eb.trace_args(out))
    if rc:
        raise RuntimeError(f"{name} rc={rc}")
    return out


def trace(p: RaysParams, rvec0, rindex_vec0, G: int = 8, resident_blocks: int = 2, small_tier: bool = False) -> dict:
    return _run(lib(small_tier).rays_emul_trace_group, "rays_emul_trace_group", p, [int(G), int(resident_blocks)], rvec0,
                rindex_vec0)


def trace_rk4_waves(p: RaysParams, rvec0, rindex_vec0, nwaves: int = 1, library=None, stride: int = 0,
                    w2_body: bool = False) -> dict:
    """The one-ray-per-lane RK4 kernel on `nwaves` whole 64-lane waves (rays beyond 64 * nwaves are pulled by lanes
    whose ray has ended; stride > 1: in the "long rays first" order of rays_trace.hpp: take_rays; w2_body: the
    body of the two-waves-per-SIMD build -- one loop, index order, residual(:) alone through the LDS window)."""
    library = library or lib()
    library.rays_emul_rk4_waves_use_w2_body(int(w2_body))
    return _run(library.rays_emul_trace_rk4_waves, "rays_emul_trace_rk4_waves", p, [int(nwaves), int(stride)], rvec0,
                rindex_vec0)


def trace_sg_waves(p: RaysParams, rvec0, rindex_vec0, nwaves: int = 1, library=None) -> dict:
    """The one-ray-per-lane Shampine-Gordon kernel on `nwaves` whole 64-lane waves (rays beyond 64 * nwaves are pulled
    by lanes whose ray has ended)."""
    return _run((library or lib()).rays_emul_trace_sg_waves, "rays_emul_trace_sg_waves", p, [int(nwaves)], rvec0,
                rindex_vec0)
