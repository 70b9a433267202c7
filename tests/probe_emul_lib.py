"""ctypes wrapper around tests/hip_emul/librays_emul_probe.so: the device right-hand side (rays_device_arith.inc)
compiled for the host and evaluated state by state -- equilibrium with its eq record, deriv_cold, deriv_num, rhs_eval
(eqn_ray + check_save) and rk4_step_as_reference, in the configuration's own shape.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from rays_amd.params import RaysParams
from tests import emul_build as eb
from tests.emul_build import d as _d, i as _i

_LIB = os.path.join(eb.DIR, "librays_emul_probe.so")
_lib = None


def load(path):
    lib = eb.load(path)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.rays_emul_probe.restype = C.c_int
    lib.rays_emul_probe.argtypes = [C.POINTER(RaysParams), C.c_int, dp, dp, dp, dp, dp, dp, ip]
    lib.rays_emul_rk4_step.restype = C.c_int
    lib.rays_emul_rk4_step.argtypes = [C.POINTER(RaysParams), C.c_int, dp, dp, dp, dp, ip]
    return lib


def lib():
    global _lib
    if _lib is None:
        eb.build("emul_probe.cpp", _LIB)
        _lib = load(_LIB)
    return _lib


def mutated_lib(tmp_path, old, new, count=1):
    """The library built from a copy of the sources with one token of rays_device_arith.inc changed."""
    directory = eb.mutated_tree(str(tmp_path / "tree"), "rays_device_arith.inc", old, new, count)
    out = str(tmp_path / "librays_emul_probe_mutated.so")
    eb.build("emul_probe.cpp", out, directory=directory)
    return load(out)


def probe(p: RaysParams, v, tab=None, lib_=None) -> dict:
    """rays_emul_probe at the states v[n][nv]: eq[n][28 + 12 ns] (the other species' ts / gradts are 0: EqPoint keeps the
    electrons'), cold[n][7], num[n][7], dvds[n][nv], resid[n], codes[n][4] as oracle_lib.probe has them."""
    l = lib_ or lib()
    if tab:
        eb.set_axisym_tables(l, tab)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, p.nv)
    n, neq = len(v), 28 + 12 * (p.nspec + 1)
    out = dict(eq=np.zeros((n, neq)), cold=np.zeros((n, 7)), num=np.zeros((n, 7)), dvds=np.zeros((n, p.nv)),
               resid=np.zeros(n), codes=np.zeros((n, 4), dtype=np.int32))
    rc = l.rays_emul_probe(C.byref(p), n, _d(v), _d(out["eq"]), _d(out["cold"]), _d(out["num"]), _d(out["dvds"]),
                           _d(out["resid"]), _i(out["codes"]))
    if rc:
        raise RuntimeError(f"rays_emul_probe rc={rc}")
    return out


def eq_columns(p):
    """the columns of the eq record the device's EqPoint carries: all but ts / gradts of the species after the first"""
    keep = np.ones(28 + 12 * (p.nspec + 1), dtype=bool)
    for s in range(1, p.nspec + 1):
        keep[28 + 12 * s + 4:28 + 12 * s + 8] = False
    return keep


def step(p: RaysParams, v, s=None, tab=None, lib_=None):
    """One step as trace_rays has it, through rk4_step_as_reference and rhs_eval: (v1, resid, codes[n][3]) with codes =
    (stop code of the stage that refused, check_save's flag, check_save's stop_ode); v1 = v after a refused stage."""
    l = lib_ or lib()
    if tab:
        eb.set_axisym_tables(l, tab)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, p.nv)
    s = None if s is None else np.ascontiguousarray(s, dtype=np.float64)
    n = len(v)
    v1, resid, codes = np.zeros((n, p.nv)), np.zeros(n), np.zeros((n, 3), dtype=np.int32)
    rc = l.rays_emul_rk4_step(C.byref(p), n, _d(v), _d(s), _d(v1), _d(resid), _i(codes))
    if rc:
        raise RuntimeError(f"rays_emul_rk4_step rc={rc}")
    return v1, resid, codes
