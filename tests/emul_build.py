"""TEST INFRASTRUCTURE ONLY: the one build rule and the one load step of the host emulation libraries
(tests/hip_emul/*.cpp: the product's kernel headers compiled for the host), and the ctypes plumbing their wrappers
share -- emul_lib, group_emul_lib, summary_lib, window_lib and fused_deposition_lib."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from rays_amd.params import AxisymTables, axisym_tables_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hip_emul")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-extern-tls-init", "-fPIC", "-shared", "-w"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"]


def dependencies():
    """Every file an emulation library can read: a wildcard, so that no library's list can fall behind its includes
    (tests/test_cpu_emul_build.py holds it against g++ -MM)."""
    csrc = os.path.join(ROOT, "rays_amd", "csrc")
    return sorted(glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(csrc, "*.inc")) +
                  [os.path.join(ROOT, "include", "rays_hip.h")] +
                  [f for pat in ("*.cpp", "*.hpp", "*.inc", os.path.join("hip", "*.h")) for f in glob.glob(os.path.join(DIR, pat))])


def stale(lib, deps=None):
    """True if `lib` is missing or any dependency is newer than it."""
    if not os.path.exists(lib):
        return True
    built = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > built for d in (dependencies() if deps is None else deps))


def command(src, out, defs=(), sanitize=False, directory=DIR):
    return ["g++", *(SANITIZE if sanitize else []), *FLAGS, *defs, "-I", directory, os.path.join(directory, src), "-o", out]


def build(src, out, defs=(), sanitize=False, directory=DIR):
    """Compiles tests/hip_emul/<src> with the -D switches `defs` into the library `out`, unless it is up to date.
    `directory`: the tests/hip_emul of a copy of the source tree (mutated_tree) -- always built."""
    if directory != DIR or stale(out):
        subprocess.check_call(command(src, out, defs, sanitize, directory))


def mutated_tree(dst, file, old, new, count=1):
    """A copy of everything an emulation library reads (rays_amd/csrc, include, tests/hip_emul) under `dst`, with `old`
    replaced by `new` in rays_amd/csrc/<file>: `old` has to occur exactly `count` times.  Returns the copy's
    tests/hip_emul, for build(..., directory=)."""
    import shutil
    for d in (os.path.join("rays_amd", "csrc"), "include", os.path.join("tests", "hip_emul")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(dst, d),
                        ignore=shutil.ignore_patterns("*.so", "*.o", "build", "*.hip", "__pycache__"))
    path = os.path.join(dst, "rays_amd", "csrc", file)
    text = open(path).read()
    assert text.count(old) == count, f"{file}: {text.count(old)} occurrences of {old!r}, expected {count}"
    open(path, "w").write(text.replace(old, new))
    return os.path.join(dst, "tests", "hip_emul")


def d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def i(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def load(path):
    """The library with its two table setters declared and the Z-function spline table of damp_fund_ECH handed over:
    the data file cut from the reference's initialize_spline_coeffs (rays_amd/data/zfun_spline_re.npz)."""
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    lib.rays_emul_set_zfun_table.restype = C.c_int
    lib.rays_emul_set_zfun_table.argtypes = [dp, C.c_int, C.c_double, C.c_double]
    lib.rays_emul_set_axisym_tables.restype = C.c_int
    lib.rays_emul_set_axisym_tables.argtypes = [C.POINTER(AxisymTables), C.c_int, C.c_double, C.c_double]
    z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
    f = np.ascontiguousarray(z["fspl_re"], dtype=np.float64)
    lib.rays_emul_set_zfun_table(d(f), len(f), float(z["x_min"]), float(z["x_max"]))
    return lib


def set_axisym_tables(lib, tab: dict):
    """Hands the eqdsk / profile tables to an emulation library (each library keeps its own copy)."""
    t, keep = axisym_tables_struct(tab)
    lin = "lin_psi" in tab   # 'eqdsk_magnetics_lin_interp'
    lib.rays_emul_set_axisym_tables(C.byref(t), int(lin), float(tab["lin_dR"]) if lin else 0.0,
                                    float(tab["lin_dZ"]) if lin else 0.0)


def axisym_tables_of(g):
    """The axi_* table dict of a fixture, or None if the fixture carries no table."""
    tab = {k[4:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("axi_")}
    return tab if any(np.size(tab.get(k, ())) for k in ("r_grid", "ne_grid", "te_grid", "ti_grid")) else None


def trace_outputs(nray, nv, npt):
    """The seven arrays of a recorded trace, zeroed."""
    return dict(ray_vec=np.zeros((nray, npt, nv)), residual=np.zeros((nray, npt)),
                npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
                end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray), max_residuals=np.zeros(nray))


def trace_args(out):
    """The seven output pointers in the order every recording entry takes them."""
    return [d(out["ray_vec"]), d(out["residual"]), i(out["npoints"]), i(out["stop_code"]), d(out["end_ray_vec"]),
            d(out["end_residuals"]), d(out["max_residuals"])]


def summary_outputs(n, nv):
    """The six summary arrays, poisoned, not zeroed: every element has to be written by the kernel."""
    return dict(npoints=np.full(n, -7, dtype=np.int32), stop_code=np.full(n, -7, dtype=np.int32),
                start_ray_vec=np.full((n, nv), np.nan), end_ray_vec=np.full((n, nv), np.nan),
                end_residuals=np.full(n, np.nan), max_residuals=np.full(n, np.nan))


_variants = {}


def variant_lib(src, stem, base_defs, wave_def, wave, tag, defs, declare):
    """librays_emul_<stem>[_wave][_<tag>].so of a variant build, built and loaded on first use (extra -D switches get a
    library of their own); declare(lib, wave) sets the argument types of its entries."""
    path = os.path.join(DIR, f"librays_emul_{stem}" + ("_wave" if wave else "") + (f"_{tag}" if tag else "") + ".so")
    if path not in _variants:
        build(src, path, [*base_defs, *([wave_def] if wave else []), *defs])
        _variants[path] = load(path)
        declare(_variants[path], wave)
    return _variants[path]
