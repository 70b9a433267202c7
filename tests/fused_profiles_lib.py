"""TEST INFRASTRUCTURE ONLY: what the two-profile fused deposition tests share -- the fixtures that carry both profiles of
the reference post-processor, and the ctypes wrappers around the host emulation of the two-profile kernels
(tests/hip_emul/emul_fused_profiles.cpp: TraceArgs::ray_vec carries the Dep2TraceArgs block, as in the product's
launches).  The library also holds the single-profile entries of emul_fused_deposition.cpp, so fl.emul_fused(...,
lib=emul_lib()) compares both paths on one set of tables."""
from __future__ import annotations

import ctypes as C

import numpy as np

from rays_amd.params import RaysParams
from tests import emul_build as eb
from tests import fused_deposition_lib as fl
from tests import summary_lib as sl

# the six fixtures with Ptotal_psi AND Ptotal_rho (dep_names, dep_work[2], dep_profile[2], dep_q_sum[2])
TWO_PROFILE_FIXTURES = ["gold_axisym16_eqdsk_zexit_rk4", "gold_axisym64_eqdsk_damp_rk4", "gold_axisym64_eqdsk_damp_sg",
                        "gold_axisym64_eqdsk129_tspline_damp_rk4", "gold_axisym64_eqdsk129_tspline_damp_sg",
                        "gold_axisym64_eqdsk_tspline_rk4_num"]
ORDERS = [("Ptotal_psi", "Ptotal_rho"), ("Ptotal_rho", "Ptotal_psi")]
BASE_DEFS = ["-DRAYS_RK4_NO_HANDOVER"]
WAVE_DEF = "-DRAYS_EMUL_DEPOSIT_WAVE=1"


def declare(lib, wave):
    fl._declare(lib, wave)
    dp, ip, pp, cp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(RaysParams), C.POINTER(C.c_int)
    tail = [dp, cp, cp, dp, dp, C.c_int, ip, ip, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp]
    if wave:
        lib.rays_emul_fused_profiles_waves.restype = C.c_int
        lib.rays_emul_fused_profiles_waves.argtypes = [pp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp] + tail
    else:
        lib.rays_emul_fused_profiles.restype = C.c_int
        lib.rays_emul_fused_profiles.argtypes = [pp, C.c_int, dp, dp] + tail


def emul_lib(wave: bool = False):
    """librays_emul_profiles[_wave].so, built on first use."""
    return eb.variant_lib("emul_fused_profiles.cpp", "profiles", BASE_DEFS, WAVE_DEF, wave, "", (), declare)


def _prepare(p, rvec0, rindex_vec0, power, specs, rho, profile_in):
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    power = np.ascontiguousarray(power, dtype=np.float64)
    (wa, na), (wb, nb) = specs
    n = len(rvec0)
    out = eb.summary_outputs(n, p.nv)   # poisoned: every element has to be written by the kernel
    works = [np.full((na, n), np.nan), np.full((nb, n), np.nan)]   # bin-major, as on the device (zeroed by the launch)
    profs = [np.full(na, np.nan), np.full(nb, np.nan)]
    pin = [None if c is None else np.ascontiguousarray(c, dtype=np.float64) for c in (profile_in or (None, None))]
    which = (C.c_int * 2)(fl.WHICH[wa], fl.WHICH[wb])
    bins = (C.c_int * 2)(int(na), int(nb))
    grid, fspl = rho if rho is not None else (None, None)
    d, i = eb.d, eb.i
    tail = [d(power), which, bins, d(grid), d(fspl), 0 if grid is None else len(grid), i(out["npoints"]),
            i(out["stop_code"]), d(out["start_ray_vec"]), d(out["end_ray_vec"]), d(out["end_residuals"]),
            d(out["max_residuals"]), d(works[0]), d(works[1]), d(pin[0]), d(pin[1]), d(profs[0]), d(profs[1])]
    return rvec0, rindex_vec0, out, works, profs, tail


def _finish(out, works, profs):
    out["works"] = [np.ascontiguousarray(w.T) for w in works]   # the reference's layout [nray][n_bins]
    out["profiles"] = profs
    return out


def emul_profiles(p: RaysParams, rvec0, rindex_vec0, power, specs, rho=None, profile_in=None, lib=None):
    """The two-profile kernel of p's shape on one emulated lane.  specs = [(which, n_bins), (which, n_bins)]; out: the
    summaries, `works` (each [nray][n_bins]) and `profiles`, in the order asked."""
    rvec0, rindex_vec0, out, works, profs, tail = _prepare(p, rvec0, rindex_vec0, power, specs, rho, profile_in)
    rc = (lib or emul_lib()).rays_emul_fused_profiles(C.byref(p), len(rvec0), eb.d(rvec0), eb.d(rindex_vec0), *tail)
    if rc:
        raise RuntimeError(f"rays_emul_fused_profiles rc={rc}")
    return _finish(out, works, profs)


def emul_profiles_waves(p: RaysParams, rvec0, rindex_vec0, power, specs, kind: str, blocks: int = 1, stride: int = 0,
                        rho=None, lib=None):
    """The two-profile kernel on whole emulated waves (kind "rk4" | "sg")."""
    rvec0, rindex_vec0, out, works, profs, tail = _prepare(p, rvec0, rindex_vec0, power, specs, rho, None)
    rc = (lib or emul_lib(wave=True)).rays_emul_fused_profiles_waves(
        C.byref(p), sl.WAVE_KINDS[kind], int(blocks), int(stride), len(rvec0), eb.d(rvec0), eb.d(rindex_vec0), *tail)
    if rc:
        raise RuntimeError(f"rays_emul_fused_profiles_waves rc={rc}")
    return _finish(out, works, profs)


def assert_same_as_single(out, singles, what=""):
    """A two-profile result against the two single-profile results of the same rays (fl.emul_fused / ..._waves)."""
    for i, ref in enumerate(singles):
        sl.assert_same(out, ref, f"{what} summaries vs single pass {i}")
        np.testing.assert_array_equal(out["works"][i], ref["work"], err_msg=f"{what}: work {i}")
        np.testing.assert_array_equal(out["profiles"][i], ref["profile"], err_msg=f"{what}: profile {i}")
