"""TEST INFRASTRUCTURE ONLY: what the summary-only trace tests share -- the expected per-ray summaries cut from a
fixture or from a full trace, and the ctypes wrappers around the host emulation of the summary-only kernels
(tests/hip_emul/emul_summary.cpp: TraceArgs::ray_vec and ::residual are null there)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from rays_amd.params import RaysParams
from tests import emul_build as eb
from tests.common import stop_codes
from tests.emul_build import d as _d, i as _i, summary_outputs as _outputs

KEYS = ("npoints", "stop_code", "start_ray_vec", "end_ray_vec", "end_residuals", "max_residuals")
_NO_STEP = -1.7976931348623157e308   # maxval of an empty array: a ray that started and recorded no step


def summaries_of(full: dict) -> dict:
    """The summaries a full trace carries: its per-ray arrays and point 1 of every trajectory (ray_tracing.f90:259)."""
    out = {k: np.asarray(full[k]) for k in KEYS if k != "start_ray_vec"}
    out["start_ray_vec"] = np.ascontiguousarray(np.asarray(full["ray_vec"])[:, 0, :])
    return out


def golden_summaries(g) -> dict:
    """The reference's per-ray summaries from a fixture's recorded arrays (ray_tracing.f90:252-260): end_residuals =
    residual(nstep), max_residuals = maxval(abs(residual(1:nstep))) with nstep = npoints - 1 recorded steps.  A ray the
    initial check_save refused (npoints = 1, end_ray_vec all zero) keeps the zeros of initialize_ray_results_m."""
    n = g["npoints"].astype(np.int64)
    res = g["residual"]
    end_res, max_res = np.zeros(len(n)), np.zeros(len(n))
    for r, k in enumerate(n):
        if k >= 2:
            end_res[r] = res[r, k - 2]
            max_res[r] = np.abs(res[r, :k - 1]).max()
        elif g["end_ray_vec"][r].any():
            max_res[r] = _NO_STEP
    return dict(npoints=g["npoints"], stop_code=stop_codes(g["stop_flag"]),
                start_ray_vec=np.ascontiguousarray(g["ray_vec"][:, 0, :]), end_ray_vec=g["end_ray_vec"],
                end_residuals=end_res, max_residuals=max_res)


def assert_same(out: dict, ref: dict, what: str = ""):
    for k in KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"{what}: {k}")


# ---- host emulation of the summary-only kernels ----------------------------------------------------------------------
def _declare(lib, wave):
    dp, ip, pp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(RaysParams)
    if wave:
        lib.rays_emul_summary_waves.restype = C.c_int
        lib.rays_emul_summary_waves.argtypes = [pp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, ip, dp, dp, dp, dp]
    else:
        lib.rays_emul_summary_trace.restype = C.c_int
        lib.rays_emul_summary_trace.argtypes = [pp, C.c_int, dp, dp, ip, ip, dp, dp, dp, dp, dp, C.c_int]


def emul_lib(wave: bool = False, tag: str = "", defs=()):
    """librays_emul_summary[_wave][_<tag>].so, built on first use (extra -D switches get a library of their own)."""
    return eb.variant_lib("emul_summary.cpp", "summary", ["-DRAYS_RK4_NO_HANDOVER"], "-DRAYS_EMUL_SUMMARY_WAVE=1", wave,
                          tag, defs, _declare)


def set_axisym_tables(g, lib):
    """Hands a fixture's eqdsk / profile tables (if it has any) to an emulation library."""
    tab = eb.axisym_tables_of(g)
    if tab is not None:
        eb.set_axisym_tables(lib, tab)


def emul_trace(p: RaysParams, rvec0, rindex_vec0, ds_values=None, lib=None) -> dict:
    """The summary-only kernel of p's shape on one emulated lane; ds_values: the fused scan's launch (arrays with a
    leading run dimension)."""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    ds = None if ds_values is None else np.ascontiguousarray(ds_values, dtype=np.float64)
    nray, runs = len(rvec0), 1 if ds is None else len(ds)
    out = _outputs(runs * nray, p.nv)
    rc = (lib or emul_lib()).rays_emul_summary_trace(
        C.byref(p), runs * nray, _d(rvec0), _d(rindex_vec0), _i(out["npoints"]), _i(out["stop_code"]),
        _d(out["start_ray_vec"]), _d(out["end_ray_vec"]), _d(out["end_residuals"]), _d(out["max_residuals"]), _d(ds),
        0 if ds is None else nray)
    if rc:
        raise RuntimeError(f"rays_emul_summary_trace rc={rc}")
    if ds is not None:
        out = {k: v.reshape((runs, nray) + v.shape[1:]) for k, v in out.items()}
    return out


WAVE_KINDS = {"rk4": 0, "rk4_w2": 1, "sg": 2, "sg_group": 3}


def emul_waves(p: RaysParams, rvec0, rindex_vec0, kind: str, blocks: int = 1, stride_or_G: int = 0, lib=None) -> dict:
    """The summary-only kernel on whole emulated waves (emul_summary.cpp: rays_emul_summary_waves)."""
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    out = _outputs(len(rvec0), p.nv)
    rc = (lib or emul_lib(wave=True)).rays_emul_summary_waves(
        C.byref(p), WAVE_KINDS[kind], int(blocks), int(stride_or_G), len(rvec0), _d(rvec0), _d(rindex_vec0),
        _i(out["npoints"]), _i(out["stop_code"]), _d(out["start_ray_vec"]), _d(out["end_ray_vec"]),
        _d(out["end_residuals"]), _d(out["max_residuals"]))
    if rc:
        raise RuntimeError(f"rays_emul_summary_waves rc={rc}")
    return out
