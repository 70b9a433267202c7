"""ctypes binding of the C ABI in include/rays_hip.h (librays_hip.so).

This is the only compute path of the package: if the HIP library is missing or no GPU is
visible the calls raise -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .params import AxisymTables, RaysFan, RaysParams, axisym_tables_struct


class DeviceResult(C.Structure):
    """rays_device_result_t (include/rays_hip.h)"""
    _fields_ = [("device", C.c_int32), ("nray", C.c_int32), ("ray_vec", C.c_void_p), ("residual", C.c_void_p),
                ("npoints", C.c_void_p), ("stop_code", C.c_void_p), ("end_ray_vec", C.c_void_p),
                ("end_residuals", C.c_void_p), ("max_residuals", C.c_void_p)]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAYS_HIP_LIB") or os.path.join(_HERE, "lib", "librays_hip.so")

# every symbol include/rays_hip.h declares
EXPORTED_SYMBOLS = (
    "rays_hip_init", "rays_hip_init_devices", "rays_hip_finalize", "rays_hip_device_count", "rays_hip_sizeof_params",
    "rays_hip_last_error", "rays_hip_set_zfun_table", "rays_hip_set_axisym_tables", "rays_hip_set_eqdsk_lin_tables",
    "rays_hip_stop_flag_text", "rays_hip_check_params", "rays_hip_trace", "rays_hip_trace_gather", "rays_hip_result_to_host", "rays_hip_trace_device", "rays_hip_scan_device", "rays_hip_ode_step_device",
    "rays_hip_kernel_name", "rays_hip_kernel_name_for", "rays_hip_probe", "rays_hip_pack_device", "rays_hip_unpack_device",
    "rays_hip_sizeof_fan", "rays_hip_ray_init", "rays_hip_ray_init_device",
    "rays_hip_set_rho_table", "rays_hip_deposition_device", "rays_hip_deposition",
    "rays_hip_keep_last_result", "rays_hip_deposition_last",
    "rays_hip_set_numerics", "rays_hip_get_numerics",
    "rays_hip_ray_diagnostics_device", "rays_hip_ray_diagnostics",
    "rays_hip_point_offsets_device", "rays_hip_ray_diagnostics_packed_device",
    "rays_hip_trace_summary_device", "rays_hip_scan_summary_device", "rays_hip_trace_summary",
    "rays_hip_summary_kernel_name_for",
    "rays_hip_trace_deposition_device", "rays_hip_trace_deposition", "rays_hip_deposition_kernel_name_for",
    "rays_hip_trace_profiles_device", "rays_hip_trace_profiles", "rays_hip_profiles_kernel_name_for",
    "rays_hip_deposition_profile_set",
    "rays_hip_rk4_loop_for",
    "rays_hip_state_init_device", "rays_hip_trace_window_device", "rays_hip_state_summary_device",
    "rays_hip_window_kernel_name_for", "rays_hip_trace_windowed",
    "rays_hip_trace_window_profiles_device", "rays_hip_window_profiles_kernel_name_for",
    "rays_hip_profile_sum_segments_device", "rays_hip_scan_profiles_device", "rays_hip_trace_profiles_segments_device",
    "rays_hip_ox_conv_device", "rays_hip_ox_conv", "rays_hip_ox_conv_kernel_name_for",
)

_lib = None


class RaysHipError(RuntimeError):
    pass


class RayStateStruct(C.Structure):
    """rays_ray_state_t (include/rays_hip.h): device pointers of the saved ray state of windowed tracing"""
    _fields_ = [("v", C.c_void_p), ("s", C.c_void_p), ("nstep", C.c_void_p), ("stop_code", C.c_void_p),
                ("resid", C.c_void_p), ("sg_err", C.c_void_p), ("flags", C.c_void_p)]


STATE_REFUSED = 1   # RAYS_STATE_REFUSED


class DepProfileStruct(C.Structure):
    """rays_dep_profile_t (include/rays_hip.h): one record of rays_hip_trace_profiles[_device]"""
    _fields_ = [("which", C.c_int), ("n_bins", C.c_int), ("work", C.c_void_p), ("profile_in", C.c_void_p),
                ("profile", C.c_void_p)]


DEP_MAX_PROFILES = 2   # RAYS_DEP_MAX_PROFILES


# rays_ox_result_t (include/rays_hip.h), in the struct's order: (field, numpy dtype, values per ray)
OX_FIELDS = (("status", np.int32, 1), ("step_number", np.int32, 1), ("iterations", np.int32, 1), ("alpha_max", np.float64, 1),
             ("x_max", np.float64, 3), ("k_max", np.float64, 3), ("x_cut", np.float64, 3), ("conv_coeff", np.float64, 1),
             ("nvecx_c", np.float64, 3), ("nvecy_c", np.float64, 3), ("nvecz_c", np.float64, 3), ("aux", np.float64, 5))
OX_AUX = ("cos_theta", "gamma", "L", "ny_c", "nz_c")             # RAYS_OX_AUX_*
OX_FOUND_MAX, OX_FOUND_CUTOFF, OX_CONVERTED, OX_EQ_REFUSED = 1, 2, 4, 8   # RAYS_OX_*
OX_CONVERSION_THRESHOLD = float(np.float32(0.0001))              # OX_conv_analysis_m.f90:32: a default-real literal


class OxResultStruct(C.Structure):
    """rays_ox_result_t (include/rays_hip.h): one pointer per field, null = not wanted"""
    _fields_ = [(name, C.c_void_p) for name, _, _ in OX_FIELDS]


def load():
    """Load librays_hip.so (built by `make -C rays_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch bundles its own HIP runtime (libamdhip64.so.7, the SONAME of the system's too).  Whichever is loaded
    # first serves the whole process; loaded in the other order -- this library (and with it /opt/rocm's runtime)
    # first, torch afterwards -- the second runtime to initialise finds "no ROCm-capable device".  The Python host
    # uses torch for device memory and streams (DeviceTrace, ode_step, bench.py), so torch goes first, always.
    # A host that needs the C ABI alone (no DeviceTrace / ode_step / bench) sets RAYS_AMD_NO_TORCH=1 and saves the import.
    if "torch" in __import__("sys").modules or not os.environ.get("RAYS_AMD_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise RaysHipError(
            f"{LIB_PATH} not found: build it with `make -C rays_amd/csrc` (needs hipcc, gfx950). "
            "rays_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    pp = C.POINTER(RaysParams)
    lib.rays_hip_init.restype = C.c_int
    lib.rays_hip_init.argtypes = [C.c_int]
    lib.rays_hip_init_devices.restype = C.c_int
    lib.rays_hip_init_devices.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.rays_hip_finalize.restype = C.c_int
    lib.rays_hip_device_count.restype = C.c_int
    lib.rays_hip_sizeof_params.restype = C.c_int
    if lib.rays_hip_sizeof_params() != C.sizeof(RaysParams):
        raise RaysHipError("rays_params_t layout mismatch between librays_hip.so and rays_amd.params")
    lib.rays_hip_last_error.restype = C.c_int
    lib.rays_hip_last_error.argtypes = [C.c_char_p, C.c_int]
    lib.rays_hip_stop_flag_text.restype = C.c_char_p
    lib.rays_hip_stop_flag_text.argtypes = [C.c_int]
    lib.rays_hip_set_zfun_table.restype = C.c_int
    lib.rays_hip_set_zfun_table.argtypes = [dp, C.c_int, C.c_double, C.c_double]
    lib.rays_hip_set_axisym_tables.restype = C.c_int
    lib.rays_hip_set_axisym_tables.argtypes = [C.POINTER(AxisymTables)]
    lib.rays_hip_set_eqdsk_lin_tables.restype = C.c_int
    lib.rays_hip_set_eqdsk_lin_tables.argtypes = [C.POINTER(AxisymTables), C.c_double, C.c_double]
    lib.rays_hip_check_params.restype = C.c_int
    lib.rays_hip_check_params.argtypes = [pp]
    lib.rays_hip_kernel_name.restype = C.c_char_p
    lib.rays_hip_kernel_name.argtypes = [pp]
    lib.rays_hip_kernel_name_for.restype = C.c_char_p
    lib.rays_hip_kernel_name_for.argtypes = [pp, C.c_int]
    lib.rays_hip_trace.restype = C.c_int
    lib.rays_hip_trace.argtypes = [pp, C.c_int, dp, dp, dp, dp, ip, ip, dp, dp, dp, dp]
    lib.rays_hip_trace_gather.restype = C.c_int
    lib.rays_hip_trace_gather.argtypes = [pp, C.c_int, dp, dp, C.POINTER(DeviceResult)]
    lib.rays_hip_result_to_host.restype = C.c_int
    lib.rays_hip_result_to_host.argtypes = [pp, C.POINTER(DeviceResult), dp, dp, ip, ip, dp, dp, dp]
    lib.rays_hip_trace_device.restype = C.c_int
    lib.rays_hip_trace_device.argtypes = [pp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.rays_hip_scan_device.restype = C.c_int
    lib.rays_hip_scan_device.argtypes = [pp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    # (a library given through RAYS_HIP_LIB may predate the summary-only entries -- tools/summary_trace_bench.py times
    # the parent commit's library next to this one; calling them there raises)
    if hasattr(lib, "rays_hip_trace_summary_device"):
        lib.rays_hip_trace_summary_device.restype = C.c_int
        lib.rays_hip_trace_summary_device.argtypes = [pp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.rays_hip_scan_summary_device.restype = C.c_int
        lib.rays_hip_scan_summary_device.argtypes = [pp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.rays_hip_trace_summary.restype = C.c_int
        lib.rays_hip_trace_summary.argtypes = [pp, C.c_int, dp, dp, ip, ip, dp, dp, dp, dp, dp]
        lib.rays_hip_summary_kernel_name_for.restype = C.c_char_p
        lib.rays_hip_summary_kernel_name_for.argtypes = [pp, C.c_int]
    # (likewise the fused trace + deposition entries -- tools/fused_deposition_bench.py)
    if hasattr(lib, "rays_hip_trace_deposition_device"):
        lib.rays_hip_trace_deposition_device.restype = C.c_int
        lib.rays_hip_trace_deposition_device.argtypes = [pp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp,
                                                         vp, vp, vp, vp]
        lib.rays_hip_trace_deposition.restype = C.c_int
        lib.rays_hip_trace_deposition.argtypes = [pp, C.c_int, dp, dp, dp, C.c_int, C.c_int, ip, ip, dp, dp, dp, dp, dp, dp,
                                                  dp]
        lib.rays_hip_deposition_kernel_name_for.restype = C.c_char_p
        lib.rays_hip_deposition_kernel_name_for.argtypes = [pp, C.c_int]
    # (likewise the several-profiles entries -- tools/fused_profiles_bench.py)
    if hasattr(lib, "rays_hip_trace_profiles_device"):
        rp = C.POINTER(DepProfileStruct)
        lib.rays_hip_trace_profiles_device.restype = C.c_int
        lib.rays_hip_trace_profiles_device.argtypes = [pp, C.c_int, vp, vp, vp, C.c_int, rp, vp, vp, vp, vp, vp, vp, vp]
        lib.rays_hip_trace_profiles.restype = C.c_int
        lib.rays_hip_trace_profiles.argtypes = [pp, C.c_int, dp, dp, dp, C.c_int, rp, ip, ip, dp, dp, dp, dp, dp]
        lib.rays_hip_profiles_kernel_name_for.restype = C.c_char_p
        lib.rays_hip_profiles_kernel_name_for.argtypes = [pp, C.c_int, C.c_int]
        lib.rays_hip_deposition_profile_set.restype = C.c_int
        lib.rays_hip_deposition_profile_set.argtypes = [pp, C.POINTER(C.c_int)]
    # (likewise the step-loop query -- an A/B run times the parent commit's library next to this one)
    if hasattr(lib, "rays_hip_rk4_loop_for"):
        lib.rays_hip_rk4_loop_for.restype = C.c_int
        lib.rays_hip_rk4_loop_for.argtypes = [pp, C.c_int]
    # (likewise the windowed-tracing entries -- tools/window_trace_bench.py)
    if hasattr(lib, "rays_hip_trace_window_device"):
        sp = C.POINTER(RayStateStruct)
        lib.rays_hip_state_init_device.restype = C.c_int
        lib.rays_hip_state_init_device.argtypes = [pp, C.c_int, vp, vp, sp, vp, vp]
        lib.rays_hip_trace_window_device.restype = C.c_int
        lib.rays_hip_trace_window_device.argtypes = [pp, C.c_int, sp, C.c_int, vp, vp, vp, vp]
        lib.rays_hip_state_summary_device.restype = C.c_int
        lib.rays_hip_state_summary_device.argtypes = [pp, C.c_int, sp, vp, vp, vp, vp, vp, vp]
        lib.rays_hip_window_kernel_name_for.restype = C.c_char_p
        lib.rays_hip_window_kernel_name_for.argtypes = [pp, C.c_int, C.c_int]
        lib.rays_hip_trace_windowed.restype = C.c_int
        lib.rays_hip_trace_windowed.argtypes = [pp, C.c_int, dp, dp, C.c_int, dp, dp, ip, ip, dp, dp, dp, dp]
    # (likewise the deposition windows -- tools/window_deposition_bench.py)
    if hasattr(lib, "rays_hip_trace_window_profiles_device"):
        lib.rays_hip_trace_window_profiles_device.restype = C.c_int
        lib.rays_hip_trace_window_profiles_device.argtypes = [pp, C.c_int, C.POINTER(RayStateStruct), C.c_int, vp, C.c_int,
                                                              C.POINTER(DepProfileStruct), vp, vp]
        lib.rays_hip_window_profiles_kernel_name_for.restype = C.c_char_p
        lib.rays_hip_window_profiles_kernel_name_for.argtypes = [pp, C.c_int, C.c_int]
    # (likewise the segmented deposition entries -- tools/scan_profiles_bench.py)
    if hasattr(lib, "rays_hip_scan_profiles_device"):
        rp = C.POINTER(DepProfileStruct)
        lib.rays_hip_profile_sum_segments_device.restype = C.c_int
        lib.rays_hip_profile_sum_segments_device.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
        lib.rays_hip_scan_profiles_device.restype = C.c_int
        lib.rays_hip_scan_profiles_device.argtypes = [pp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, rp, vp, vp, vp, vp, vp,
                                                      vp, vp]
        lib.rays_hip_trace_profiles_segments_device.restype = C.c_int
        lib.rays_hip_trace_profiles_segments_device.argtypes = [pp, C.c_int, vp, vp, vp, C.c_int, rp, C.c_int, vp, C.c_int,
                                                                vp, vp, vp, vp, vp, vp, vp]
    lib.rays_hip_ode_step_device.restype = C.c_int
    lib.rays_hip_ode_step_device.argtypes = [pp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.rays_hip_pack_device.restype = C.c_int
    lib.rays_hip_pack_device.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.rays_hip_unpack_device.restype = C.c_int
    lib.rays_hip_unpack_device.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.rays_hip_probe.restype = C.c_int
    lib.rays_hip_probe.argtypes = [pp, C.c_int, dp, dp, dp, dp, dp, ip]
    lib.rays_hip_sizeof_fan.restype = C.c_int
    if lib.rays_hip_sizeof_fan() != C.sizeof(RaysFan):
        raise RaysHipError("rays_fan_t layout mismatch between librays_hip.so and rays_amd.params")
    fp = C.POINTER(RaysFan)
    lib.rays_hip_ray_init.restype = C.c_int
    lib.rays_hip_ray_init.argtypes = [pp, fp, C.c_int, dp, dp, dp, ip]
    lib.rays_hip_ray_init_device.restype = C.c_int
    lib.rays_hip_ray_init_device.argtypes = [pp, fp, C.c_int, vp, vp, ip, vp]
    lib.rays_hip_set_rho_table.restype = C.c_int
    lib.rays_hip_set_rho_table.argtypes = [dp, dp, C.c_int]
    lib.rays_hip_deposition.restype = C.c_int
    lib.rays_hip_deposition.argtypes = [pp, C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, dp]
    lib.rays_hip_deposition_device.restype = C.c_int
    lib.rays_hip_deposition_device.argtypes = [pp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.rays_hip_keep_last_result.restype = C.c_int
    lib.rays_hip_keep_last_result.argtypes = [C.c_int]
    lib.rays_hip_deposition_last.restype = C.c_int
    lib.rays_hip_deposition_last.argtypes = [pp, C.c_int, C.c_int, C.c_int, dp, dp, dp]
    lib.rays_hip_set_numerics.restype = C.c_int
    lib.rays_hip_set_numerics.argtypes = [C.c_int]
    lib.rays_hip_get_numerics.restype = C.c_int
    # (defined in a translation unit of their own, rays_diag.hip: a library given through RAYS_HIP_LIB that is built
    # from rays_capi.hip alone -- the CPU tier's emulated C ABI -- does not have them; calling them there raises)
    if hasattr(lib, "rays_hip_ray_diagnostics_device"):
        lib.rays_hip_ray_diagnostics_device.restype = C.c_int
        lib.rays_hip_ray_diagnostics_device.argtypes = [pp, C.c_int, vp, vp, vp, C.c_uint32, vp, vp, vp]
        lib.rays_hip_ray_diagnostics.restype = C.c_int
        lib.rays_hip_ray_diagnostics.argtypes = [pp, C.c_int, dp, dp, ip, C.c_uint32, dp, ip]
        lib.rays_hip_point_offsets_device.restype = C.c_int
        lib.rays_hip_point_offsets_device.argtypes = [C.c_int, C.c_int, vp, vp, vp]
        lib.rays_hip_ray_diagnostics_packed_device.restype = C.c_int
        lib.rays_hip_ray_diagnostics_packed_device.argtypes = [pp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int64, C.c_uint32,
                                                               vp, vp, vp]
    # (likewise rays_oxconv.hip)
    if hasattr(lib, "rays_hip_ox_conv_device"):
        lib.rays_hip_ox_conv_device.restype = C.c_int
        lib.rays_hip_ox_conv_device.argtypes = [pp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(OxResultStruct), vp]
        lib.rays_hip_ox_conv.restype = C.c_int
        lib.rays_hip_ox_conv.argtypes = [pp, C.c_int, dp, ip, C.POINTER(OxResultStruct), ip, ip]
        lib.rays_hip_ox_conv_kernel_name_for.restype = C.c_char_p
        lib.rays_hip_ox_conv_kernel_name_for.argtypes = [pp]
    _lib = lib
    return lib


def last_error() -> str:
    buf = C.create_string_buffer(1024)
    load().rays_hip_last_error(buf, 1024)
    return buf.value.decode(errors="replace")


def _check(rc: int, what: str):
    if rc != 0:
        raise RaysHipError(f"{what} failed (rc={rc}): {last_error()}")


NUMERICS = {"exact": 0, "tolerance": 1}


def set_numerics(mode: str) -> str:
    """rays_hip_set_numerics: "exact" (bit-identical to the reference CPU path; default) or "tolerance" (not
    bit-identical: every step within 1e-10 relative of the reference's -- 4e-15 measured on the headline fan --, exact
    ray counts / step indices / stop flags; cold RK4 kernels; include/rays_hip.h).  Returns the previous setting."""
    prev = load().rays_hip_set_numerics(NUMERICS[mode])
    if prev < 0:
        raise RaysHipError("rays_hip_set_numerics: " + last_error())
    return "tolerance" if prev == 1 else "exact"


def get_numerics() -> str:
    return "tolerance" if load().rays_hip_get_numerics() == 1 else "exact"


def stop_flag_text(code: int) -> str:
    return load().rays_hip_stop_flag_text(int(code)).decode()


_ZFUN_PATH = os.path.join(_HERE, "data", "zfun_spline_re.npz")
_zfun_set = False


def set_zfun_table(fspl_re=None, x_min=None, x_max=None):
    """Hand the Z-function spline table (fsplRe[nx][4]) to the library.  Default: the table shipped
    in rays_amd/data (cut from the reference's initialize_spline_coeffs, zfunctions_m.f90:436-466)."""
    global _zfun_set
    if fspl_re is None:
        z = np.load(_ZFUN_PATH)
        fspl_re, x_min, x_max = z["fspl_re"], float(z["x_min"]), float(z["x_max"])
    fspl_re = np.ascontiguousarray(fspl_re, dtype=np.float64)
    _check(load().rays_hip_set_zfun_table(_dp(fspl_re), len(fspl_re), float(x_min), float(x_max)),
           "rays_hip_set_zfun_table")
    _zfun_set = True


def set_axisym_tables(tab: dict):
    """Hand the host-built spline tables of an eqdsk equilibrium to the library (copied)."""
    t, keep = axisym_tables_struct(tab)
    if "lin_psi" in tab:   # magnetics_model = 'eqdsk_magnetics_lin_interp'
        _check(load().rays_hip_set_eqdsk_lin_tables(C.byref(t), float(tab["lin_dR"]), float(tab["lin_dZ"])),
               "rays_hip_set_eqdsk_lin_tables")
        return
    _check(load().rays_hip_set_axisym_tables(C.byref(t)), "rays_hip_set_axisym_tables")


def ensure_tables(p: RaysParams):
    if p.damping_model and not _zfun_set:
        set_zfun_table()


def check_params(p: RaysParams):
    _check(load().rays_hip_check_params(C.byref(p)), "rays_hip_check_params")


def kernel_name(p: RaysParams, nray: int = 0) -> str:
    """Kernel specialisation a trace of `nray` rays would launch (0: the default build)."""
    lib = load()
    name = (lib.rays_hip_kernel_name_for(C.byref(p), int(nray)) if nray else lib.rays_hip_kernel_name(C.byref(p))).decode()
    if not name:   # refused parameters or a shape the library was not built with (make FULL=1): never a silent ""
        check_params(p)
        raise RaysHipError("rays_hip_kernel_name: no kernel for this configuration")
    return name


def rk4_loop(p: RaysParams, nray: int = 0) -> str:
    """Which of its step loops the RK4 kernel `kernel_name(p, nray)` runs for p: "lean" (the loop compiled for runs whose
    Solovev density model is not 'constant', whose species have no parabolic temperature profile and whose ray_param is
    not 'arcl') or "general".  The kernel's name is the same for both.  RAYS_HIP_RK4_LOOP=general in the environment
    (read by the library at every launch) forces the general loop."""
    which = load().rays_hip_rk4_loop_for(C.byref(p), int(nray))
    if which < 0:
        check_params(p)
        raise RaysHipError("rays_hip_rk4_loop_for: not an RK4 configuration")
    return "lean" if which else "general"


def summary_kernel_name(p: RaysParams, nray: int = 0) -> str:
    """Kernel specialisation a summary-only trace of `nray` rays would launch (always an exact kernel)."""
    name = load().rays_hip_summary_kernel_name_for(C.byref(p), int(nray)).decode()
    if not name:
        check_params(p)
        raise RaysHipError("rays_hip_summary_kernel_name_for: no summary-only kernel for this configuration")
    return name


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def ray_init_host(p: RaysParams, fan: RaysFan, nray_max: int):
    """rays_hip_ray_init: the launch fan built on the GPU, returned as host arrays
    (rvec0[nray][3], rindex_vec0[nray][3], ray_pwr_wt[nray]) -- the ray_init_m contract."""
    n = int(nray_max)
    rvec0, rindex_vec0, w = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    nray = C.c_int32(0)
    _check(load().rays_hip_ray_init(C.byref(p), C.byref(fan), n, _dp(rvec0), _dp(rindex_vec0), _dp(w),
                                    C.byref(nray)), "rays_hip_ray_init")
    k = nray.value
    return rvec0[:k].copy(), rindex_vec0[:k].copy(), w[:k].copy()


def ray_init_device(p: RaysParams, fan: RaysFan, nray_max: int, d_rvec0: int, d_rindex_vec0: int,
                    stream: int = 0) -> int:
    """rays_hip_ray_init_device: fills the device arrays (nray_max x 3 doubles each), returns nray."""
    nray = C.c_int32(0)
    _check(load().rays_hip_ray_init_device(C.byref(p), C.byref(fan), int(nray_max), d_rvec0, d_rindex_vec0,
                                           C.byref(nray), stream), "rays_hip_ray_init_device")
    return nray.value


DEP_PROFILES = {"Ptotal_psi": 0, "Ptotal_rho": 1, "Ptotal_x": 2}


def set_rho_table(grid, fspl):
    """rho(psiN) spline of the eqdsk equilibrium (needed for the Ptotal_rho deposition profile)."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    fspl = np.ascontiguousarray(fspl, dtype=np.float64)
    _check(load().rays_hip_set_rho_table(_dp(grid), _dp(fspl), len(grid)), "rays_hip_set_rho_table")


def deposition_device(p: RaysParams, which: str, n_bins: int, nray: int, d_ray_vec: int, d_npoints: int,
                      d_power: int, d_work: int, d_profile_in, d_profile_out: int, stream: int = 0):
    """rays_hip_deposition_device on device pointers (torch `.data_ptr()`s); d_profile_in may be None."""
    _check(load().rays_hip_deposition_device(C.byref(p), DEP_PROFILES[which], int(n_bins), int(nray), d_ray_vec,
                                             d_npoints, d_power, d_work, d_profile_in, d_profile_out, stream),
           "rays_hip_deposition_device")


def init_devices(device_ids):
    """rays_hip_init_devices: explicit slot -> device list for trace_host (repeats allowed)."""
    ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
    if load().rays_hip_init_devices(len(device_ids), ids) < 0:
        raise RaysHipError("rays_hip_init_devices: " + last_error())


def finalize():
    """rays_hip_finalize: everything the library holds on the devices and in pinned memory goes back to the driver.
    The tables and settings stay; the next call initialises again as the first one did."""
    _check(load().rays_hip_finalize(), "rays_hip_finalize")


def deposition_host(p: RaysParams, which: str, n_bins: int, ray_vec, npoints, initial_ray_power):
    """rays_hip_deposition: host arrays in (the ray_results_m image), (work[nray][n_bins], profile[n_bins]) out."""
    ray_vec = np.ascontiguousarray(ray_vec, dtype=np.float64)
    npoints = np.ascontiguousarray(npoints, dtype=np.int32)
    power = np.ascontiguousarray(initial_ray_power, dtype=np.float64)
    nray = len(npoints)
    work, prof = np.zeros((nray, n_bins)), np.zeros(n_bins)
    _check(load().rays_hip_deposition(C.byref(p), DEP_PROFILES[which], int(n_bins), nray, _dp(ray_vec), _ip(npoints),
                                      _dp(power), _dp(work), _dp(prof)), "rays_hip_deposition")
    return work, prof


# RAYS_DIAG_* of include/rays_hip.h, in enum order; the names are the variables of the reference's
# ray_detailed_diagnostics files (axisym_toroid_processor_m.f90:424-445; X, Y: the slab processor's)
DIAG_FIELDS = ("s", "ne", "Te_kev", "modB", "alpha_e", "gamma_e", "Psi", "R", "X", "Y", "Z", "n_par", "n_perp",
               "P_absorbed", "n_imag", "xi_0", "xi_1", "xi_2", "residual")


def diag_field_mask(fields=None):
    """(bit mask, names in enum order -- the order of the output's leading dimension) of a selection of DIAG_FIELDS
    (None: all nineteen)."""
    if fields is None:
        fields = DIAG_FIELDS
    if isinstance(fields, str):
        fields = (fields,)
    unknown = [f for f in fields if f not in DIAG_FIELDS]
    if unknown or not len(fields):
        raise ValueError(f"ray diagnostics: unknown or empty field selection {unknown or fields}; known: {DIAG_FIELDS}")
    names = tuple(f for f in DIAG_FIELDS if f in fields)
    return sum(1 << DIAG_FIELDS.index(f) for f in names), names


def ray_diagnostics_device(p: RaysParams, nray: int, d_ray_vec: int, d_residual: int, d_npoints: int, fields,
                           d_out: int, d_first_bad_point: int = 0, stream: int = 0):
    """rays_hip_ray_diagnostics_device on device pointers (torch `.data_ptr()`s): d_out[k][nray][nstep_max+1] with k
    over the selected fields in DIAG_FIELDS order; asynchronous on `stream`.  Returns the names in that order."""
    ensure_tables(p)
    mask, names = diag_field_mask(fields)
    _check(load().rays_hip_ray_diagnostics_device(C.byref(p), int(nray), d_ray_vec, d_residual, d_npoints, mask, d_out,
                                                  d_first_bad_point or None, stream or None),
           "rays_hip_ray_diagnostics_device")
    return names


DIAG_IN_PADDED, DIAG_IN_PACKED = 0, 1   # RAYS_DIAG_IN_* of include/rays_hip.h


def point_offsets_device(nray: int, nstep_max: int, d_npoints: int, d_offsets: int, stream: int = 0):
    """rays_hip_point_offsets_device: d_offsets[0 .. nray] (int64) = exclusive prefix sum of clamp(npoints, 0,
    nstep_max + 1), the total in d_offsets[nray]; asynchronous on `stream`."""
    _check(load().rays_hip_point_offsets_device(int(nray), int(nstep_max), d_npoints or None, d_offsets or None,
                                                stream or None), "rays_hip_point_offsets_device")


def ray_diagnostics_packed_device(p: RaysParams, nray: int, d_ray_vec: int, d_residual: int, d_npoints: int,
                                  d_offsets: int, out_stride: int, fields, d_out: int, d_first_bad_point: int = 0,
                                  stream: int = 0, packed_input: bool = False):
    """rays_hip_ray_diagnostics_packed_device on device pointers: d_out[k][out_stride], point j of ray i at
    d_out[k][d_offsets[i] + j], nothing else written and nothing at or beyond out_stride of a field; d_ray_vec /
    d_residual are the padded arrays of the trace, or with packed_input the packed ones of pack_device.  Asynchronous
    on `stream`.  Returns the names in DIAG_FIELDS order."""
    ensure_tables(p)
    mask, names = diag_field_mask(fields)
    _check(load().rays_hip_ray_diagnostics_packed_device(
        C.byref(p), int(nray), DIAG_IN_PACKED if packed_input else DIAG_IN_PADDED, d_ray_vec, d_residual, d_npoints,
        d_offsets, int(out_stride), mask, d_out, d_first_bad_point or None, stream or None),
        "rays_hip_ray_diagnostics_packed_device")
    return names


def diag_offsets(npoints, nstep_max=None):
    """The host restatement of point_offsets_device: int64[nray + 1]."""
    n = np.asarray(npoints, dtype=np.int64)
    n = np.clip(n, 0, None if nstep_max is None else int(nstep_max) + 1)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(n, dtype=np.int64)])


def diag_unpack(packed, offsets, npt: int):
    """Host scatter of a packed diagnostics dictionary ({field: array[total]}, "offsets", "first_bad_point" as
    DeviceTrace.diagnostics(packed=True) / RayResults.diagnostics(packed=True) return it, as numpy arrays) into the
    padded one: {field: array[nray][npt]} with +0.0 wherever no point was recorded, "first_bad_point" passed on."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nray = len(offsets) - 1
    cnt = np.diff(offsets)
    if nray and (cnt.min() < 0 or cnt.max() > npt):
        raise ValueError("diag_unpack: `offsets` is not the prefix sum of point counts within 0 .. npt")
    total = int(offsets[-1])
    live = np.arange(npt)[None, :] < cnt[:, None]
    out = {}
    for k, a in packed.items():
        if k == "offsets":
            continue
        a = np.asarray(a)
        if k == "first_bad_point":
            out[k] = a
            continue
        if a.ndim != 1 or len(a) < total:
            raise ValueError(f"diag_unpack: {k} has shape {a.shape}, expected [>= {total}]")
        full = np.zeros((nray, npt))
        full[live] = a[:total]
        out[k] = full
    return out


def diag_pack(padded, npoints):
    """The inverse of diag_unpack: {field: array[nray][npt]} -> {field: array[total]} plus "offsets"."""
    npoints = np.asarray(npoints)
    out = {}
    npt = None
    for k, a in padded.items():
        a = np.asarray(a)
        if k == "first_bad_point":
            out[k] = a
            continue
        npt = a.shape[1]
        live = np.arange(npt)[None, :] < np.clip(npoints, 0, npt)[:, None]
        out[k] = np.ascontiguousarray(a[live])
    out["offsets"] = diag_offsets(npoints, None if npt is None else npt - 1)
    return out


def ray_diagnostics_host(p: RaysParams, ray_vec, residual, npoints, fields=None, block_rays: int = 0):
    """rays_hip_ray_diagnostics: the ray_results_m arrays in, ({name: array[nray][nstep_max+1]}, first_bad_point[nray])
    out.  Blocking, on the current device.  block_rays > 0 is a TEST HOOK: rays per device block instead of the
    library's bound of 2**21 trajectory slots per block, handed over by setting RAYS_HIP_DIAG_BLOCK_RAYS in os.environ
    around the call -- not thread-safe, and a child process started meanwhile inherits it."""
    ensure_tables(p)
    mask, names = diag_field_mask(fields)
    ray_vec = np.ascontiguousarray(ray_vec, dtype=np.float64)
    residual = np.ascontiguousarray(residual, dtype=np.float64)
    npoints = np.ascontiguousarray(npoints, dtype=np.int32)
    nray, npt = len(npoints), p.nstep_max + 1
    if ray_vec.shape != (nray, npt, p.nv) or residual.shape != (nray, npt):
        raise ValueError("ray_diagnostics_host: arrays do not have the ray_results_m shapes of this run")
    out = np.zeros((len(names), nray, npt))
    bad = np.zeros(nray, dtype=np.int32)
    saved = os.environ.get("RAYS_HIP_DIAG_BLOCK_RAYS")
    if block_rays:
        os.environ["RAYS_HIP_DIAG_BLOCK_RAYS"] = str(int(block_rays))
    try:
        rc = load().rays_hip_ray_diagnostics(C.byref(p), nray, _dp(ray_vec), _dp(residual), _ip(npoints), mask, _dp(out),
                                             _ip(bad))
    finally:
        if block_rays:
            if saved is None:
                del os.environ["RAYS_HIP_DIAG_BLOCK_RAYS"]
            else:
                os.environ["RAYS_HIP_DIAG_BLOCK_RAYS"] = saved
    _check(rc, "rays_hip_ray_diagnostics")
    return {n: out[k] for k, n in enumerate(names)}, bad


def ox_conv_kernel_name(p: RaysParams) -> str:
    """The scan kernel of the O-X conversion analysis for p's shape; raises where it is not built (make FULL=1)."""
    name = load().rays_hip_ox_conv_kernel_name_for(C.byref(p)).decode()
    if not name:
        raise RaysHipError("rays_hip_ox_conv_kernel_name_for: " + last_error())
    return name


def ox_conv_device(p: RaysParams, nray: int, d_ray_vec: int, d_npoints: int, out: dict, d_offsets: int = 0,
                   packed_input: bool = False, stream: int = 0):
    """rays_hip_ox_conv_device on device pointers: `out` maps field names of OX_FIELDS to device pointers (torch
    `.data_ptr()`s); a field that is missing or None is not wanted.  d_ray_vec: the padded trace array, or with
    packed_input the packed one with d_offsets[nray + 1].  Asynchronous on `stream`."""
    ensure_tables(p)
    unknown = [k for k in out if k not in [f for f, _, _ in OX_FIELDS]]
    if unknown:
        raise ValueError(f"ox_conv_device: unknown result fields {unknown}")
    res = OxResultStruct(**{f: (int(out[f]) if out.get(f) else None) for f, _, _ in OX_FIELDS})
    _check(load().rays_hip_ox_conv_device(C.byref(p), int(nray), DIAG_IN_PACKED if packed_input else DIAG_IN_PADDED,
                                          d_ray_vec, d_npoints, d_offsets or None, C.byref(res), stream),
           "rays_hip_ox_conv_device")


def ox_conv_host(p: RaysParams, ray_vec, npoints, fields=None, block_rays: int = 0) -> dict:
    """rays_hip_ox_conv: the ray_results_m arrays in; {field: array} for `fields` (names of OX_FIELDS; None = all) plus
    "number_of_rays_converted" and "converted_ray_number" (1-based, in ray order) out.  conv_coeff and the CONVERTED bit
    are the host libm's.  Blocking, on the current device.  block_rays > 0 is a TEST HOOK: rays per device block, handed
    over by setting RAYS_HIP_OX_BLOCK_RAYS in os.environ around the call (not thread-safe)."""
    ensure_tables(p)
    known = [f for f, _, _ in OX_FIELDS]
    fields = known if fields is None else list(fields)
    unknown = [k for k in fields if k not in known]
    if unknown:
        raise ValueError(f"ox_conv_host: unknown result fields {unknown}; known: {known}")
    ray_vec = np.ascontiguousarray(ray_vec, dtype=np.float64)
    npoints = np.ascontiguousarray(npoints, dtype=np.int32)
    nray, npt = len(npoints), p.nstep_max + 1
    if ray_vec.shape != (nray, npt, p.nv):
        raise ValueError("ox_conv_host: ray_vec does not have the ray_results_m shape of this run")
    out = {f: np.zeros((nray, w) if w > 1 else nray, dtype=dt) for f, dt, w in OX_FIELDS if f in fields}
    res = OxResultStruct(**{f: (out[f].ctypes.data if f in out else None) for f, _, _ in OX_FIELDS})
    n_conv = C.c_int32(0)
    conv = np.zeros(max(nray, 1), dtype=np.int32)
    saved = os.environ.get("RAYS_HIP_OX_BLOCK_RAYS")
    if block_rays:
        os.environ["RAYS_HIP_OX_BLOCK_RAYS"] = str(int(block_rays))
    try:
        rc = load().rays_hip_ox_conv(C.byref(p), nray, _dp(ray_vec), _ip(npoints), C.byref(res), C.byref(n_conv), _ip(conv))
    finally:
        if block_rays:
            if saved is None:
                del os.environ["RAYS_HIP_OX_BLOCK_RAYS"]
            else:
                os.environ["RAYS_HIP_OX_BLOCK_RAYS"] = saved
    _check(rc, "rays_hip_ox_conv")
    out["number_of_rays_converted"] = int(n_conv.value)
    out["converted_ray_number"] = conv[:n_conv.value].copy()
    return out


NO_KEPT_RESULT = 5   # RAYS_HIP_NO_KEPT_RESULT


def keep_last_result(on: bool) -> bool:
    """rays_hip_keep_last_result: later trace_host calls leave their result's device image in place for
    deposition_last (until the next trace_host / keep_last_result(False)).  Returns the previous setting."""
    return bool(load().rays_hip_keep_last_result(1 if on else 0))


def deposition_last(p: RaysParams, which: str, n_bins: int, initial_ray_power, want_work: bool = True):
    """rays_hip_deposition_last: the profiles of the rays the last trace_host call traced, binned on the device(s) that
    hold them (no trajectory upload).  Returns (work[nray][n_bins] or None, profile[n_bins]), or None when no such
    image is held."""
    power = np.ascontiguousarray(initial_ray_power, dtype=np.float64)
    nray = len(power)
    work = np.zeros((nray, n_bins)) if want_work else None
    prof = np.zeros(n_bins)
    rc = load().rays_hip_deposition_last(C.byref(p), DEP_PROFILES[which], int(n_bins), nray, _dp(power),
                                         _dp(work) if want_work else None, _dp(prof))
    if rc == NO_KEPT_RESULT:
        return None
    _check(rc, "rays_hip_deposition_last")
    return work, prof


def trace_host(p: RaysParams, rvec0, rindex_vec0, ngpu: int = 0, out: dict = None) -> dict:
    """rays_hip_trace: host numpy arrays in / out (the Fortran drop-in entry).  `out`: the result
    arrays of an earlier call over the same fan to write into (the library overwrites points
    1..npoints only, so they must hold zeros or an earlier result of the same fan -- the Fortran host's
    situation, whose arrays are allocated and zero-filled once by initialize_ray_results_m)."""
    lib = load()
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    nray, nv, npt = len(rvec0), p.nv, p.nstep_max + 1
    if ngpu is not None and lib.rays_hip_init(int(ngpu)) < 0:   # None: keep the init_devices() selection
        raise RaysHipError("rays_hip_init: " + last_error())
    ensure_tables(p)
    if out is None:
        out = dict(
            ray_vec=np.zeros((nray, npt, nv)), residual=np.zeros((nray, npt)),
            npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
            end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray), max_residuals=np.zeros(nray))
    elif out["ray_vec"].shape != (nray, npt, nv) or not out["ray_vec"].flags.c_contiguous:
        raise ValueError("trace_host: `out` does not match this fan")
    el = C.c_double(0.0)
    rc = lib.rays_hip_trace(C.byref(p), nray, _dp(rvec0), _dp(rindex_vec0), _dp(out["ray_vec"]),
                            _dp(out["residual"]), _ip(out["npoints"]), _ip(out["stop_code"]),
                            _dp(out["end_ray_vec"]), _dp(out["end_residuals"]),
                            _dp(out["max_residuals"]), C.byref(el))
    _check(rc, "rays_hip_trace")
    out["elapsed_s"] = el.value
    return out


def trace_gather(p: RaysParams, rvec0, rindex_vec0, to_host: bool = True):
    """rays_hip_trace_gather: rays sharded over the selected devices, trajectories gathered on the root device
    with RCCL.  Returns the device-resident result block and, with to_host, the arrays copied out."""
    lib = load()
    ensure_tables(p)
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    res = DeviceResult()
    _check(lib.rays_hip_trace_gather(C.byref(p), len(rvec0), _dp(rvec0), _dp(rindex_vec0), C.byref(res)),
           "rays_hip_trace_gather")
    if not to_host:
        return res, None
    nray, nv, npt = len(rvec0), p.nv, p.nstep_max + 1
    out = dict(ray_vec=np.zeros((nray, npt, nv)), residual=np.zeros((nray, npt)),
               npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
               end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray), max_residuals=np.zeros(nray))
    _check(lib.rays_hip_result_to_host(C.byref(p), C.byref(res), _dp(out["ray_vec"]), _dp(out["residual"]),
                                       _ip(out["npoints"]), _ip(out["stop_code"]), _dp(out["end_ray_vec"]),
                                       _dp(out["end_residuals"]), _dp(out["max_residuals"])),
           "rays_hip_result_to_host")
    return res, out


def trace_device(p: RaysParams, nray: int, d_rvec0: int, d_rindex_vec0: int, d_ray_vec: int,
                 d_residual: int, d_npoints: int, d_stop_code: int, d_end_ray_vec: int = 0,
                 d_end_residuals: int = 0, d_max_residuals: int = 0, stream: int = 0,
                 zero_fill: bool = True):
    """rays_hip_trace_device: raw device pointers (ints), asynchronous on `stream`."""
    ensure_tables(p)
    rc = load().rays_hip_trace_device(
        C.byref(p), int(nray), d_rvec0, d_rindex_vec0, d_ray_vec, d_residual, d_npoints, d_stop_code,
        d_end_ray_vec or None, d_end_residuals or None, d_max_residuals or None, stream or None,
        0 if zero_fill else 1)
    _check(rc, "rays_hip_trace_device")


def scan_device(p: RaysParams, n_runs: int, d_ds_values: int, nray: int, d_rvec0: int, d_rindex_vec0: int,
                d_ray_vec: int, d_residual: int, d_npoints: int, d_stop_code: int, d_end_ray_vec: int = 0,
                d_end_residuals: int = 0, d_max_residuals: int = 0, stream: int = 0, zero_fill: bool = True):
    """rays_hip_scan_device: all runs of a `ds` scan in ONE launch (outputs carry a leading run dimension)."""
    ensure_tables(p)
    rc = load().rays_hip_scan_device(
        C.byref(p), int(n_runs), d_ds_values, int(nray), d_rvec0, d_rindex_vec0, d_ray_vec, d_residual,
        d_npoints, d_stop_code, d_end_ray_vec or None, d_end_residuals or None, d_max_residuals or None,
        stream or None, 0 if zero_fill else 1)
    _check(rc, "rays_hip_scan_device")


def trace_summary_host(p: RaysParams, rvec0, rindex_vec0, ngpu: int = 0) -> dict:
    """rays_hip_trace_summary: host numpy arrays in, the per-ray summaries out -- no trajectory exists anywhere.
    ngpu as for trace_host (None: keep the init_devices() selection)."""
    lib = load()
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    nray, nv = len(rvec0), p.nv
    if ngpu is not None and lib.rays_hip_init(int(ngpu)) < 0:
        raise RaysHipError("rays_hip_init: " + last_error())
    ensure_tables(p)
    out = dict(npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
               start_ray_vec=np.zeros((nray, nv)), end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray),
               max_residuals=np.zeros(nray))
    el = C.c_double(0.0)
    rc = lib.rays_hip_trace_summary(C.byref(p), nray, _dp(rvec0), _dp(rindex_vec0), _ip(out["npoints"]),
                                    _ip(out["stop_code"]), _dp(out["start_ray_vec"]), _dp(out["end_ray_vec"]),
                                    _dp(out["end_residuals"]), _dp(out["max_residuals"]), C.byref(el))
    _check(rc, "rays_hip_trace_summary")
    out["elapsed_s"] = el.value
    return out


def trace_summary_device(p: RaysParams, nray: int, d_rvec0: int, d_rindex_vec0: int, d_npoints: int, d_stop_code: int,
                         d_start_ray_vec: int, d_end_ray_vec: int, d_end_residuals: int, d_max_residuals: int,
                         stream: int = 0):
    """rays_hip_trace_summary_device: raw device pointers (ints; d_start_ray_vec may be 0), asynchronous on `stream`."""
    ensure_tables(p)
    rc = load().rays_hip_trace_summary_device(
        C.byref(p), int(nray), d_rvec0 or None, d_rindex_vec0 or None, d_npoints or None, d_stop_code or None,
        d_start_ray_vec or None, d_end_ray_vec or None, d_end_residuals or None, d_max_residuals or None,
        stream or None)
    _check(rc, "rays_hip_trace_summary_device")


def _dep_which(which) -> int:
    if which not in DEP_PROFILES:
        raise ValueError(f"deposition profile {which!r}: known are {tuple(DEP_PROFILES)}")
    return DEP_PROFILES[which]


def deposition_kernel_name(p: RaysParams, nray: int = 0) -> str:
    """Kernel specialisation a fused trace + deposition of `nray` rays would launch (always an exact kernel: the
    summary-only kernel's name with EQ + 64)."""
    name = load().rays_hip_deposition_kernel_name_for(C.byref(p), int(nray)).decode()
    if not name:
        check_params(p)
        raise RaysHipError("rays_hip_deposition_kernel_name_for: no fused deposition kernel for this configuration")
    return name


def trace_deposition_device(p: RaysParams, nray: int, d_rvec0: int, d_rindex_vec0: int, d_power: int, which: str,
                            n_bins: int, d_npoints: int, d_stop_code: int, d_start_ray_vec: int, d_end_ray_vec: int,
                            d_end_residuals: int, d_max_residuals: int, d_work: int, d_profile_in, d_profile_out: int,
                            stream: int = 0):
    """rays_hip_trace_deposition_device: raw device pointers (ints; d_start_ray_vec and d_profile_in may be 0 / None),
    asynchronous on `stream`.  d_work[n_bins][nray] is zeroed by the call; the profile continues d_profile_in."""
    w = _dep_which(which)
    ensure_tables(p)
    rc = load().rays_hip_trace_deposition_device(
        C.byref(p), int(nray), d_rvec0 or None, d_rindex_vec0 or None, d_power or None, w, int(n_bins),
        d_npoints or None, d_stop_code or None, d_start_ray_vec or None, d_end_ray_vec or None, d_end_residuals or None,
        d_max_residuals or None, d_work or None, d_profile_in or None, d_profile_out or None, stream or None)
    _check(rc, "rays_hip_trace_deposition_device")


def trace_deposition_host(p: RaysParams, rvec0, rindex_vec0, initial_ray_power, which: str, n_bins: int, ngpu: int = 0,
                          want_work: bool = True) -> dict:
    """rays_hip_trace_deposition: host numpy arrays in; the per-ray summaries, profile[n_bins] and (want_work)
    work[nray][n_bins] out -- no trajectory exists anywhere.  ngpu as for trace_host (None: keep the init_devices()
    selection)."""
    lib = load()
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    power = np.ascontiguousarray(initial_ray_power, dtype=np.float64)
    nray, nv = len(rvec0), p.nv
    if power.shape != (nray,):
        raise ValueError("trace_deposition_host: initial_ray_power must hold one weight per ray")
    w = _dep_which(which)
    if ngpu is not None and lib.rays_hip_init(int(ngpu)) < 0:
        raise RaysHipError("rays_hip_init: " + last_error())
    ensure_tables(p)
    nb = max(int(n_bins), 0)
    out = dict(npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
               start_ray_vec=np.zeros((nray, nv)), end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray),
               max_residuals=np.zeros(nray), work=np.zeros((nray, nb)) if want_work else None, profile=np.zeros(nb))
    el = C.c_double(0.0)
    rc = lib.rays_hip_trace_deposition(C.byref(p), nray, _dp(rvec0), _dp(rindex_vec0), _dp(power), w, int(n_bins),
                                       _ip(out["npoints"]), _ip(out["stop_code"]), _dp(out["start_ray_vec"]),
                                       _dp(out["end_ray_vec"]), _dp(out["end_residuals"]), _dp(out["max_residuals"]),
                                       _dp(out["work"]) if want_work else None, _dp(out["profile"]), C.byref(el))
    _check(rc, "rays_hip_trace_deposition")
    out["elapsed_s"] = el.value
    return out


def deposition_profile_set(p: RaysParams) -> tuple:
    """rays_hip_deposition_profile_set: the names of the profiles of p's equilibrium, in the reference's order
    (calculate_deposition_profiles loops over all of them)."""
    ensure_tables(p)
    which = (C.c_int * DEP_MAX_PROFILES)()
    n = load().rays_hip_deposition_profile_set(C.byref(p), which)
    names = {v: k for k, v in DEP_PROFILES.items()}
    return tuple(names[which[i]] for i in range(n))


def profiles_kernel_name(p: RaysParams, nray: int, n_profiles: int) -> str:
    """Kernel rays_hip_trace_profiles* would launch for n_profiles records; "" where there is none (two profiles on a
    slab or Solovev configuration)."""
    return load().rays_hip_profiles_kernel_name_for(C.byref(p), int(nray), int(n_profiles)).decode()


def _profile_records(records):
    """[(which, n_bins, work, profile_in, profile), ...] (addresses as ints or None) -> the C array"""
    arr = (DepProfileStruct * max(len(records), 1))()
    for r, (which, n_bins, work, profile_in, profile) in zip(arr, records):
        r.which, r.n_bins = _dep_which(which), int(n_bins)
        r.work, r.profile_in, r.profile = work or None, profile_in or None, profile or None
    return arr


def trace_profiles_device(p: RaysParams, nray: int, d_rvec0: int, d_rindex_vec0: int, d_power: int, records,
                          d_npoints: int, d_stop_code: int, d_start_ray_vec: int, d_end_ray_vec: int,
                          d_end_residuals: int, d_max_residuals: int, stream: int = 0):
    """rays_hip_trace_profiles_device: raw device pointers (ints); records = [(which, n_bins, d_work, d_profile_in,
    d_profile), ...], one or two.  Asynchronous on `stream`; every work is zeroed by the call."""
    arr = _profile_records(records)
    ensure_tables(p)
    rc = load().rays_hip_trace_profiles_device(
        C.byref(p), int(nray), d_rvec0 or None, d_rindex_vec0 or None, d_power or None, len(records), arr,
        d_npoints or None, d_stop_code or None, d_start_ray_vec or None, d_end_ray_vec or None, d_end_residuals or None,
        d_max_residuals or None, stream or None)
    _check(rc, "rays_hip_trace_profiles_device")


def trace_profiles_host(p: RaysParams, rvec0, rindex_vec0, initial_ray_power, profiles, ngpu: int = 0,
                        want_work: bool = True) -> dict:
    """rays_hip_trace_profiles: host numpy arrays in; profiles = [(which, n_bins), ...].  Out: the per-ray summaries,
    and `works` / `profiles` as lists in the order asked (work[nray][n_bins]; None without want_work)."""
    lib = load()
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    power = np.ascontiguousarray(initial_ray_power, dtype=np.float64)
    nray, nv = len(rvec0), p.nv
    if power.shape != (nray,):
        raise ValueError("trace_profiles_host: initial_ray_power must hold one weight per ray")
    if ngpu is not None and lib.rays_hip_init(int(ngpu)) < 0:
        raise RaysHipError("rays_hip_init: " + last_error())
    ensure_tables(p)
    out = dict(npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
               start_ray_vec=np.zeros((nray, nv)), end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray),
               max_residuals=np.zeros(nray), works=[], profiles=[])
    records = []
    for which, n_bins in profiles:
        nb = max(int(n_bins), 0)
        out["works"].append(np.zeros((nray, nb)) if want_work else None)
        out["profiles"].append(np.zeros(nb))
        records.append((which, n_bins, out["works"][-1].ctypes.data if want_work else None, None,
                        out["profiles"][-1].ctypes.data))
    arr = _profile_records(records)
    el = C.c_double(0.0)
    rc = lib.rays_hip_trace_profiles(C.byref(p), nray, _dp(rvec0), _dp(rindex_vec0), _dp(power), len(records), arr,
                                     _ip(out["npoints"]), _ip(out["stop_code"]), _dp(out["start_ray_vec"]),
                                     _dp(out["end_ray_vec"]), _dp(out["end_residuals"]), _dp(out["max_residuals"]),
                                     C.byref(el))
    _check(rc, "rays_hip_trace_profiles")
    out["elapsed_s"] = el.value
    return out


def profile_sum_segments(work, segments, profile_in=None, profile_out=None, stream: int = 0):
    """rays_hip_profile_sum_segments_device on torch CUDA tensors: work[n_bins][nray] (float64, contiguous); segments: an
    int32 CUDA tensor of n_seg + 1 offsets, or (n_seg, rays_per_seg) for uniform segments; profile_in / profile_out
    [n_seg][n_bins] (profile_out is allocated when None; the same tensor for both is allowed).  Returns profile_out.
    Asynchronous on `stream`."""
    import torch

    if work.dim() != 2 or work.dtype != torch.float64 or not work.is_contiguous() or not work.is_cuda:
        raise ValueError("profile_sum_segments: work is a contiguous float64 CUDA tensor [n_bins][nray]")
    n_bins, nray = int(work.shape[0]), int(work.shape[1])
    if torch.is_tensor(segments):
        if segments.dtype != torch.int32 or segments.dim() != 1 or not segments.is_contiguous() or not segments.is_cuda or \
                len(segments) < 1:
            raise ValueError("profile_sum_segments: offsets are a contiguous int32 CUDA tensor of n_seg + 1 entries")
        n_seg, d_off, per = len(segments) - 1, segments.data_ptr(), 0
    else:
        n_seg, per = (int(x) for x in segments)
        d_off = None
    for name, t in (("profile_in", profile_in), ("profile_out", profile_out)):
        if t is not None and (tuple(t.shape) != (n_seg, n_bins) or t.dtype != torch.float64 or not t.is_contiguous()
                              or not t.is_cuda):
            raise ValueError(f"profile_sum_segments: {name} is a contiguous float64 CUDA tensor [n_seg][n_bins]")
    if profile_out is None:
        profile_out = torch.empty((max(n_seg, 0), n_bins), dtype=torch.float64, device=work.device)
    rc = load().rays_hip_profile_sum_segments_device(
        n_bins, nray, n_seg, d_off, per, work.data_ptr() or None, None if profile_in is None else profile_in.data_ptr(),
        profile_out.data_ptr() or None, stream or None)
    _check(rc, "rays_hip_profile_sum_segments_device")
    return profile_out


def scan_profiles_device(p: RaysParams, n_runs: int, d_ds_values: int, nray: int, d_rvec0: int, d_rindex_vec0: int,
                         d_power: int, records, d_npoints: int, d_stop_code: int, d_start_ray_vec: int,
                         d_end_ray_vec: int, d_end_residuals: int, d_max_residuals: int, stream: int = 0):
    """rays_hip_scan_profiles_device: the fused ds scan, raw device pointers (ints).  The starts and d_power are per fan
    member; records = [(which, n_bins, d_work[n_bins][n_runs * nray], d_profile_in, d_profile[n_runs][n_bins]), ...];
    the summaries are [n_runs * nray].  Asynchronous on `stream`; every work is zeroed by the call."""
    arr = _profile_records(records)
    ensure_tables(p)
    rc = load().rays_hip_scan_profiles_device(
        C.byref(p), int(n_runs), d_ds_values or None, int(nray), d_rvec0 or None, d_rindex_vec0 or None, d_power or None,
        len(records), arr, d_npoints or None, d_stop_code or None, d_start_ray_vec or None, d_end_ray_vec or None,
        d_end_residuals or None, d_max_residuals or None, stream or None)
    _check(rc, "rays_hip_scan_profiles_device")


def trace_profiles_segments_device(p: RaysParams, nray: int, d_rvec0: int, d_rindex_vec0: int, d_power: int, records,
                                   n_seg: int, d_seg_offsets, rays_per_seg: int, d_npoints: int, d_stop_code: int,
                                   d_start_ray_vec: int, d_end_ray_vec: int, d_end_residuals: int, d_max_residuals: int,
                                   stream: int = 0):
    """rays_hip_trace_profiles_segments_device: trace_profiles_device with one profile per segment of rays -- d_profile_in
    and d_profile of every record are [n_seg][n_bins]; d_seg_offsets: int32[n_seg + 1] on the device, or 0 / None with a
    uniform rays_per_seg."""
    arr = _profile_records(records)
    ensure_tables(p)
    rc = load().rays_hip_trace_profiles_segments_device(
        C.byref(p), int(nray), d_rvec0 or None, d_rindex_vec0 or None, d_power or None, len(records), arr, int(n_seg),
        d_seg_offsets or None, int(rays_per_seg), d_npoints or None, d_stop_code or None, d_start_ray_vec or None,
        d_end_ray_vec or None, d_end_residuals or None, d_max_residuals or None, stream or None)
    _check(rc, "rays_hip_trace_profiles_segments_device")


def window_kernel_name(p: RaysParams, nray: int = 0, recording: bool = True) -> str:
    """Kernel a window of `nray` rays would launch (always exact, always the one-ray-per-lane kernel: the recording
    kernel's name with EQ + 128, the summary-only kernel's for recording=False)."""
    name = load().rays_hip_window_kernel_name_for(C.byref(p), int(nray), 1 if recording else 0).decode()
    if not name:
        check_params(p)
        raise RaysHipError("rays_hip_window_kernel_name_for: no continuation kernel for this configuration")
    return name


def _state_struct(state) -> RayStateStruct:
    """state: an object with the seven attributes of rays_ray_state_t as device tensors (sg_err may be None)."""
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    return RayStateStruct(ptr(state.v), ptr(state.s), ptr(state.nstep), ptr(state.stop_code), ptr(state.resid),
                          ptr(state.sg_err), ptr(state.flags))


def state_init_device(p: RaysParams, nray: int, d_rvec0: int, d_rindex_vec0: int, state, d_start_ray_vec: int = 0,
                      stream: int = 0):
    """rays_hip_state_init_device: the saved ray state of every ray at its launch point (initialize_ode_vector and the
    initial check_save); d_start_ray_vec (may be 0) gets point 1.  Asynchronous on `stream`."""
    ensure_tables(p)
    st = _state_struct(state)
    _check(load().rays_hip_state_init_device(C.byref(p), int(nray), d_rvec0 or None, d_rindex_vec0 or None, C.byref(st),
                                             d_start_ray_vec or None, stream or None), "rays_hip_state_init_device")


def trace_window_device(p: RaysParams, nray: int, state, n_steps: int, d_ray_vec_win: int, d_residual_win: int,
                        d_npoints_win: int, stream: int = 0):
    """rays_hip_trace_window_device: every ray under way advances by at most n_steps recorded steps; the state is updated
    in place.  Both window arrays 0: a summary window.  Asynchronous on `stream`."""
    ensure_tables(p)
    st = _state_struct(state)
    _check(load().rays_hip_trace_window_device(C.byref(p), int(nray), C.byref(st), int(n_steps), d_ray_vec_win or None,
                                               d_residual_win or None, d_npoints_win or None, stream or None),
           "rays_hip_trace_window_device")


def state_summary_device(p: RaysParams, nray: int, state, d_npoints: int, d_stop_code: int, d_end_ray_vec: int,
                         d_end_residuals: int, d_max_residuals: int, stream: int = 0):
    """rays_hip_state_summary_device: the five per-ray summary arrays of a trace from the state."""
    st = _state_struct(state)
    _check(load().rays_hip_state_summary_device(C.byref(p), int(nray), C.byref(st), d_npoints or None, d_stop_code or None,
                                                d_end_ray_vec or None, d_end_residuals or None, d_max_residuals or None,
                                                stream or None), "rays_hip_state_summary_device")


def window_profiles_kernel_name(p: RaysParams, nray: int, n_profiles: int) -> str:
    """Kernel rays_hip_trace_window_profiles_device would launch for n_profiles records (the fused deposition kernel's
    name with EQ + 128); "" where there is none."""
    return load().rays_hip_window_profiles_kernel_name_for(C.byref(p), int(nray), int(n_profiles)).decode()


def trace_window_profiles_device(p: RaysParams, nray: int, state, n_steps: int, d_power: int, records,
                                 d_npoints_win: int, stream: int = 0):
    """rays_hip_trace_window_profiles_device: a summary-policy window that bins every point it accepts.  records =
    [(which, n_bins, d_work, d_profile_in, d_profile), ...], one or two; each work is an accumulator the call never
    zeroes; d_profile 0 = no sum in this window.  Asynchronous on `stream`."""
    arr = _profile_records(records)
    ensure_tables(p)
    st = _state_struct(state)
    _check(load().rays_hip_trace_window_profiles_device(C.byref(p), int(nray), C.byref(st), int(n_steps), d_power or None,
                                                        len(records), arr, d_npoints_win or None, stream or None),
           "rays_hip_trace_window_profiles_device")


def trace_windowed_host(p: RaysParams, rvec0, rindex_vec0, n_steps: int, ngpu: int = 0, out: dict = None) -> dict:
    """rays_hip_trace_windowed: trace_host's arguments and results, traced in windows of n_steps on one device -- the
    device holds the ray state and two window slabs, never [nray][nstep_max + 1][nv]."""
    lib = load()
    rvec0 = np.ascontiguousarray(rvec0, dtype=np.float64)
    rindex_vec0 = np.ascontiguousarray(rindex_vec0, dtype=np.float64)
    nray, nv, npt = len(rvec0), p.nv, p.nstep_max + 1
    if ngpu is not None and lib.rays_hip_init(int(ngpu)) < 0:
        raise RaysHipError("rays_hip_init: " + last_error())
    ensure_tables(p)
    if out is None:
        out = dict(
            ray_vec=np.zeros((nray, npt, nv)), residual=np.zeros((nray, npt)),
            npoints=np.zeros(nray, dtype=np.int32), stop_code=np.zeros(nray, dtype=np.int32),
            end_ray_vec=np.zeros((nray, nv)), end_residuals=np.zeros(nray), max_residuals=np.zeros(nray))
    elif out["ray_vec"].shape != (nray, npt, nv) or not out["ray_vec"].flags.c_contiguous:
        raise ValueError("trace_windowed_host: `out` does not match this fan")
    el = C.c_double(0.0)
    rc = lib.rays_hip_trace_windowed(C.byref(p), nray, _dp(rvec0), _dp(rindex_vec0), int(n_steps), _dp(out["ray_vec"]),
                                     _dp(out["residual"]), _ip(out["npoints"]), _ip(out["stop_code"]),
                                     _dp(out["end_ray_vec"]), _dp(out["end_residuals"]), _dp(out["max_residuals"]),
                                     C.byref(el))
    _check(rc, "rays_hip_trace_windowed")
    out["elapsed_s"] = el.value
    return out


def scan_summary_device(p: RaysParams, n_runs: int, d_ds_values: int, nray: int, d_rvec0: int, d_rindex_vec0: int,
                        d_npoints: int, d_stop_code: int, d_start_ray_vec: int, d_end_ray_vec: int,
                        d_end_residuals: int, d_max_residuals: int, stream: int = 0):
    """rays_hip_scan_summary_device: all runs of a `ds` scan in ONE summary-only launch (leading run dimension)."""
    ensure_tables(p)
    rc = load().rays_hip_scan_summary_device(
        C.byref(p), int(n_runs), d_ds_values or None, int(nray), d_rvec0 or None, d_rindex_vec0 or None,
        d_npoints or None, d_stop_code or None, d_start_ray_vec or None, d_end_ray_vec or None,
        d_end_residuals or None, d_max_residuals or None, stream or None)
    _check(rc, "rays_hip_scan_summary_device")


def ode_step(p: RaysParams, v0, s0=None):
    """rays_hip_ode_step_device on host arrays (through torch device buffers): one output step of the
    configured ODE solver + check_save from each state v0[n][nv].  Returns (v1, resid, stop_code)."""
    import torch

    ensure_tables(p)
    v0 = np.ascontiguousarray(v0, dtype=np.float64).reshape(-1, p.nv)
    n = len(v0)
    d_v0 = torch.as_tensor(v0).cuda()
    d_s0 = None if s0 is None else torch.as_tensor(np.ascontiguousarray(s0, dtype=np.float64)).cuda()
    d_v1 = torch.zeros((n, p.nv), dtype=torch.float64, device="cuda")
    d_res = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    rc = load().rays_hip_ode_step_device(C.byref(p), n, d_v0.data_ptr(), None if d_s0 is None else d_s0.data_ptr(),
                                         d_v1.data_ptr(), d_res.data_ptr(), d_sc.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream or None)
    _check(rc, "rays_hip_ode_step_device")
    return d_v1.cpu().numpy(), d_res.cpu().numpy(), d_sc.cpu().numpy()


def pack_device(nray, nv, nstep_max, d_npoints, d_offsets, d_ray_vec, d_residual, d_packed_vec,
                d_packed_res, stream=0):
    _check(load().rays_hip_pack_device(int(nray), int(nv), int(nstep_max), d_npoints, d_offsets,
                                       d_ray_vec, d_residual, d_packed_vec, d_packed_res,
                                       stream or None), "rays_hip_pack_device")


def unpack_device(nray, nv, nstep_max, d_npoints, d_offsets, d_packed_vec, d_packed_res, d_ray_vec,
                  d_residual, stream=0):
    _check(load().rays_hip_unpack_device(int(nray), int(nv), int(nstep_max), d_npoints, d_offsets,
                                         d_packed_vec, d_packed_res, d_ray_vec, d_residual,
                                         stream or None), "rays_hip_unpack_device")


def probe(p: RaysParams, v) -> dict:
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, p.nv)
    n = len(v)
    cold, num = np.zeros((n, 7)), np.zeros((n, 7))
    dvds, resid, codes = np.zeros((n, p.nv)), np.zeros(n), np.zeros((n, 4), dtype=np.int32)
    rc = load().rays_hip_probe(C.byref(p), n, _dp(v), _dp(cold), _dp(num), _dp(dvds), _dp(resid),
                               _ip(codes))
    _check(rc, "rays_hip_probe")
    return dict(cold=cold, num=num, dvds=dvds, resid=resid, codes=codes)
