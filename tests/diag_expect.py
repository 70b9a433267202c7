"""Expected values of the per-point ray diagnostics (include/rays_hip.h: RAYS_DIAG_*), built from an `eq_point` record
(the reference's own, cut by oracle/ref_dump_driver.f90, or the oracle's, which tests/test_cpu_oracle.py pins to it bit
for bit) with the formulae of axisym_toroid_processor_m.f90:355-415 evaluated in numpy float64 in the reference's
written order -- test infrastructure shared by the CPU and the GPU tier."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

from rays_amd import hip
from rays_amd.params import AxisymTables, RaysParams, axisym_tables_struct, copy_params
from rays_amd.ray_init import _axisym_fields, _host_fields
from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = hip.DIAG_FIELDS
E_CHARGE = float(np.float32(1.6022e-19))   # constants_m.f90:48: a default-real literal
EQ_NEEDING = ("ne", "Te_kev", "modB", "alpha_e", "gamma_e", "n_par", "n_perp", "n_imag", "xi_0", "xi_1", "xi_2")


def assert_bits(got, want, what=""):
    """bit-equal, NaN matching NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} values differ; first at {tuple(i)}: "
                             f"got {got[tuple(i)]!r}, want {want[tuple(i)]!r}")


# ---- the emulated diag_point (tests/hip_emul/emul_diag.cpp) ---------------------------------------------------------
_DIR = os.path.join(ROOT, "tests", "hip_emul")
_emul = None


def emul_lib():
    global _emul
    if _emul is None:
        subprocess.check_call(["make", "-s", "-C", _DIR, "-f", "Makefile.diag"])
        lib = C.CDLL(os.path.join(_DIR, "librays_emul_diag.so"))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.rays_emul_ray_diagnostics.restype = C.c_int
        lib.rays_emul_ray_diagnostics.argtypes = [C.POINTER(RaysParams), C.c_int, dp, dp, ip, C.c_uint32, dp, ip]
        lib.rays_emul_diag_set_zfun_table.argtypes = [dp, C.c_int, C.c_double, C.c_double]
        z = np.load(os.path.join(ROOT, "rays_amd", "data", "zfun_spline_re.npz"))
        f = np.ascontiguousarray(z["fspl_re"], dtype=np.float64)
        lib.rays_emul_diag_set_zfun_table(f.ctypes.data_as(dp), len(f), float(z["x_min"]), float(z["x_max"]))
        lib.rays_emul_diag_set_axisym_tables.argtypes = [C.POINTER(AxisymTables), C.c_int, C.c_double, C.c_double]
        _emul = lib
    return _emul


def emul_set_tables(tab):
    if tab and any(np.size(tab.get(k, ())) for k in ("r_grid", "ne_grid", "te_grid", "ti_grid")):
        t, keep = axisym_tables_struct(tab)
        lin = "lin_psi" in tab
        emul_lib().rays_emul_diag_set_axisym_tables(C.byref(t), int(lin), float(tab["lin_dR"]) if lin else 0.0,
                                                    float(tab["lin_dZ"]) if lin else 0.0)


def emul_diagnostics(p, ray_vec, residual, npoints, fields=None):
    """rays_emul_ray_diagnostics: ({name: array[nray][npt]}, first_bad_point) like hip.ray_diagnostics_host"""
    mask, names = hip.diag_field_mask(fields)
    ray_vec = np.ascontiguousarray(ray_vec, dtype=np.float64)
    residual = np.ascontiguousarray(residual, dtype=np.float64)
    npoints = np.ascontiguousarray(npoints, dtype=np.int32)
    nray, npt = residual.shape
    q = copy_params(p)
    q.nstep_max = npt - 1
    assert ray_vec.shape == (nray, npt, p.nv)
    out = np.full((len(names), nray, npt), np.nan)
    bad = np.zeros(nray, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = emul_lib().rays_emul_ray_diagnostics(C.byref(q), nray, ray_vec.ctypes.data_as(dp), residual.ctypes.data_as(dp),
                                              npoints.ctypes.data_as(ip), mask, out.ctypes.data_as(dp), bad.ctypes.data_as(ip))
    assert rc == 0, f"rays_emul_ray_diagnostics rc={rc}"
    return {n: out[k] for k, n in enumerate(names)}, bad


# ---- expectations -----------------------------------------------------------------------------------------------------
def from_eq_record(p, v, eq, resid):
    """NE .. XI_2, R and the copies at one state from an eq_point record (layout: oracle/rays_oracle.c
    rays_oracle_probe): the table of include/rays_hip.h, left to right.  N_IMAG and PSI are not in the record."""
    f64 = np.float64
    v = np.asarray(v, dtype=f64)
    eq = np.asarray(eq, dtype=f64)
    bmag, bunit = eq[3], eq[7:10]
    ns0, ts0, omgc0, alpha0, gamma0 = eq[28], eq[32], eq[36], eq[38], eq[39]
    kvec = v[3:6]
    with np.errstate(all="ignore"):
        k3 = (kvec[0] * bunit[0] + kvec[1] * bunit[1]) + kvec[2] * bunit[2]
        d = kvec - k3 * bunit
        k1 = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        out = dict(s=v[6], X=v[0], Y=v[1], Z=v[2], R=np.sqrt(v[0] * v[0] + v[1] * v[1]), residual=f64(resid),
                   P_absorbed=v[7] if p.damping_model else f64(0.0),
                   ne=ns0, modB=bmag, alpha_e=alpha0, gamma_e=abs(gamma0), Te_kev=ts0 / f64(E_CHARGE) / f64(1000.0),
                   n_par=k3 / f64(p.k0), n_perp=k1 / f64(p.k0), xi_0=f64(0.0), xi_1=f64(0.0), xi_2=f64(0.0))
        if ts0 > 0.0 and abs(k3) > 0.0:
            vth = np.sqrt(f64(2.0) * ts0 / f64(p.ms[0]))
            out.update(xi_0=f64(p.omgrf) / (k3 * vth), xi_1=(f64(p.omgrf) + omgc0) / (k3 * vth),
                       xi_2=(f64(p.omgrf) + f64(2.0) * omgc0) / (k3 * vth))
    return out


def _probe_params(p):
    """nv = 7 | 8, ray_param = arcl, no gradient / species rows: then dvds(8) = 2 ki exactly at v(8) = 0
    (eqn_ray.f90:203)"""
    q = copy_params(p)
    q.multi_spec_damping = 0
    q.integrate_eq_gradients = 0
    q.ray_param = 0
    q.nv = 8 if p.damping_model else 7
    return q


def n_imag_expected(p, v, q=None):
    if not p.damping_model:
        return np.float64(0.0)
    q = q or _probe_params(p)
    v8 = np.concatenate([np.asarray(v, dtype=np.float64)[:7], [0.0]])
    o = oracle_lib.probe(q, v8)
    return (o["dvds"][7] / np.float64(2.0)) / np.float64(p.k0)


def _eqlin_psi(tab, R, Z):
    """GetPsi of eqdsk_utilities_m.f90:144-162 (bilinear; Psi(nr, nz) in Fortran order, PSIAXIS subtracted)"""
    rg, zg, psi = tab["r_grid"], tab["z_grid"], np.asarray(tab["lin_psi"])
    nr = len(rg)
    hr, hz = rg[1] - rg[0], zg[1] - zg[0]
    i, j = 1 + int((R - rg[0]) / hr), 1 + int((Z - zg[0]) / hz)
    x, y = (R - rg[i - 1]) / hr, (Z - zg[j - 1]) / hz
    at = lambda a, b: psi[(a - 1) + (b - 1) * nr]
    omx, omy = 1.0 - x, 1.0 - y
    return ((at(i, j) * omx * omy + at(i + 1, j) * x * omy) + at(i, j + 1) * omx * y) + at(i + 1, j + 1) * x * y


def psi_expected(p, tab, v):
    """psiN of the host restatement in rays_amd/ray_init.py (pinned by the launcher fixtures); the bilinear eqdsk model,
    which the host launcher does not restate, from GetPsi above"""
    if p.equilib_model == 0:
        return 0.0
    if p.equilib_model == 1 or p.axisym.magnetics_model == 1:
        return _host_fields(p, v[:3])[3]["psiN"] if p.equilib_model == 1 else _solmag_psiN(p, v)
    x, y, z = (float(t) for t in v[:3])
    if p.axisym.magnetics_model == 2:
        return _eqlin_psi(tab, math.sqrt(x * x + y * y), z) / p.axisym.psiB
    err, b, ns, extra = _axisym_fields(p, v[:3], tab)
    assert err in (0, 24, 13), err
    return extra["psiN"]


def _solmag_psiN(p, v):
    """'solovev_magnetics' under axisym_toroid: _host_fields' Solovev branch on the same parameter block (it reads
    p.solovev, where the magnetics namelist travels)"""
    q = copy_params(p)
    q.equilib_model = 1
    return _host_fields(q, v[:3])[3]["psiN"]


def expected_at_points(p, tab, v, resid, stride=1):
    """All nineteen fields at the states v[n][nv] (every `stride`-th is evaluated; the rest stay NaN) from the oracle's
    probe: {name: array[n]}"""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    out = {name: np.full(n, np.nan) for name in FIELDS}
    q = _probe_params(p)
    for i in range(0, n, stride):
        v8 = np.concatenate([v[i, :7], [0.0]])[:q.nv]
        o = oracle_lib.probe(q, v8)
        e = from_eq_record(p, v[i], o["eq"], resid[i])
        e["n_imag"] = (o["dvds"][7] / np.float64(2.0)) / np.float64(p.k0) if p.damping_model else np.float64(0.0)
        e["Psi"] = psi_expected(p, tab, v[i])
        for name in FIELDS:
            out[name][i] = e[name]
    return out
