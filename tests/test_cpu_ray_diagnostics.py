"""CPU tier of the per-point ray diagnostics (include/rays_hip.h: rays_hip_ray_diagnostics): the product's diag_point
(rays_amd/csrc/rays_diag.hpp) compiled for the host (tests/hip_emul/emul_diag.cpp) against the reference's own probe
records, the oracle and the host restatements, bit for bit; the file writer; the Fortran binding."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rays_amd import hip, results
from rays_amd.params import copy_params
from tests import diag_expect as dx
from tests.common import GOLDEN_CASES, ROOT, load_golden


def _tab(g):
    return {k[4:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("axi_")}


def _load(name):
    g, nml, p = load_golden(name)
    tab = _tab(g)
    dx.emul_set_tables(tab)
    return g, p, tab


def _with_probes():
    out = []
    for name in GOLDEN_CASES:
        with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False) as g:
            if "probes" in g.files:
                out.append(name)
    return out


PROBED = _with_probes()


def _at_states(p, v, resid, fields=None):
    """the emulated diagnostics at n independent states: n one-point rays"""
    n = len(v)
    d, bad = dx.emul_diagnostics(p, v.reshape(n, 1, p.nv), np.asarray(resid).reshape(n, 1), np.ones(n, dtype=np.int32), fields)
    return {k: a[:, 0] for k, a in d.items()}, bad


def test_there_are_probed_fixtures():
    assert len(PROBED) >= 3


@pytest.mark.parametrize("name", PROBED)
def test_fields_equal_the_references_eq_records(name):
    """1: NE, MODB, ALPHA_E, GAMMA_E, TE_KEV bit-equal to the reference binary's eq record at every probe state;
    N_PAR, N_PERP, XI_0..2, R bit-equal to the formulae on the reference's eq values in the written order."""
    g, p, tab = _load(name)
    pr = g["probes"]
    got, bad = _at_states(p, pr["v"], pr["resid"])
    assert not bad.any()
    for i, rec in enumerate(pr):
        want = dx.from_eq_record(p, rec["v"], rec["eq"], rec["resid"])
        for key in ("ne", "modB", "alpha_e", "gamma_e", "Te_kev", "n_par", "n_perp", "xi_0", "xi_1", "xi_2", "R",
                    "s", "X", "Y", "Z", "P_absorbed", "residual"):
            dx.assert_bits(got[key][i], want[key], f"{name} probe {i} {key}")


DAMPED = [n for n in GOLDEN_CASES if "damp" in n]


@pytest.mark.parametrize("name", DAMPED)
def test_n_imag_equals_the_oracles_ray_equation(name):
    """2: N_IMAG bit-equal to (dvds(8)/2)/k0 of the oracle's eqn_ray with nv = 8, arcl, v(8) = 0, at every 7th recorded
    point (and at the probes where the fixture has them)."""
    g, p, tab = _load(name)
    assert p.damping_model
    npts = g["npoints"]
    v = np.concatenate([g["ray_vec"][r, :n:7] for r, n in enumerate(npts)])
    if "probes" in g.files:
        v = np.concatenate([v, g["probes"]["v"]])
    got, bad = _at_states(p, v, np.zeros(len(v)), ("n_imag",))
    assert not bad.any()
    want = np.array([dx.n_imag_expected(p, x) for x in v])
    assert np.count_nonzero(want) > 0, "no damped point among the sampled ones"
    dx.assert_bits(got["n_imag"], want, name)


@pytest.mark.parametrize("name", ["gold_axisym64_eqdsk_damp_rk4", "gold_axisym64_solmag_damp_rk4",
                                  "gold_axisym64_eqlin_damp_rk4", "gold_solovev64_damp_rk4", "cfg1_slab16_rk4"])
def test_psi_equals_the_host_restatement(name):
    """3: PSI bit-equal to psiN of rays_amd/ray_init.py's fields, one fixture per magnetics model + a Solovev
    equilibrium; 0 for the slab."""
    g, p, tab = _load(name)
    npts = g["npoints"]
    v = np.concatenate([g["ray_vec"][r, :n:5] for r, n in enumerate(npts)])
    got, _ = _at_states(p, v, np.zeros(len(v)), ("Psi",))
    want = np.array([dx.psi_expected(p, tab, x) for x in v])
    dx.assert_bits(got["Psi"], want, name)
    assert (want != 0).any() == (p.equilib_model != 0)


def _padded(g, p, extra=3):
    """the fixture's arrays with `extra` unrecorded slots behind the longest ray"""
    rv, res = g["ray_vec"], g["residual"]
    npt = rv.shape[1] + extra
    a, b = np.zeros((rv.shape[0], npt, p.nv)), np.zeros((rv.shape[0], npt))
    a[:, :rv.shape[1]], b[:, :rv.shape[1]] = rv, res
    return a, b, g["npoints"].astype(np.int32)


@pytest.mark.parametrize("name", ["gold_axisym64_eqdsk_damp_rk4", "gold_slab16_fast_rk4", "gold_solovev64_sg_cold"])
def test_field_selection_and_padding(name):
    """4: any subset of fields gives the values of the full set; slots past npoints are +0.0; without damping
    N_IMAG = P_ABSORBED = 0; with the electrons' t_prof_model = zero XI_* = TE_KEV = 0."""
    g, p, tab = _load(name)
    rv, res, npts = _padded(g, p)
    full, bad = dx.emul_diagnostics(p, rv, res, npts)
    assert set(full) == set(hip.DIAG_FIELDS) and not bad.any()
    live = np.arange(rv.shape[1])[None, :] < npts[:, None]
    for k, a in full.items():
        assert not a[~live].view(np.uint64).any(), f"{k}: a slot past npoints is not +0.0"
    for sel in (("n_imag",), ("s", "residual"), ("Psi", "R", "Z"), ("xi_1", "ne"), ("n_par", "P_absorbed", "X"),
                hip.DIAG_FIELDS[::2], hip.DIAG_FIELDS[1::2]):
        part, _ = dx.emul_diagnostics(p, rv, res, npts, sel)
        assert set(part) == set(sel)
        for k in sel:
            dx.assert_bits(part[k], full[k], f"{name} {k} selected as {sel}")
    if not p.damping_model:
        assert not full["n_imag"].any() and not full["P_absorbed"].any()
    else:
        assert full["n_imag"].any() and full["P_absorbed"].any()
    if name == "gold_solovev64_sg_cold":
        for k in ("xi_0", "xi_1", "xi_2", "Te_kev"):
            assert not full[k].any(), k
    assert np.array_equal(full["s"][live], rv[..., 6][live]) and np.array_equal(full["residual"], res * live)


def test_unknown_field_is_refused():
    with pytest.raises(ValueError, match="unknown"):
        hip.diag_field_mask(("s", "nope"))
    assert hip.diag_field_mask(None)[0] == (1 << 19) - 1
    assert hip.diag_field_mask(("residual", "s")) == ((1 << 18) | 1, ("s", "residual"))


@pytest.mark.parametrize("slab", [False, True])
def test_write_ray_diagnostics_NC(tmp_path, slab):
    """5: the file read back with scipy: dimensions, variable names in order, shapes, values."""
    from scipy.io import netcdf_file

    name = "gold_slab16_damp_rk4" if slab else "gold_axisym64_eqdsk_damp_rk4"
    g, p, tab = _load(name)
    rv, res, npts = _padded(g, p)
    diag, _ = dx.emul_diagnostics(p, rv, res, npts)
    assert results.ray_diagnostics_file_name(" lbl ", slab) == ("ray_detailed_diagnostics_slab.lbl.nc" if slab else
                                                               "ray_detailed_diagnostics.lbl.nc")
    path = str(tmp_path / results.ray_diagnostics_file_name("lbl", slab))
    date = [2024, 5, 6, -240, 7, 8, 9, 10]
    results.write_ray_diagnostics_NC(path, diag, npts, p.nv, run_label="lbl", date_vector=date, slab=slab)
    coords = ["X", "Y", "Z"] if slab else ["Psi", "R", "Z"]
    order = ["date_vector", "npoints", "s", "ne", "Te_kev", "modB", "alpha_e", "gamma_e"] + coords + \
            ["n_par", "n_perp", "P_absorbed", "n_imag", "xi_0", "xi_1", "xi_2", "residual"]
    maxnp = int(npts.max())
    with netcdf_file(path, "r", mmap=False) as f:
        assert list(f.dimensions.items()) == [("number_of_rays", len(npts)), ("max_number_of_points", maxnp),
                                              ("dim_v_vector", p.nv), ("d8", 8)]
        assert list(f.variables) == order
        lab = f.RAYS_run_label
        assert (lab.decode() if isinstance(lab, bytes) else str(lab)).strip() == "lbl"
        assert np.array_equal(f.variables["date_vector"].data, date)
        assert np.array_equal(f.variables["npoints"].data, npts)
        for k in order[2:]:
            var = f.variables[k]
            assert var.dimensions == ("number_of_rays", "max_number_of_points") and var.data.dtype == np.dtype(">f8")
            assert var.data.shape == (len(npts), maxnp)
            dx.assert_bits(np.array(var.data, dtype=np.float64), diag[k][:, :maxnp], k)
    with pytest.raises(ValueError, match="not in"):
        results.write_ray_diagnostics_NC(path, {"s": diag["s"]}, npts, p.nv)


def test_fortran_binding_compiles(tmp_path):
    """6: amdflang -c fortran/rays_hip_m.f90 fortran/ray_diagnostics_hip.f90"""
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no amdflang on this machine")
    for src in ("rays_hip_m.f90", "ray_diagnostics_hip.f90"):
        subprocess.check_call([fc, "-O2", "-c", os.path.join(ROOT, "fortran", src), "-o", str(tmp_path / (src + ".o"))],
                              cwd=str(tmp_path))
    assert (tmp_path / "ray_diagnostics_hip_m.mod").exists()
