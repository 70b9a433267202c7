"""Reader for the raw dumps written by oracle/ref_dump_driver.f90 (test infrastructure)."""
from __future__ import annotations

import numpy as np

MAGIC = 0x52415953


def read_dump(path: str) -> dict:
    b = open(path, "rb").read()
    hdr = np.frombuffer(b, dtype="<i4", count=8)
    assert int(hdr[0]) == MAGIC and int(hdr[1]) == 2, hdr
    nray, nv, nstep_max, nspec, probe_stride = (int(x) for x in hdr[2:7])
    off = 32
    out = dict(nray=nray, nv=nv, nstep_max=nstep_max, nspec=nspec)

    def take(dtype, count, shape=None):
        nonlocal off
        a = np.frombuffer(b, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a.reshape(shape) if shape else a

    sc = take("<f8", 8)
    for k, v in zip(("omgrf", "k0", "clight", "eps0", "ds", "s_max", "dispersion_resid_limit",
                     "trace_wall_s"), sc):
        out[k] = float(v)
    for k in ("qs", "ms", "n0s", "t0s", "eta"):
        out[k] = take("<f8", 6).copy()
    sol = take("<f8", 6)
    out["solovev"] = dict(zip(("rmaj", "kappa", "bphi0", "iota0", "outer_bound", "psiB"),
                              (float(x) for x in sol)))
    out["rvec0"] = take("<f8", 3 * nray, (nray, 3)).copy()
    out["rindex_vec0"] = take("<f8", 3 * nray, (nray, 3)).copy()
    out["npoints"] = take("<i4", nray).copy()
    flags = take("S60", nray)
    out["stop_flag"] = [f.decode().rstrip() for f in flags]
    npt = nstep_max + 1
    out["ray_vec"] = take("<f8", nv * npt * nray, (nray, npt, nv))
    out["residual"] = take("<f8", npt * nray, (nray, npt))
    out["end_ray_vec"] = take("<f8", nv * nray, (nray, nv)).copy()
    if probe_stride > 0:
        nprobe = int(take("<i4", 1)[0])
        neq = 28 + 12 * (nspec + 1)
        rec = np.dtype([("iray", "<i4"), ("j", "<i4"), ("v", "<f8", (nv,)), ("eq", "<f8", (neq,)),
                        ("cold", "<f8", (7,)), ("num", "<f8", (7,)), ("dvds", "<f8", (nv,)),
                        ("resid", "<f8")])
        out["probes"] = np.frombuffer(b, dtype=rec, count=nprobe, offset=off).copy()
        off += rec.itemsize * nprobe
    assert off == len(b), (off, len(b))
    return out


STATES_MAGIC = 0x52485353


def write_states(path: str, v, s):
    """The input of oracle/ref_states_driver.f90: int32 n, nv, then (s, v(1:nv)) per state."""
    v = np.ascontiguousarray(v, dtype="<f8")
    n, nv = v.shape
    rows = np.concatenate([np.asarray(s, dtype="<f8").reshape(n, 1), v], axis=1)
    with open(path, "wb") as f:
        f.write(np.array([n, nv], dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(rows).tobytes())


def read_states(path: str):
    """What oracle/ref_states_driver.f90 wrote: (probe records, step records or None).  Probe records carry the fields of
    read_dump's `probes` (without iray / j) plus the flag texts equilibrium, eqn_ray and check_save left and the
    stop_ode each of the two set; step records v1, resid, the flags and stop_ode of ode_solver and of the check_save
    behind it, and the flag equilibrium leaves at v1."""
    b = open(path, "rb").read()
    magic, n, nv, nspec, rk4 = (int(x) for x in np.frombuffer(b, dtype="<i4", count=5))
    assert magic == STATES_MAGIC, hex(magic)
    neq = 28 + 12 * (nspec + 1)
    probe = [("v", "<f8", (nv,)), ("eq_flag", "S60"), ("eq", "<f8", (neq,)), ("cold", "<f8", (7,)), ("num", "<f8", (7,)),
             ("dvds", "<f8", (nv,)), ("resid", "<f8"), ("rhs_flag", "S30"), ("rhs_stop", "<i4"), ("cs_flag", "S30"),
             ("cs_stop", "<i4"), ("num_undef", "<i4")]
    step = [("v1", "<f8", (nv,)), ("resid1", "<f8"), ("step_flag", "S30"), ("step_stop", "<i4"), ("cs1_flag", "S30"),
            ("cs1_stop", "<i4"), ("step_num_undef", "<i4"), ("eq1_flag", "S60")]
    rec = np.dtype(probe + (step if rk4 else []))
    assert 20 + rec.itemsize * n == len(b), (n, rec.itemsize, len(b))
    a = np.frombuffer(b, dtype=rec, count=n, offset=20)
    pr = np.zeros(n, dtype=np.dtype(probe))
    for name, kind, *_ in probe:
        pr[name] = np.char.rstrip(a[name]) if kind[0] == "S" else a[name]     # (Fortran pads with blanks)
    if not rk4:
        return pr, None
    st = np.zeros(n, dtype=np.dtype(step))
    for name, kind, *_ in step:
        st[name] = np.char.rstrip(a[name]) if kind[0] == "S" else a[name]
    return pr, st


def defined_masks(probe, step, numerical, geom):
    """Which parts of a state's records are facts of the reference (boolean arrays by name):
      flags   the flag equilibrium left (and eqn_ray's, which repeats it)          -- not where geom == 2
      values  eq, cold, resid and check_save's flag and stop_ode                   -- equilibrium returned no error, geom == 0
      num     deriv_num's result                   -- values, and none of the six points it displaces r to is refused
      rhs     dvds and the flag eqn_ray left       -- values (and num, where the configuration integrates with deriv_num)
      step    v1 and the flag ode_solver left      -- flags, geom == 0 (and no stage state with a refused displaced point)
      step_cs resid and flags of the check_save behind the step -- step, no stage refused, equilibrium accepts v1
    Where equilibrium returns with an error the reference stores no eq_point (equilibrium_m.f90:198-202): what the
    routines then compute with is what the state before left behind.  geom marks the states at which the reference
    reads a variable it never set or memory outside an array (tests/rhs_state_cases.py: reference_undefined)."""
    flags = geom != 2
    values = (probe["eq_flag"] == b"") & (geom == 0)
    num = values & (probe["num_undef"] == 0)
    rhs = num if numerical else values
    st = flags & (geom == 0) & (step["step_num_undef"] == 0)
    st_cs = st & (step["step_stop"] == 0) & (step["eq1_flag"] == b"")
    return dict(flags=flags, values=values, num=num, rhs=rhs, step=st, step_cs=st_cs)


def blank_undefined(probe, step, numerical, geom):
    """The records with everything that is no fact of the reference (defined_masks) zeroed: flags '', stop_ode -1."""
    probe, step = probe.copy(), step.copy()
    m = defined_masks(probe, step, numerical, geom)
    for k in ("eq", "cold", "resid"):
        probe[k][~m["values"]] = 0.0
    probe["cs_flag"][~m["values"]], probe["cs_stop"][~m["values"]] = b"", -1
    probe["num"][~m["num"]] = 0.0
    probe["dvds"][~m["rhs"]] = 0.0
    no_rhs_flag = ~(m["rhs"] | (m["flags"] & (probe["eq_flag"] != b"")))
    probe["rhs_flag"][no_rhs_flag], probe["rhs_stop"][no_rhs_flag] = b"", -1
    probe["eq_flag"][~m["flags"]] = b"?"
    step["v1"][~m["step"]] = 0.0
    step["step_flag"][~m["step"]], step["step_stop"][~m["step"]] = b"", -1
    step["resid1"][~m["step_cs"]], step["cs1_flag"][~m["step_cs"]], step["cs1_stop"][~m["step_cs"]] = 0.0, b"", -1
    step["eq1_flag"][~m["step"]] = b""
    return probe, step


def read_axisym_tables(path: str) -> dict:
    """Spline tables written by ref_dump_driver.f90 (RAYS_DUMP_AXISYM)."""
    b = open(path, "rb").read()
    nr, nz, n_rb, n_ne, n_te, n_ti = (int(x) for x in np.frombuffer(b, dtype="<i4", count=6))
    off = 24
    sc = np.frombuffer(b, dtype="<f8", count=6, offset=off)
    off += 48
    out = dict(zip(("box_rmin", "box_rmax", "box_zmin", "box_zmax", "plasma_psi_limit", "psiB"),
                   (float(x) for x in sc)))

    def take(n):
        nonlocal off
        a = np.frombuffer(b, dtype="<f8", count=n, offset=off).copy()
        off += 8 * n
        return a

    if n_rb == -1:   # 'eqdsk_magnetics_lin_interp': eqdsk_utilities_m's dR, dZ, R_grid, Z_grid, Psi(nr, nz), T(nr)
        out["lin_dR"], out["lin_dZ"] = (float(v) for v in take(2))
        out["r_grid"], out["z_grid"] = take(nr), take(nz)
        out["lin_psi"] = take(nr * nz)            # Psi(nr, nz) Fortran order, PSIAXIS subtracted
        out["lin_t"] = take(nr)
    else:
        out["r_grid"], out["z_grid"] = take(nr), take(nz)
        out["psi_fspl"] = take(16 * nr * nz)          # fspl(4,4,nr,nz) Fortran order
        out["rb_grid"], out["rb_fspl"] = take(n_rb), take(4 * n_rb)
    for key, n in (("ne", n_ne), ("te", n_te), ("ti", n_ti)):
        if n:
            out[key + "_grid"], out[key + "_fspl"] = take(n), take(4 * n)
    assert off == len(b), (off, len(b))
    return out


def read_deposition(path: str) -> dict:
    """Deposition profiles written by ref_dump_driver.f90 (RAYS_DUMP_DEPOSITION): the reference's
    post_process_lib/deposition_profiles_m applied to the run's ray_results_m arrays."""
    b = open(path, "rb").read()
    n_prof, n_bins, nray = (int(x) for x in np.frombuffer(b, dtype="<i4", count=3))
    off = 12

    def take(n):
        nonlocal off
        a = np.frombuffer(b, dtype="<f8", count=n, offset=off).copy()
        off += 8 * n
        return a

    out = dict(n_bins=n_bins, power=take(nray), names=[], work=[], profile=[], q_sum=[])
    n_rho = int(np.frombuffer(b, dtype="<i4", count=1, offset=off)[0])
    off += 4
    if n_rho:
        out["rho_grid"], out["rho_fspl"] = take(n_rho), take(4 * n_rho)
    for _ in range(n_prof):
        out["names"].append(b[off:off + 20].decode().strip())
        off += 20
        take(2)  # grid_min, grid_max
        out["work"].append(take(n_bins * nray).reshape(nray, n_bins))   # work(n_bins, nray)
    for _ in range(n_prof):
        out["profile"].append(take(n_bins))
        out["q_sum"].append(float(take(1)[0]))
    assert off == len(b), (off, len(b))
    return out
