"""Launches for the three device ray launchers (rays_ray_init.hpp / .hip, rays_fan_setup.inc): what the trajectory
fixtures never launch.  TEST INFRASTRUCTURE ONLY.

A case is one existing configs/<base>.in plus a dictionary of namelist overrides {group: {key: value}}; the overridden
namelist is the base's text with the overriding assignments appended to their groups (a later assignment wins, in
the reference's namelist read and in rays_amd/namelist.py alike), so the reference and every implementation under
test read the same text.  The expectation is the reference's own record: oracle/_ref/ref_launch
(oracle/ref_launch_driver.f90: the reference's initialize, then nray, rvec0, rindex_vec0, ray_pwr_wt of ray_init_m)
run on that namelist, collected by generate() into tests/golden/launch_cases.npz.

Classes (DESIGN.md 2a has the table of what each catches):
    A  every wave_mode x both k0_sign on each launcher (and each magnetics model of the axisym one), 8 x 8 fans that
       straddle the mode's cutoff; the species counts the launcher is instantiated for (1, 3, 4, 6)
    B  compaction shapes: 1 .. 1025 candidates at one position (all kept | straddling), a 15 295-candidate Solovev fan
       over 35 positions, slab fans of 256 and 255 members at 12 positions with whole empty blocks at both ends
    C  thresholds: 1 x 16 (or 16 x 1) fans whose step is the spacing of doubles at `arg >= 0` / `discr >= 0`
    D  degenerate launches: the magnetic axis, vacuum inside the box, positions the equilibrium refuses, negative density
    E  nothing survives: the reference stops with a text

Deterministic: no random numbers, no clock.  The starting values of class C were bisected with rays_amd/ray_init.py
(scratch work, any implementation would do) and are written here as hex floats: the generator does not run the code
under test.  With a step of one spacing of doubles, a0 + i*da is exact for all 16 members.

Solovev r loops: the reference sets ray_pwr_wt(count) = 1 after each r loop and nothing else
(solovev_ray_init_nphi_ntheta_m.f90:196; the array is divided by nray at the end, :206), so a loop that ends with no survivor SO FAR writes ray_pwr_wt(0), outside
the array.  No case here has one: wherever an r position of a Solovev case drops everything (class D: the axis, the
vacuum, outside the box), it comes AFTER a position with survivors.  The other entries of ray_pwr_wt are unset in the
reference; the record keeps the indices that were set (`wt_index`) and zero elsewhere."""
from __future__ import annotations

import math
import os
import re
import shutil
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join("tests", "golden", "launch_cases.npz")
REF_LAUNCH = os.path.join(ROOT, "oracle", "_ref", "ref_launch")
STOP_TEXT = "No successful ray initializations"
MAGIC = 0x4C41554E

Case = namedtuple("Case", "name cls base overrides")

SLAB, SOLOVEV, AXISYM = "simple_slab", "solovev", "axisym_toroid_ray_init_R_Z_nphi_ntheta"
GROUP = {SLAB: "simple_slab_ray_init_list", SOLOVEV: "solovev_ray_init_nphi_ktheta_list",
         AXISYM: "axisym_toroid_ray_init_R_Z_nphi_ntheta_list"}
MODES = ("plus", "minus", "fast", "slow")

# the bases: one per launcher and magnetics model, and one per species count the launcher is instantiated for
B_SLAB, B_SOL = "cfg1_slab16_rk4", "cfg2_solovev1024_rk4"
B_AXI = {"eqdsk": "gold_axisym64_eqdsk_damp_rk4", "eqlin": "gold_axisym64_eqlin_damp_rk4",
         "solmag": "gold_axisym64_solmag_damp_rk4"}
B_SPECIES = {1: "gold_slab_ns1_rk4", 3: "gold_slab_shear_gauss_3spec_sg_num", 4: "gold_solovev64_4spec_rk4_num",
             6: "gold_slab_6spec_sg"}


def H(s):
    return float.fromhex(s)


def _launcher_of(base):
    return SLAB if "slab" in base else AXISYM if "axisym" in base else SOLOVEV


def _fan(base, mode=None, sign=None, nray_max=None, eq=None, **kw):
    """overrides: the launcher's group (kw), wave_mode / k0_sign, nray_max, the equilibrium's group (eq = (group, {..}))"""
    o = {GROUP[_launcher_of(base)]: dict(kw)}
    rf = {}
    if mode is not None:
        rf["wave_mode"] = mode
    if sign is not None:
        rf["k0_sign"] = sign
    if rf:
        o["rf_list"] = rf
    if nray_max is not None:
        o["ray_init_list"] = dict(nray_max=nray_max)
    if eq is not None:
        o[eq[0]] = dict(eq[1])
    return o


# fans in (n_y, n_z) | (n_theta, n_phi) that straddle the cutoff of every mode at the bases' launch points (a dimension of
# one member sits in the middle of its range)
def _axis(n, lo, hi):
    return (lo + (hi - lo) / 2.0, 0.0) if n == 1 else (lo, (hi - lo) / (n - 1))


def _slab8(n_y=8, n_z=8, y=(-2.3, 2.3), z=(-1.3, 1.3), **kw):
    (y0, dy), (z0, dz) = _axis(n_y, *y), _axis(n_z, *z)
    return dict(dict(n_x_launch=1, n_ky_launch=n_y, rindex_y0=y0, delta_rindex_y0=dy, n_kz_launch=n_z, rindex_z0=z0,
                     delta_rindex_z0=dz), **kw)


def _tor8(n_t=8, n_p=8, t=(-1.2, 1.2), ph=(-1.3, 1.3), **kw):
    (t0, dt), (p0, dp) = _axis(n_t, *t), _axis(n_p, *ph)
    return dict(dict(n_rindex_theta=n_t, rindex_theta0=t0, delta_rindex_theta=dt, n_rindex_phi=n_p, rindex_phi0=p0,
                     delta_rindex_phi=dp), **kw)


def _torA(**kw):
    """the 8 x 8 window of class A: steps of 0.2 from (-0.45, -0.5), which holds members inside the narrow propagating
    range of the 'minus' root at the axisym bases' launch point (n_perp^2 < 0.08, |n_par| < 0.2) and beyond every cutoff"""
    return _tor8(8, 8, t=(-0.45, 0.95), ph=(-0.5, 0.9), **kw)


def _cases():
    out = []

    def add(name, cls, base, overrides):
        assert name not in {c.name for c in out}, name
        out.append(Case(name, cls, base, overrides))

    # ---- A: modes and sign ----
    for mode in MODES:
        for sign in (1, -1):
            tag = f"{mode}_{'pos' if sign > 0 else 'neg'}"
            add(f"A.slab.{tag}", "A", B_SLAB, _fan(B_SLAB, mode, sign, 100, **_slab8()))
            add(f"A.solovev.{tag}", "A", B_SOL, _fan(B_SOL, mode, sign, **_torA()))
            for mag, base in B_AXI.items():
                add(f"A.axisym_{mag}.{tag}", "A", base, _fan(base, mode, sign, **_torA()))
    for ns, base in B_SPECIES.items():
        for mode, sign in (("fast", -1), ("slow", 1)):
            fan = _slab8() if _launcher_of(base) == SLAB else _torA()
            add(f"A.species{ns}.{mode}_{'pos' if sign > 0 else 'neg'}", "A", base, _fan(base, mode, sign, 100, **fan))

    # ---- B: compaction shapes ----
    # one launch position, n candidates as n_a x n_b: all kept (a narrow fan well inside the propagating range) and
    # straddling the cutoff (the class A ranges)
    shapes = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (1, 257), 511: (7, 73),
              512: (16, 32), 513: (27, 19), 1025: (25, 41)}
    for n, (na, nb) in shapes.items():
        assert na * nb == n
        keep_s = dict(n_x_launch=1, n_ky_launch=na, rindex_y0=-0.1, delta_rindex_y0=0.2 / max(na, 1),
                      n_kz_launch=nb, rindex_z0=0.05, delta_rindex_z0=0.3 / max(nb, 1))
        keep_t = dict(n_rindex_theta=na, rindex_theta0=-0.1, delta_rindex_theta=0.2 / max(na, 1),
                      n_rindex_phi=nb, rindex_phi0=0.05, delta_rindex_phi=0.3 / max(nb, 1))
        add(f"B.slab.n{n}.keep", "B", B_SLAB, _fan(B_SLAB, nray_max=n, **keep_s))
        add(f"B.solovev.n{n}.keep", "B", B_SOL, _fan(B_SOL, nray_max=n, **keep_t))
        if n > 1:
            add(f"B.slab.n{n}.mixed", "B", B_SLAB, _fan(B_SLAB, "fast", nray_max=n, **_slab8(na, nb)))
            add(f"B.solovev.n{n}.mixed", "B", B_SOL, _fan(B_SOL, "plus", nray_max=n, **_tor8(na, nb)))
    # (a single member beyond the cutoff is class E's)
    # the large mixed Solovev fan: 5 x 7 positions of 23 x 19 = 437 members, 15 295 candidates in 60 blocks, launch
    # boundaries inside waves; every r loop has survivors
    big = dict(n_r_launch=5, r_launch0=0.3, dr_launch=-0.075, n_theta_launch=7, theta_launch0=0.0, dtheta_launch=0.9,
               n_rindex_theta=23, rindex_theta0=-1.6, delta_rindex_theta=0.15,
               n_rindex_phi=19, rindex_phi0=-1.5, delta_rindex_phi=0.17)
    for mode in ("minus", "fast"):
        add(f"B.solovev.big.{mode}", "B", B_SOL, _fan(B_SOL, mode, nray_max=15295, **big))
    # slab: 12 x positions of 16 x 16 (and 15 x 17) members; the first three and the last three lie outside xmin..xmax =
    # -0.5..0.5: whole empty blocks at the start and at the end
    for tag, (na, nb) in (("256", (16, 16)), ("255", (15, 17))):
        add(f"B.slab.x12.{tag}", "B", B_SLAB,
            _fan(B_SLAB, "slow", nray_max=12 * na * nb, **_slab8(na, nb, n_x_launch=12, x_launch0=-0.95, dx_launch=0.17)))

    out.extend(_threshold_cases())

    # ---- D: degenerate launches ----
    # the magnetic axis as the LAST r position (r_launch = 0.2, 0.1, 0.0): gradpsi = 0 there, every unit vector NaN
    add("D.solovev.axis", "D", B_SOL, _fan(B_SOL, **_tor8(n_r_launch=3, r_launch0=0.2, dr_launch=-0.1, n_theta_launch=2,
                                                          dtheta_launch=1.5)))
    # vacuum inside the box (outer_bound = 1.4 < R = 1.45 < box_rmax = 1.5: psiN > 1, zero density): R = L = S = P = 1,
    # discr = 0 exactly, plus and minus tie; after a position inside the plasma
    for mode in MODES:
        add(f"D.solovev.vacuum.{mode}", "D", B_SOL,
            _fan(B_SOL, mode, **_tor8(n_r_launch=2, r_launch0=0.35, dr_launch=0.1)))
    # positions the equilibrium refuses: r = 0.35, 0.45 (vacuum), 0.55 (R = 1.55 outside the box)
    add("D.solovev.outside_box", "D", B_SOL, _fan(B_SOL, **_tor8(n_r_launch=3, r_launch0=0.35, dr_launch=0.1)))
    add("D.solovev.outside_box_z", "D", B_SOL,
        _fan(B_SOL, **_tor8(n_r_launch=1, r_launch0=0.35, n_theta_launch=3, theta_launch0=0.0, dtheta_launch=0.7),
             eq=("solovev_eq_list", dict(box_zmax=0.3))))
    add("D.slab.outside_box", "D", B_SLAB, _fan(B_SLAB, nray_max=256, **_slab8(n_x_launch=4, x_launch0=-0.3, dx_launch=0.4)))
    # the axisym box test's 1e-13 margin: R_launch0 next to box_rmax = 1.5 (solovev_magnetics: its own test of the same
    # box has no margin) -- kept where the launch is refused or in the scrape-off plasma; plasma_psi_limit
    for mag, base in B_AXI.items():
        add(f"D.axisym_{mag}.psi_limit", "D", base,
            _fan(base, **_torA(), eq=("axisym_toroid_eq_list", dict(plasma_psi_limit=0.5))))
        add(f"D.axisym_{mag}.beyond_margin", "D", base, _fan(base, **_torA(R_launch0=1.5 + 2e-13)))
        add(f"D.axisym_{mag}.z_beyond_margin", "D", base, _fan(base, **_torA(Z_launch0=-0.7 - 2e-13)))
        add(f"D.axisym_{mag}.inside_psi_limit", "D", base,
            _fan(base, **_torA(R_launch0=1.2), eq=("axisym_toroid_eq_list", dict(plasma_psi_limit=0.5))))
    # NaN n2, n3: the axisym launcher's test `abs(Im(npsi)) > 10*tiny` is false for a NaN, so the reference KEEPS such
    # launches, with NaN index vectors (the slab and Solovev launchers' `Im /= 0.` drops them): the magnetic axis under
    # solovev_magnetics (grad psi = 0: NaN unit vectors), and -- on every magnetics model -- a NaN rindex_theta0
    add("D.axisym_solmag.axis", "D", B_AXI["solmag"], _fan(B_AXI["solmag"], **_torA(R_launch0=1.0)))
    for mag, base in B_AXI.items():
        add(f"D.axisym_{mag}.nan_index", "D", base, _fan(base, **_torA(rindex_theta0=float("nan"))))
    add("D.axisym_eqdsk.within_margin", "D", B_AXI["eqdsk"], _fan(B_AXI["eqdsk"], **_torA(R_launch0=1.5 + 5e-14)))
    # vacuum on the slab: the linear profile 1 + x/Ln is exactly zero at x = -Ln = -0.3; nz = 0.25 .. 2 holds nz = 1
    # exactly, where b = c = discr = 0 and the small root is 0/0 -- the one zero divisor a namelist reaches (NaN in
    # compiler-rt's __divdc3 and in divdc3_re alike)
    for mode in MODES:
        add(f"D.slab.vacuum.{mode}", "D", "gold_slab_negative_dens_rk4",
            _fan("gold_slab_negative_dens_rk4", mode, nray_max=24,
                 **_slab8(3, 8, y=(-0.5, 0.5), z=(0.25, 2.0), x_launch0=-0.3)))
    # negative density: the linear slab profile 1 + x/Ln below x = -Ln = -0.3 (gold_slab_negative_dens_rk4)
    add("D.slab.negative_dens", "D", "gold_slab_negative_dens_rk4",
        _fan("gold_slab_negative_dens_rk4", nray_max=256, **_slab8(n_x_launch=4, x_launch0=-0.45, dx_launch=0.1)))

    # ---- E: nothing survives ----
    # (Solovev: an r loop that ends with no survivor writes ray_pwr_wt(0), see above -- with a fan of 64 the C library
    #  aborts the reference on the damaged heap before it reaches its stop statement; with a single candidate it reaches it)
    add("E.slab", "E", B_SLAB, _fan(B_SLAB, "plus", nray_max=64, **_slab8(z=(2.0, 2.7))))
    add("E.slab.outside", "E", B_SLAB, _fan(B_SLAB, nray_max=64, **_slab8(x_launch0=0.7)))
    add("E.slab.one", "E", B_SLAB, _fan(B_SLAB, "plus", nray_max=1, **_slab8(1, 1, z=(2.0, 2.0))))
    add("E.solovev.one", "E", B_SOL, _fan(B_SOL, nray_max=1, **_tor8(1, 1, ph=(2.0, 2.0))))
    for mag, base in B_AXI.items():
        add(f"E.axisym_{mag}", "E", base, _fan(base, **_tor8(ph=(2.0, 2.7))))
    add("E.axisym_eqdsk.outside", "E", B_AXI["eqdsk"], _fan(B_AXI["eqdsk"], **_torA(R_launch0=1.6)))
    return out


# ---- C: thresholds ----
# (case name, base, mode, which parameter is scanned, the launcher's fixed values, overrides of other groups, the scan's
#  first value as a hex float: 8 spacings of doubles before the crossing the bisection found; the step is the spacing of
#  doubles there)
THRESHOLDS = []


def _thr(launcher, what, scan, fixed, extra, a0_by_mode):
    base = B_SLAB if launcher == "slab" else B_SOL
    for mode in MODES:
        THRESHOLDS.append((f"C.{launcher}.{mode}.{what}", base, mode, scan, fixed, extra, a0_by_mode[mode]))


def _pf_ms(pf, ms):
    return dict(plus=pf, fast=pf, minus=ms, slow=ms)


def _all(a0):
    return dict.fromkeys(MODES, a0)


# slab, x = -0.08 (B along z: n2 = ny, n3 = nz; plus is the fast root there): arg >= 0 along y on both sides and along z
_thr("slab", "arg_y", "y", dict(rindex_z0=0.4), {}, _pf_ms("0x1.257c86d714951p-2", "0x1.e2ba41fd5fbe1p+0"))
_thr("slab", "arg_y_neg", "y", dict(rindex_z0=0.4), {}, _pf_ms("-0x1.257c86d714960p-2", "-0x1.e2ba41fd5fbf0p+0"))
_thr("slab", "arg_z", "z", dict(rindex_y0=0.1), {}, dict(plus="0x1.2db27311c1410p-1", fast="0x1.2db27311c1410p-1",
                                                           minus=None, slow=None))
_thr("slab", "arg_z", "z", dict(rindex_y0=2.0), {}, dict(plus=None, fast=None, minus="0x1.50a0f5498d479p-1",
                                                           slow="0x1.50a0f5498d479p-1"))
# slab, x = 0.02 (just beyond the plasma cutoff, alpha_e > 1): the two roots coalesce at a POSITIVE n_perp^2 near the
# optimal n_par of the O-X conversion, so discr >= 0 alone decides keep / drop, for every mode; along z, and -- with
# by0 = 0.3, where n3 depends on ny -- along y
_thr("slab", "discr_z", "z", dict(rindex_y0=0.0, x_launch0=0.02), {}, _all("0x1.602d6795760e9p-1"))
_thr("slab", "discr_y", "y", dict(rindex_z0=0.6, x_launch0=0.02), {"slab_eq_list": dict(by0=0.3)},
     _all("0x1.efd7c2a820ce9p-2"))
# Solovev, (r, theta) = (0.35, 0): n3 ~ rindex_phi, n2 ~ rindex_theta; the fast / slow assignment changes along phi
_thr("solovev", "arg_theta", "theta", dict(rindex_phi0=0.4), {},
     dict(plus="0x1.b18c55af586a3p-1", slow="0x1.b18c55af586a3p-1", minus="0x1.a8bee4a95b85cp-1", fast="0x1.a8bee4a95b85cp-1"))
_thr("solovev", "arg_theta_neg", "theta", dict(rindex_phi0=0.4), {},
     dict(plus="-0x1.b18c5033b9454p-1", slow="-0x1.b18c5033b9454p-1", minus="-0x1.a8beeb6e074e3p-1",
          fast="-0x1.a8beeb6e074e3p-1"))
_thr("solovev", "arg_phi", "phi", dict(rindex_theta0=0.1), {},
     dict(plus="0x1.e0e9fa6fc432ep-1", minus="0x1.cf2254acb5f09p-1", fast="0x1.e0e9fa6fc432ep-1", slow="0x1.dab2bc82f1054p-1"))
# Solovev with n0 = 1.2e20 at r = 0.17 (alpha_e just above 1): the coalescence at positive n_perp^2 again; along phi,
# and -- with iota0 = 0.3 at theta = 0.8, where n3 depends on rindex_theta -- along theta
_DENSE = {"species_list": dict(n0=1.2e20)}
_thr("solovev", "discr_phi", "phi", dict(rindex_theta0=0.0, r_launch0=0.17), _DENSE, _all("0x1.39ffae2846fe9p-1"))
_thr("solovev", "discr_theta", "theta", dict(rindex_phi0=0.55, r_launch0=0.17, theta_launch0=0.8),
     dict(_DENSE, solovev_eq_list=dict(iota0=0.3)), _all("-0x1.335a1e3780496p-3"))
# the fast / slow choice at a dead tie, fabs(plus) <= fabs(minus) with both sides the same double: b == 0 exactly (the roots
# are +-sqrt(-c/a)) at member 8 of the fan, where sd/(2a) and 2c/sd also round to the same magnitude -- slab, ny = 0
_thr("slab", "tie_z", "z", dict(rindex_y0=0.0, x_launch0=-0.39), {},
     dict(plus=None, minus=None, fast="0x1.4a4640728508cp-1", slow="0x1.4a4640728508cp-1"))
_thr("slab", "tie_z_2", "z", dict(rindex_y0=0.0, x_launch0=-0.375), {},
     dict(plus=None, minus=None, fast="0x1.3d7b6e85a770ep-1", slow="0x1.3d7b6e85a770ep-1"))
THRESHOLDS = [t for t in THRESHOLDS if t[-1] is not None]


def _threshold_cases():
    out = []
    for name, base, mode, scan, fixed, extra, a0 in THRESHOLDS:
        a0 = H(a0)
        step = math.ulp(a0)
        assert all(math.frexp(a0 + i * step)[1] == math.frexp(a0)[1] for i in range(16)), name   # one binade: exact
        slab = _launcher_of(base) == SLAB
        ka = dict(y=("n_ky_launch", "rindex_y0", "delta_rindex_y0"), z=("n_kz_launch", "rindex_z0", "delta_rindex_z0"),
                  theta=("n_rindex_theta", "rindex_theta0", "delta_rindex_theta"),
                  phi=("n_rindex_phi", "rindex_phi0", "delta_rindex_phi"))
        other = {"y": "z", "z": "y", "theta": "phi", "phi": "theta"}[scan]
        kw = dict(fixed)
        kw.update({ka[scan][0]: 16, ka[scan][1]: a0, ka[scan][2]: step, ka[other][0]: 1})
        if slab:
            kw.setdefault("n_x_launch", 1)
        o = _fan(base, mode, nray_max=16, **kw)
        for group, d in extra.items():
            o.setdefault(group, {}).update(d)
        out.append(Case(name, "C", base, o))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
CLASSES = ("A", "B", "C", "D", "E")


def of_class(*classes):
    return [c.name for c in CASES if c.cls in classes]


# ---- the overridden namelist ----
def _fmt(v):
    if isinstance(v, bool):
        return ".true." if v else ".false."
    if isinstance(v, str):
        return "'" + v + "'"
    if isinstance(v, int):
        return str(v)
    return repr(float(v))     # 17 significant digits: read back to the same double


def namelist_text(case):
    """configs/<base>.in with the case's assignments appended to their groups (a group the base lacks is added)"""
    text = open(os.path.join(ROOT, "configs", case.base + ".in")).read()
    for group, kv in case.overrides.items():
        lines = "".join(f" {k} = {_fmt(v)}\n" for k, v in kv.items())
        m = re.search(r"^[ \t]*&" + group + r"[ \t]*$", text, re.I | re.M)
        if m:
            end = re.compile(r"^[ \t]*/[ \t]*$", re.M).search(text, m.end())
            text = text[:end.start()] + lines + text[end.start():]
        else:
            text += f" &{group}\n{lines}/\n"
    return text


def load_case(name):
    """(case, nml, params, fan, nray_max, tables) of a case, with the base's host tables attached to every library"""
    from rays_amd.namelist import parse_namelist
    from rays_amd.params import params_from_namelist
    from rays_amd.ray_init import fan_from_namelist
    from tests.common import load_golden
    case = BY_NAME[name]
    g, _, _ = load_golden(case.base)
    tab = {k[4:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("axi_")}
    nml = parse_namelist(namelist_text(case))
    p = params_from_namelist(nml, tab or None)
    fan, nray_max = fan_from_namelist(nml)
    return case, nml, p, fan, nray_max, (tab or None)


def n_candidates(case):
    from rays_amd.namelist import parse_namelist
    nml = parse_namelist(namelist_text(case))
    model = _launcher_of(case.base)
    g = nml[GROUP[model].lower()]
    gi = lambda k: int(g.get(k, 1))
    if model == SLAB:
        return gi("n_x_launch") * gi("n_y_launch") * gi("n_z_launch") * gi("n_ky_launch") * gi("n_kz_launch")
    return gi("n_r_launch") * gi("n_theta_launch" if model == SOLOVEV else "n_z_launch") * gi("n_rindex_theta") * \
        gi("n_rindex_phi")


# ---- the reference's record of a case ----
def _solovev_marks(nml, rvec0):
    """0-based indices the Solovev launcher sets in ray_pwr_wt: (the survivor count after each r loop) - 1, recomputed
    from the recorded rvec0 (its launch positions are rmaj + r cos(theta), 0, r sin(theta) of the namelist values)."""
    g = nml["solovev_ray_init_nphi_ktheta_list"]
    rmaj = float(nml["solovev_eq_list"]["rmaj"])
    n_r, n_t = int(g.get("n_r_launch", 1)), int(g.get("n_theta_launch", 1))
    pos = {}
    for ir in range(n_r):
        for it in range(n_t):
            theta = float(g.get("theta_launch0", 0.0)) + it * float(g.get("dtheta_launch", 0.0))
            r = float(g.get("r_launch0", 0.0)) + ir * float(g.get("dr_launch", 0.0))
            key = (rmaj + r * math.cos(theta), 0.0, r * math.sin(theta))
            assert pos.setdefault(key, ir) == ir, "two r loops share a launch position"
    loop = np.array([pos[tuple(float(x) for x in row)] for row in rvec0], dtype=np.int64)
    assert (np.diff(loop) >= 0).all()
    counts = [int((loop <= ir).sum()) for ir in range(n_r)]
    assert all(c >= 1 for c in counts), "an r loop ends with no survivor so far: the reference writes ray_pwr_wt(0)"
    return np.array(sorted(set(c - 1 for c in counts)), dtype=np.int32)


def run_reference(case, exe=None):
    """The record of one case: {nray, rvec0, rindex_vec0, ray_pwr_wt, wt_index} or {nray: 0, exit, stop}"""
    from rays_amd.namelist import parse_namelist
    text = namelist_text(case)
    nml = parse_namelist(text)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "rays.in"), "w") as f:
            f.write(text)
        for f in os.listdir(os.path.join(ROOT, "configs")):
            if f.endswith(".geqdsk"):
                shutil.copy(os.path.join(ROOT, "configs", f), d)
        env = dict(os.environ, RAYS_LAUNCH_OUT="launch.bin", OMP_NUM_THREADS="1")
        run = subprocess.run([exe or REF_LAUNCH], cwd=d, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                             text=True, timeout=600)
        path = os.path.join(d, "launch.bin")
        if not os.path.exists(path):
            lines = [x.strip() for x in run.stderr.splitlines() if STOP_TEXT in x]
            assert lines, f"{case.name}: the reference ended (exit status {run.returncode}) without a fan: {run.stderr[-400:]}"
            stop = re.sub(r"^(Fortran )?STOP:?\s*", "", lines[-1])     # (the runtime's own prefix is not the reference's text)
            return dict(nray=np.int32(0), exit=np.int32(run.returncode), stop=np.array(stop))
        assert run.returncode == 0, (case.name, run.returncode, run.stderr[-400:])
        raw = open(path, "rb").read()
    magic, nray = np.frombuffer(raw, dtype="<i4", count=2)
    assert magic == MAGIC and len(raw) == 8 + 8 * 7 * nray, case.name
    body = np.frombuffer(raw, dtype="<f8", offset=8)
    rvec0, rindex_vec0, w = body[:3 * nray].reshape(nray, 3), body[3 * nray:6 * nray].reshape(nray, 3), body[6 * nray:]
    if _launcher_of(case.base) == SOLOVEV:
        idx = _solovev_marks(nml, rvec0)
        blank = np.zeros(nray)
        blank[idx] = w[idx]
        w = blank
    else:
        idx = np.arange(nray, dtype=np.int32)
    return dict(nray=np.int32(nray), rvec0=rvec0.copy(), rindex_vec0=rindex_vec0.copy(), ray_pwr_wt=np.array(w),
                wt_index=idx)


def generate(out_root, exe=None):
    out = {"cases": np.array([c.name for c in CASES])}
    total = 0
    for c in CASES:
        assert 0 < n_candidates(c), c.name
        for k, v in run_reference(c, exe).items():
            out[c.name + ":" + k] = v
        total += int(out[c.name + ":nray"])
    path = os.path.join(out_root, FIXTURE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"launch_cases: {len(CASES)} cases, {total} rays -> {os.path.getsize(path) / 1e3:.0f} kB")


_fixture = None


def load_fixture(name):
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, FIXTURE), allow_pickle=False)
    pre = name + ":"
    return {k[len(pre):]: _fixture[k] for k in _fixture.files if k.startswith(pre)}


# ---- comparison: bit for bit, NaN equal to NaN, no tolerance ----
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _first_bad(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    same = ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).reshape(len(a), -1).all(axis=1)
    bad = np.flatnonzero(~same)
    return (int(bad[0]), len(bad)) if len(bad) else None


def compare_fan(name, rec, rvec0, rindex_vec0, ray_pwr_wt, what):
    """An implementation's fan against the reference's record of the case: count, order, values, weights"""
    want = int(rec["nray"])
    assert want > 0, f"{name}: the reference launched nothing"
    assert len(rvec0) == want and len(rindex_vec0) == want, \
        f"{what}, {name}: {len(rvec0)} rays, the reference launched {want}"
    for key, got in (("rvec0", rvec0), ("rindex_vec0", rindex_vec0)):
        bad = _first_bad(got, rec[key])
        assert bad is None, (f"{what}, {name}: {key} differs from the reference at ray {bad[0]} ({bad[1]} rays in all): "
                             f"got {np.asarray(got)[bad[0]]!r}, want {rec[key][bad[0]]!r}")
    if ray_pwr_wt is not None:
        i = rec["wt_index"]
        assert len(ray_pwr_wt) == want
        bad = _first_bad(np.asarray(ray_pwr_wt)[i], rec["ray_pwr_wt"][i])
        assert bad is None, (f"{what}, {name}: ray_pwr_wt differs from the reference at ray {int(i[bad[0]])}: got "
                             f"{np.asarray(ray_pwr_wt)[i][bad[0]]!r}, want {rec['ray_pwr_wt'][i][bad[0]]!r}")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    generate(ROOT)
