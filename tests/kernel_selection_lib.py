"""Which kernel the C ABI names for every request: the table tests/test_cpu_kernel_selection.py compares with
tests/golden/kernel_selection.json.  No device is needed: without one find_kernel (rays_capi.hip) takes 256 compute
units, so a fan counts as two waves per SIMD from 131072 rays on.

    python -m tests.kernel_selection_lib tests/golden/kernel_selection.json     (re)writes the table

The file holds a table of strings (kernel names and refusal messages) and, per request, either the indices of the five
names asked for + the step loop, or the index of the message rays_hip_check_params refused it with."""
import ctypes as C
import glob
import itertools
import json
import os
import sys

from rays_amd import hip
from rays_amd.namelist import read_namelist
from rays_amd.params import AXI_N, SLAB_N, SOLOVEV_N, copy_params, params_from_namelist
from rays_amd.trace import load_axisym_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("RAYS_HIP_SG_GROUP", "RAYS_HIP_FORCE_WAVES_PER_SIMD")

NRAYS = (0, 1, 131071, 131072, 1048576)
NUMERICS = ("exact", "tolerance")
SG_GROUP = (None, "0")
FORCE_WAVES = (None, "1", "2")
# the requests made for every configuration, in the order of its list in the table
CONFIG_REQUESTS = list(itertools.product(NRAYS, NUMERICS, SG_GROUP, FORCE_WAVES))

# the synthetic sweep: one fixture's parameters per equilibrium, the five switches of a kernel group overridden, with
# every row count nv they allow (damping x integrate_eq_gradients) and every species count
SWEEP_BASE = {0: "cfg1_slab16_rk4.in", 1: "cfg2_solovev1024_rk4.in", 2: "gold_axisym64_solmag_damp_rk4.in"}
# (solver, derivative, unit exponents, multi_spec_damping, damping, integrate_eq_gradients)
SWEEP_SWITCHES = [s for s in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)) if s[4] or not s[3]]
SWEEP_REQUESTS = list(itertools.product((1, 2, 3, 4, 5, 6), (1, 1048576), NUMERICS))


def load_config(path):
    nml = read_namelist(path)
    return params_from_namelist(nml, load_axisym_tables(path, nml))


def loadable_configs():
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*.in"))):
        try:
            out[os.path.basename(path)] = load_config(path)
        except Exception:   # not a run's namelist (an eqdsk generator's input, a launcher-only file)
            pass
    return out


def sweep_params(base, solver, deriv, unit_exp, multi_spec, damping, grad, ns):
    """base's equilibrium with the group switches set: parabolic density and temperature profiles whose exponents are 1
    (unit_exp) or 2, nspec = ns - 1 species that repeat the first ion, and the nv that goes with the rows asked for."""
    p = copy_params(base)
    p.ode_solver, p.ray_deriv, p.multi_spec_damping = solver, deriv, multi_spec
    p.damping_model, p.integrate_eq_gradients, p.nspec = damping, grad, ns - 1
    p.nv = 7 + damping + (ns if multi_spec else 0) + 5 * grad
    e = {0: p.slab, 1: p.solovev, 2: p.axisym}[p.equilib_model]
    e.alphan1 = e.alphan2 = 1.0 if unit_exp else 2.0
    # the models under which unit_exponents (rays_dev_params.inc) reads the exponents: 'parabolic' in each equilibrium
    if p.equilib_model == 0:
        e.dens_prof_model = SLAB_N["parabolic"]
    elif p.equilib_model == 1:
        e.dens_prof_model = SOLOVEV_N["parabolic"]
    else:
        e.density_prof_model = AXI_N["parabolic"]
    for i in range(1, ns):
        for a in (p.qs, p.ms, p.n0s, p.t0s, p.eta, e.t_prof_model):
            a[i] = a[min(i, base.nspec)]
    return p


class Table:
    def __init__(self, lib=None):
        self.lib = lib or hip.load()
        self.strings = [""]

    def index(self, s):
        if s not in self.strings:
            self.strings.append(s)
        return self.strings.index(s)

    def ask(self, p, nray):
        """[recording, summary-only, fused deposition, continuation recording, continuation summary-only, step loop],
        or [refusal message]."""
        lib, ref = self.lib, C.byref(p)
        if lib.rays_hip_check_params(ref):
            return [self.index(hip.last_error())]
        names = [lib.rays_hip_kernel_name_for(ref, nray), lib.rays_hip_summary_kernel_name_for(ref, nray),
                 lib.rays_hip_deposition_kernel_name_for(ref, nray), lib.rays_hip_window_kernel_name_for(ref, nray, 1),
                 lib.rays_hip_window_kernel_name_for(ref, nray, 0)]
        return [self.index(n.decode()) for n in names] + [lib.rays_hip_rk4_loop_for(ref, nray)]


def requests(table, p, reqs):
    """The answers to reqs = [(nray, numerics[, RAYS_HIP_SG_GROUP, RAYS_HIP_FORCE_WAVES_PER_SIMD])] for p."""
    out = []
    for nray, numerics, *env in reqs:
        hip.set_numerics(numerics)
        for k, v in zip(ENV, env or (None, None)):
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        out.append(table.ask(p, nray))
    return out


def selection_table():
    saved = {k: os.environ.get(k) for k in ENV}
    numerics = hip.get_numerics()
    try:
        t = Table()
        configs = loadable_configs()
        out = {"configs": {name: requests(t, p, CONFIG_REQUESTS) for name, p in configs.items()}, "sweep": {}}
        for eq, name in SWEEP_BASE.items():
            for sw in SWEEP_SWITCHES:
                rows = []
                for (ns, nray, num) in SWEEP_REQUESTS:
                    rows += requests(t, sweep_params(configs[name], *sw, ns), [(nray, num)])
                out["sweep"]["%d_%s" % (eq, "".join(map(str, sw)))] = rows
        out["strings"] = t.strings
        return out
    finally:
        hip.set_numerics(numerics)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(selection_table(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
