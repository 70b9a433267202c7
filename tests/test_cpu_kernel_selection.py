"""CPU tier: the kernel the C ABI names for a request -- recording, summary-only, fused deposition, continuation
(recording and not) and the RK4 step loop -- for every configuration, fan size, numerics setting and developer switch,
and for a synthetic sweep that reaches each of the 48 kernel groups at every species count, equals
tests/golden/kernel_selection.json, the table the library gave before its objects registered themselves
(tests/kernel_selection_lib.py writes it).  No device: find_kernel takes 256 compute units without one."""
import json
import os
import re
import subprocess
import sys

import pytest

from rays_amd import hip
from tests import kernel_selection_lib as ks
from tests.common import ROOT

EMUL = os.path.join(ROOT, "tests", "hip_emul")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "kernel_selection.json")) as f:
        return json.load(f)


def _text(table, row):
    s = table["strings"]
    return ["refused: " + s[row[0]]] if len(row) == 1 else [s[i] for i in row[:5]] + [row[5]]


def test_every_request_gets_the_kernel_it_got_before(golden):
    got = ks.selection_table()
    assert sorted(got["configs"]) == sorted(golden["configs"])
    assert sorted(got["sweep"]) == sorted(golden["sweep"]) and len(got["sweep"]) == 3 * len(ks.SWEEP_SWITCHES)
    for part, reqs in (("configs", ks.CONFIG_REQUESTS), ("sweep", ks.SWEEP_REQUESTS)):
        for key, rows in golden[part].items():
            assert len(rows) == len(got[part][key]) == len(reqs)
            for req, want, have in zip(reqs, rows, got[part][key]):
                assert _text(got, have) == _text(golden, want), (part, key, req)


def test_the_table_reaches_every_build_and_every_branch(golden):
    """At least one name of each of the six builds, a two-waves-per-SIMD kernel, a lane-group kernel and a refusal; every
    one of the 48 groups answers with a kernel for some species count."""
    rows = [r for part in ("configs", "sweep") for rs in golden[part].values() for r in rs]
    names = [_text(golden, r) for r in rows]
    eq = lambda n: int(re.search(r"<(\d+),", n).group(1))
    named = [n for n in names if len(n) == 6]
    assert any(n[0] and not eq(n[0]) & 16 for n in named)           # recording, exact
    assert any(n[0] and eq(n[0]) & 16 for n in named)               # tolerance
    assert any(n[1] and eq(n[1]) & 0xE0 == 32 for n in named)       # summary-only
    assert any(n[2] and eq(n[2]) & 0xE0 == 96 for n in named)       # fused deposition
    assert any(n[3] and eq(n[3]) & 0xE0 == 128 for n in named)      # continuation, recording
    assert any(n[4] and eq(n[4]) & 0xE0 == 160 for n in named)      # continuation, summary-only
    assert any("_w2<" in n[0] for n in named) and any(n[0].startswith("sg_group_kernel<") for n in named)
    assert any(len(n) == 1 and "no kernel built for this configuration" in n[0] for n in names)
    assert any(n[5] == 1 for n in named) and any(n[5] == 0 for n in named) and any(n[5] == -1 for n in named)
    groups = set()
    for key, rs in golden["sweep"].items():
        e, (solver, deriv, ue, ms) = int(key[0]), map(int, key[2:6])
        for r in rs:
            n = _text(golden, r)
            if len(n) == 6:
                bits = eq(n[0])   # the equilibrium, then one bit each for unit exponents and multi_spec_damping
                assert (bits & 3, bits >> 2 & 1, bits >> 3 & 1) == (e, ue, ms), (key, n)
                assert n[0].startswith("sg_" if solver else "rk4_"), (key, n)
                groups.add((solver, e, deriv, ue, ms))
    assert len(groups) == 48


_EMUL_SCRIPT = """
import ctypes as C, json, os, sys
from rays_amd import hip
from tests import kernel_selection_lib as ks
lib, out = hip.load(), {}
for name in ("cfg2_solovev1024_rk4.in", "cfg1_slab16_rk4.in"):
    p = ks.load_config(os.path.join("configs", name))
    rc = lib.rays_hip_check_params(C.byref(p))
    out[name] = [rc, hip.last_error() if rc else ""]
    t = ks.Table(lib)
    row = t.ask(p, 1024)
    if len(row) == 6:
        out[name] += [t.strings[i] for i in row[:5]]
print(json.dumps(out))
"""


def test_emulated_c_abi_refuses_the_groups_it_is_not_linked_with():
    """The emulated C ABI library links three recording groups and nothing else: a configuration of one of them
    resolves, with no kernel of any other build; one of another group is refused with the message of
    rays_hip_check_params, as before.  (In a process of its own: one process loads one C ABI library.)"""
    subprocess.check_call(["make", "-s", "-f", "Makefile.capi", "-j4"], cwd=EMUL)
    env = dict(os.environ, RAYS_HIP_LIB=os.path.join(EMUL, "build_capi", "librays_capi_emul.so"), RAYS_AMD_NO_TORCH="1")
    r = subprocess.run([sys.executable, "-c", _EMUL_SCRIPT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["cfg2_solovev1024_rk4.in"] == [0, "", "rk4_trace_kernel<5, 2, 0, 7>", "", "", "", ""]     # group 0_1_0_1_0
    rc, message = out["cfg1_slab16_rk4.in"]                                                                  # group 0_0_0_1_0
    assert rc != 0 and message == (
        "rays_hip: no kernel built for this configuration (RK4, equilibrium 0, 2 species, cold dD, nv = 7): "
        "the default library holds nspec = 1 plus the fixtures' shapes -- rebuild with "
        "`make -C rays_amd/csrc FULL=1` for every species count")
    hip.check_params(ks.load_config(os.path.join(ROOT, "configs", "cfg1_slab16_rk4.in")))   # (the product library holds it)
