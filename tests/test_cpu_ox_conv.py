"""CPU tier of the O-X conversion analysis (rays_amd/csrc/rays_oxconv.hpp; include/rays_hip.h: rays_hip_ox_conv*): the
product's device functions and both kernels compiled for the host (tests/hip_emul/emul_oxconv.cpp: the scan kernel on
the wave emulator, with its ballots, shuffles and the carried lane 63) against tests/golden/ox_conv_cases.npz -- the
reference's own eq_point records and the module's formulae (tests/ox_conv_expect.py) -- bit for bit on every case and
every field; the compiler facts the restatement rests on (norm2, minval); the list-directed writer; the Fortran binding;
and one-token changes to the device code, each of which has to fail.

1. the emulated analysis equals the fixture on every case, in both input layouts, the host finish included
2. the scan kernel on the wave emulator: S.synthetic and S.capped tiled over several blocks with a ragged last one
3. norm2 and minval as the reference's compiler evaluates them: a program of ours, compiled here (skips without amdflang)
4. the expected records rebuilt with the C oracle's equilibrium are the fixture's (the oracle is pinned to the reference)
5. the committed fixture is what the committed generator produces (where oracle/_ref exists)
6. results.write_OX_conversion_data_LD
7. the Fortran binding and fortran/ox_conv_analysis_hip.f90 compile (skips without amdflang)
8. one-token changes"""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from rays_amd import hip, results
from tests import emul_build as eb
from tests import oracle_lib
from tests import ox_conv_expect as ox
from tests.common import ROOT, host_libm_is_the_variant_the_fixtures_were_cut_with

CASES = ox.case_names()


def _case(name):
    fx = ox.load_fixture(name)
    p, tab = ox.load_params(name)
    q, rv, npts = ox.padded(p, fx)
    return fx, q, rv, npts, tab


def _compare(name, lib=None, layouts=(False, True), what="emulated"):
    """test 1's comparison; conv_coeff and the converted list where the host libm is the fixtures'"""
    fx, q, rv, npts, tab = _case(name)
    libm = host_libm_is_the_variant_the_fixtures_were_cut_with()
    for use_packed in layouts:
        got = ox.emul_ox_conv(q, rv, npts, host_finish=True, use_packed=use_packed, lib=lib, tab=tab)
        tag = f"{what}, {name}, {'packed' if use_packed else 'padded'}"
        ox.assert_records(got, fx, tag, conv="exact" if libm else None)
        for k in ox.INT_FIELDS:                                     # no sentinel survives
            assert (got[k] != -77).all(), (tag, k)
        for k in ox.FLOAT_FIELDS:
            if k != "conv_coeff":
                keep = (fx["status"] & ox.EQ_REFUSED) == 0
                assert ox.same_bits(np.isnan(got[k][keep]), np.isnan(fx[k][keep])), (tag, k)
        if libm:
            assert np.array_equal(got["converted"], fx["converted"]), (tag, got["converted"], fx["converted"])
        refused = (fx["status"] & ox.EQ_REFUSED) != 0
        for k in ox.INT_FIELDS[1:] + ox.FLOAT_FIELDS:               # a refused ray holds its bit and zeros
            assert not np.asarray(got[k])[refused].any(), (tag, k)


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_emulated_analysis_equals_the_fixture(name):
    _compare(name)


def test_fixture_holds_what_the_cases_are_for():
    """the figures the issue chose the slab cases for, and the events of S.synthetic (the generator asserts them when it
    cuts the fixture; here on the committed file)"""
    a, b = ox.load_fixture("T.slab_ox"), ox.load_fixture("T.slab_x")
    assert len(a["status"]) == 48 and ((a["status"] & 3) == 3).all() and len(a["converted"]) == 31
    assert a["step_number"].min() == 124 and a["step_number"].max() == 187
    assert int(((a["step_number"] == 128)).sum()) >= 1, "the deciding pair 128 | 129 straddles a chunk edge"
    assert set(a["iterations"].tolist()) <= {3, 4} and (b["iterations"] == 8).all() and len(b["converted"]) == 31
    for name in CASES:
        fx = ox.load_fixture(name)
        both = (fx["status"] & 3) == 3
        assert not (np.abs(fx["conv_coeff"][both] / ox.THRESHOLD - 1.0) < 1e-6).any(), name
        assert fx["ray_vec"].shape[1] <= 253 and len(fx["status"]) <= 64, name
        if name.startswith("T."):
            assert 4 * both.sum() >= len(both) and ((fx["status"] & 4) != 0).sum() >= 3 and \
                (both & ((fx["status"] & 4) == 0)).sum() >= 3 and not (fx["status"] & ox.EQ_REFUSED).any(), name
    for name in ("T.curved_solovev", "T.curved_axisym"):             # the first decrease on both sides of point 64
        s = ox.load_fixture(name)["step_number"]
        assert s.min() < 64 <= s.max(), (name, s.min(), s.max())
    assert os.path.getsize(os.path.join(ROOT, ox.FIXTURE)) < 1_000_000


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,copies", [("S.synthetic", 3), ("S.capped", 35)])
def test_scan_kernel_on_the_wave_emulator(name, copies):
    """the rays repeated: 66 | 70 rays = 17 | 18 scan blocks of four waves with a ragged last block, two ascent blocks
    with a ragged last wave; every copy gives the expected record"""
    fx, q, rv, npts, tab = _case(name)
    got = ox.emul_ox_conv(q, np.tile(rv, (copies, 1, 1)), np.tile(npts, copies), host_finish=False, tab=tab)
    want = {k: np.tile(fx[k], (copies,) + (1,) * (fx[k].ndim - 1)) for k in ox.INT_FIELDS + ox.FLOAT_FIELDS}
    ox.assert_records(got, want, f"{name} x {copies}", conv=None)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _amdflang():
    return shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)


def test_norm2_and_minval_as_the_compiler_evaluates_them(tmp_path):
    """tests/fortran/norm2_minval_probe.f90 (ours), compiled with the reference build's flags: norm2 of a 3-element
    section of a derived type's component, norm2 and minval of a 2-element constructor -- the forms the module uses --
    against ox.norm2 / ox.minval2 on 1e5 random vectors and every triple of a set of extreme values."""
    import itertools
    fc = _amdflang()
    if fc is None:
        pytest.skip("no amdflang on this machine")
    exe = str(tmp_path / "probe")
    subprocess.check_call([fc, "-O2", "-fopenmp", "-ffp-contract=off", "-w", os.path.join(ROOT, "tests", "fortran", "norm2_minval_probe.f90"),
                           "-o", exe], cwd=str(tmp_path))
    rng = np.random.default_rng(20261021)
    v = rng.standard_normal((100000, 3)) * 10.0 ** rng.integers(-6, 7, (100000, 3))
    extreme = [0.0, -0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-200, 1e200, -1e200, 1.7976931348623157e308, float("inf"),
               float("nan"), 1.0, 3.0, 4.0]
    v = np.concatenate([v, np.array(list(itertools.product(extreme, repeat=3)))])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(v)) + v.astype("<f8").tobytes())
    subprocess.check_call([exe, "in.bin", "out.bin"], cwd=str(tmp_path))
    got = np.fromfile(tmp_path / "out.bin", dtype="<f8").reshape(len(v), 3)
    with np.errstate(all="ignore"):
        want = np.array([[ox.norm2(t), ox.norm2(t[:2]), ox.minval2(float(t[0]), 0.25 * float(t[1]))] for t in v])
    for k, what in enumerate(("norm2 of three", "norm2 of two", "minval of two")):
        same = (got[:, k].view(np.uint64) == want[:, k].view(np.uint64)) | (np.isnan(got[:, k]) & np.isnan(want[:, k]))
        assert same.all(), f"{what}: {int((~same).sum())} differ; first: {v[np.argmin(same)].tolist()} -> " \
                           f"{got[np.argmin(same), k]!r}, restated {want[np.argmin(same), k]!r}"


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_expected_records_rebuilt_with_the_oracle(name):
    """tests/ox_conv_expect.py on the C oracle's eq_point records (pinned to the reference's by tests/test_cpu_oracle.py
    and the state fixtures) gives the fixture's records: the fixture can be checked where oracle/_ref is absent."""
    if not host_libm_is_the_variant_the_fixtures_were_cut_with():
        pytest.skip("the host libm is not the variant the fixtures were cut with")
    fx, q, rv, npts, tab = _case(name)

    def eq_at(x, k):
        bad, eqs = [], []
        for xi, ki in zip(x, k):
            v = np.zeros(q.nv)
            v[0:3], v[3:6] = xi, ki
            o = oracle_lib.probe(q, v)
            bad.append(int(o["codes"][0]) != 0)
            eqs.append(o["eq"])
        return np.array(bad), np.array(eqs)

    alpha, refused = np.zeros(fx["alpha"].shape), np.zeros(fx["alpha"].shape, dtype=bool)
    for r in range(len(npts)):
        bad, eqs = eq_at(rv[r, :npts[r], 0:3], rv[r, :npts[r], 3:6])
        for j in range(npts[r]):
            refused[r, j] = bad[j]
            alpha[r, j] = 0.0 if bad[j] else ox.eq_fields(eqs[j])["alpha0"]
    assert np.array_equal(refused, fx["refused"]) and ox.same_bits(alpha, fx["alpha"])
    rec = ox.expected_records(q.k0, rv, npts, alpha, refused, eq_at)
    ox.assert_records(rec, fx, f"oracle-built records, {name}")
    assert np.array_equal(rec["converted"], fx["converted"]) and ox.same_bits(rec["exponent"], fx["exponent"])


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_states")),
                    reason="oracle/_ref/ref_states not built (no reference tree here)")
def test_committed_fixture_is_what_the_generator_produces():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_ox_conv_cases.py"), "--check"],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_list_directed_writer(tmp_path):
    """write_OX_conversion_data_LD on T.slab_ox: one record group per converted ray, the loop index, values that read
    back to the same binary64, a leading blank and at most 79 columns per record, items in the reference's order."""
    fx = ox.load_fixture("T.slab_ox")
    fields = {k: fx[k] for k in ox.INT_FIELDS + ox.FLOAT_FIELDS}
    fields.update(number_of_rays_converted=len(fx["converted"]), converted_ray_number=fx["converted"])
    oxc = results.OXConversion.from_fields(fields)
    path = str(tmp_path / results.ox_conversion_file_name("gsd"))
    assert path.endswith("OX_conv_data.gsd.dat")
    results.write_OX_conversion_data_LD(path, oxc)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and all(l.startswith(" ") and len(l) <= 79 for l in lines[:-1])
    rec = results.read_OX_conversion_data_LD(path)
    assert [r["index"] for r in rec] == list(range(1, 32))
    for r, ray in zip(rec, fx["converted"]):
        i = int(ray) - 1
        want = (fx["conv_coeff"][i], ox.norm2(fx["nvecz_c"][i]), ox.norm2(fx["nvecy_c"][i]))
        assert ox.same_bits([r["conv_coeff"], r["nz_c"], r["ny_c"]], want), (ray, r, want)
    first = " ".join(lines[:2]).split()
    assert first[:2] == ["ray", "1"] and first[2:5] == ["conv", "coeff", "="] and first[6:8] == ["nz_c", "="] and \
        first[9:11] == ["ny_c", "="], first
    assert lines[0].startswith(" ray  1   conv coeff =  ")      # a blank in front of every item but none between the texts
    for tok in (first[5], first[8], first[11]):                  # reals as write_results_LD writes them
        assert tok == results.ld_real(float(tok.replace("E", "e")))
    # nothing converted: an empty file
    fields.update(number_of_rays_converted=0, converted_ray_number=np.zeros(0, dtype=np.int32))
    results.write_OX_conversion_data_LD(path, results.OXConversion.from_fields(fields))
    assert open(path).read() == ""


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_fortran_files_compile(tmp_path):
    """amdflang -c fortran/rays_hip_m.f90 fortran/ox_conv_analysis_hip.f90"""
    fc = _amdflang()
    if fc is None:
        pytest.skip("no amdflang on this machine")
    for src in ("rays_hip_m.f90", "ox_conv_analysis_hip.f90"):
        subprocess.check_call([fc, "-O2", "-w", "-c", os.path.join(ROOT, "fortran", src), "-o", str(tmp_path / (src + ".o"))],
                              cwd=str(tmp_path))
    assert (tmp_path / "ox_conv_analysis_m.mod").exists()


def test_python_binding_names_the_header():
    """hip.OX_FIELDS is rays_ox_result_t, field for field, and the status bits are the header's"""
    import re
    header = open(os.path.join(ROOT, "include", "rays_hip.h")).read()
    body = re.search(r"typedef struct rays_ox_result_t \{(.*?)\} rays_ox_result_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _, _ in hip.OX_FIELDS]
    bits = dict(re.findall(r"RAYS_OX_(FOUND_MAX|FOUND_CUTOFF|CONVERTED|EQ_REFUSED) = (\d+)", header))
    assert (hip.OX_FOUND_MAX, hip.OX_FOUND_CUTOFF, hip.OX_CONVERTED, hip.OX_EQ_REFUSED) == \
        tuple(int(bits[k]) for k in ("FOUND_MAX", "FOUND_CUTOFF", "CONVERTED", "EQ_REFUSED")) == \
        (ox.FOUND_MAX, ox.FOUND_CUTOFF, ox.CONVERTED, ox.EQ_REFUSED)
    assert hip.OX_CONVERSION_THRESHOLD == ox.THRESHOLD and len(hip.OX_AUX) == dict((f, w) for f, _, w in hip.OX_FIELDS)["aux"]


# ---- 8 ------------------------------------------------------------------------------------------------------------------
# (name: old text, new text, occurrences, the case that has to show it, the rays (S.synthetic names) or None)
MUTATIONS = {
    "decrease < -> <=": ("alpha < before;  // :240", "alpha <= before;  // :240", 1, "S.synthetic", "plateau"),
    "carried lane 0 for 63": ("carry = __shfl(alpha, 63);", "carry = __shfl(alpha, 0);", 1, "S.synthetic", "decrease_64_65|decrease_128_129"),
    "minval -> maxval": ("if (b < a || (a != a && b == b)) m = b;", "if (b > a || (a != a && b == b)) m = b;", 1, "T.slab_x", None),
    "abs(nz_c) dropped": ("const double dz = fabs(nz_c) - n_crit,", "const double dz = (nz_c) - n_crit,", 1, "S.synthetic", None),
    "yc for zc": ("fdiv(ox_dot(R.k_max, zc), P.k0);        // :380", "fdiv(ox_dot(R.k_max, yc), P.k0);        // :380", 1, "T.slab_ox", None),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_one_token_changes_are_caught(mutation, tmp_path):
    old, new, count, case, rays = MUTATIONS[mutation]
    out = str(tmp_path / "librays_emul_oxconv_mut.so")
    lib = ox.emul_lib(out, directory=eb.mutated_tree(str(tmp_path / "tree"), "rays_oxconv.hpp", old, new, count))
    if mutation == "abs(nz_c) dropped" and not host_libm_is_the_variant_the_fixtures_were_cut_with():
        pytest.skip("conv_coeff is compared where the host libm is the fixtures'")
    with pytest.raises(AssertionError) as e:
        _compare(case, lib=lib, layouts=(False,), what="mutated")
    if rays:                                   # the rays that own the event show it first
        fx = ox.load_fixture(case)
        names = [str(n) for n in fx["names"]]
        import re
        m = re.search(r"rays? \[?(\d+)", str(e.value))
        assert m and re.search(rays, names[int(m.group(1))]), (str(e.value), rays)


def test_tolerance_comparison_is_unheld(tmp_path):
    """`<=` -> `<` on abs(alpha - 1) <= 1e-4 (both places): no state of the fixture sits on the tolerance itself, so the
    change is NOT caught -- asserted, so that this is known rather than assumed."""
    out = str(tmp_path / "librays_emul_oxconv_mut.so")
    lib = ox.emul_lib(out, directory=eb.mutated_tree(str(tmp_path / "tree"), "rays_oxconv.hpp", "<= kOxAlphaTol", "< kOxAlphaTol", 2))
    for name in CASES:
        _compare(name, lib=lib, layouts=(False,), what="tolerance < for <=")
