"""CPU tier of the deposition binner (rays_amd/csrc/rays_deposition.hpp: deposit_ray + the ray-ordered profile sum).

tests/golden/deposition_binner_cases.npz holds synthetic rays (tests/deposition_cases.py) and what the REFERENCE's
binner_real made of them (oracle/_ref/ref_binner), on four grids at six bin counts: every branch of the binner, which
the four traced deposition fixtures do not reach.  Compared here, bit for bit: a plain restatement of the reference's
statements (tests/deposition_ref.py), the product source compiled for the host (tests/emul_lib.py), and the product
source as a stand-alone program under AddressSanitizer + UBSan with exactly sized rows.  The GPU tier
(tests/test_gpu_deposition_binner.py) runs the same cases through the kernels."""
import os
import subprocess

import numpy as np
import pytest

from tests import deposition_cases as dc
from tests import deposition_ref as dr
from tests import emul_lib
from tests.common import ROOT, load_golden

FIXTURE = os.path.join(ROOT, "tests", "golden", "deposition_binner_cases.npz")
EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")


@pytest.fixture(scope="module")
def z():
    f = np.load(FIXTURE, allow_pickle=False)
    return {k: f[k] for k in f.files}


def combos(z):
    return [(ig, float(lo), float(hi), int(nb)) for ig, (lo, hi) in enumerate(z["grids"]) for nb in z["n_bins"]]


def assert_bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, msg
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    assert not len(bad), f"{msg}: {len(bad)} elements differ, first at {bad[0]}: {a[tuple(bad[0])]!r} != {b[tuple(bad[0])]!r}"


def test_fixture_inputs_are_what_the_generator_makes(z):
    assert [tuple(g) for g in z["grids"]] == list(dc.GRIDS) and list(z["n_bins"]) == list(dc.N_BINS)
    assert str(z["families"]) == dc.FAMILIES and len(z["npoints"]) == dc.NRAY <= 48 and z["Q"].shape[1] == dc.NPT <= 12
    for ig, lo, hi, nb in combos(z):
        x, q, npts = dc.cases(lo, hi, nb)
        assert_bits(x, z["x_" + dc.key(ig, nb)])
        assert_bits(q, z["Q"])
        np.testing.assert_array_equal(npts, z["npoints"])
    for a, b in zip(dc.edge_cases(), (z["edge_grid"], z["edge_n_bins"], z["edge_x"], z["edge_Q"], z["edge_npoints"])):
        np.testing.assert_array_equal(a, b)
    assert sorted(set(z["npoints"][[i for i, f in enumerate(dc.FAMILIES) if f == "h"]])) == [0, 1, 2]


def test_fixture_reaches_every_branch_of_the_binner(z):
    """Counted from the inputs, with the reference's own comparisons: what the slab fixture has none of."""
    for ig, lo, hi, nb in combos(z):
        w = (hi - lo) / nb
        n = dict.fromkeys(("one_bin", "two_bins", "middle_fill", "clip_low", "clip_high", "clip_both", "outside", "tiny",
                           "descending", "repeated", "touch_xmin", "touch_xmax", "both_on_xmax", "dropped", "negative_dQ"), 0)
        for x, q, npt in zip(z["x_" + dc.key(ig, nb)], z["Q"], z["npoints"]):
            assert not dc.has_undefined_segment(x[:npt], lo, hi, nb)    # the reference is undefined there
            for i in range(1, npt):
                xl, xh, dq = min(x[i - 1], x[i]), max(x[i - 1], x[i]), q[i] - q[i - 1]
                n["descending"] += x[i] < x[i - 1]
                n["repeated"] += x[i] == x[i - 1] and dq != 0
                n["negative_dQ"] += dq < 0
                if abs(dq) < 4 * dc.TINY:
                    n["tiny"] += 1
                    continue
                if xh < lo or xl > hi:
                    n["outside"] += 1
                    continue
                n["touch_xmin"] += xh == lo and xl < lo
                n["touch_xmax"] += xl == hi and xh > hi
                n["both_on_xmax"] += xl == hi == xh
                n["clip_low"] += xl < lo
                n["clip_high"] += xh > hi
                n["clip_both"] += xl < lo and xh > hi
                il = 1 if xl < lo else int(np.floor((xl - lo) / w)) + 1
                ih = nb if xh >= hi else int(np.floor((xh - lo) / w)) + 1
                n["one_bin"] += ih == il
                n["two_bins"] += ih == il + 1
                n["middle_fill"] += ih > il + 1
                n["dropped"] += ih < il
        always = set(n) - {"two_bins", "middle_fill"}
        want = always | ({"two_bins"} if nb >= 2 else set()) | ({"middle_fill"} if nb >= 3 else set())
        missing = [k for k in sorted(want) if not n[k]]
        assert not missing, (lo, hi, nb, missing, n)
        ierr = set(z["ierr_" + dc.key(ig, nb)].tolist())
        assert ierr == {0, 1, 2}


def test_restatement_equals_the_reference_on_every_case(z):
    for ig, lo, hi, nb in combos(z):
        rows, ierrs = z["rows_" + dc.key(ig, nb)], z["ierr_" + dc.key(ig, nb)]
        assert rows.shape == (dc.NRAY, nb) and np.isfinite(rows).all()
        for i, npt in enumerate(z["npoints"]):
            x, q = z["x_" + dc.key(ig, nb)][i, :npt], z["Q"][i, :npt]
            for guard in (True, False):    # no case of this set needs the guard
                row, ierr = dr.bin_ray(x, q, lo, hi, nb, guard=guard)
                assert_bits(row, rows[i], f"grid {ig} n_bins {nb} ray {i} ({dc.FAMILIES[i]})")
                assert ierr == ierrs[i]


def test_restatement_equals_the_slab_fixture():
    """the traced fixture of 'Ptotal_x': dep_work and dep_profile of the reference post-processor"""
    g, nml, p = load_golden("gold_slab16_damp_rk4")
    rv = g["dep_ray_vec_full"]
    nb = int(g["dep_n_bins"])
    work = np.stack([dr.bin_ray(rv[i, :n, 0], rv[i, :n, 7] * g["dep_power"][i], p.slab.xmin, p.slab.xmax, nb)[0]
                     for i, n in enumerate(g["npoints_full"])])
    assert_bits(work, g["dep_work"][0])
    assert_bits(dr.profile_sum(work), g["dep_profile"][0])


def test_product_source_on_host_equals_the_reference_on_every_case(z):
    none, none4 = np.zeros(1), np.zeros(4)
    for ig, lo, hi, nb in combos(z):
        p = dc.slab_params(lo, hi)
        rv = dc.ray_vec_of(z["x_" + dc.key(ig, nb)], z["Q"], p.nv)
        work, prof = emul_lib.deposition(p, 2, nb, rv, z["npoints"], np.ones(dc.NRAY), none, none4)
        assert_bits(work, z["rows_" + dc.key(ig, nb)], f"grid {ig} n_bins {nb}")
        assert_bits(prof, dr.profile_sum(z["rows_" + dc.key(ig, nb)]))


def test_reference_binner_against_exact_arithmetic(z):
    """The reference itself, on the interior families a, b and e: every bin within 2**-30 * sum |delta_Q| (over the
    segments touching the bin) of delta_Q times the exact overlap fraction of segment and bin, computed with
    fractions.Fraction from the same float inputs.  The bound is derived: each real-number index carries at most 3
    roundings on a magnitude of at most 320, so a delta_ix >= 2**-10 is good to about 2**-32 relative; 4 is the margin.
    Measured maximum of |float - exact| / sum |delta_Q| over all 24 (grid, n_bins): 2**-44.1."""
    from fractions import Fraction as F
    worst = 0.0
    for ig, lo, hi, nb in combos(z):
        w = (hi - lo) / nb
        for i, npt in enumerate(z["npoints"]):
            if dc.FAMILIES[i] not in "abe":
                continue
            x, q = z["x_" + dc.key(ig, nb)][i, :npt], z["Q"][i, :npt]
            dix = np.abs(np.diff((x - lo) / w))
            assert ((dix == 0) | (dix >= 2.0 ** -10)).all() and (x >= lo).all() and (x <= hi).all()
            exact, touched = dr.exact_bins(x, q, lo, hi, nb)
            for b in range(nb):
                err = abs(F(float(z["rows_" + dc.key(ig, nb)][i, b])) - exact[b])
                assert err <= touched[b] / 2 ** 30, (ig, nb, i, b, float(err), float(touched[b]))
                if touched[b]:
                    worst = max(worst, float(err / touched[b]))
    print(f"reference binner vs exact arithmetic: max |float - exact| / sum|delta_Q| = 2**{np.log2(worst):.1f}")
    assert worst > 0


FAN_GRID, FAN_BINS = 2, 100   # the non-dyadic grid at the reference's default bin count


def fan_work(z, nray):
    x, q, npts, pw = dc.tiled_fan(z, FAN_GRID, FAN_BINS, nray)
    lo, hi = z["grids"][FAN_GRID]
    return np.stack([dr.bin_ray(x[i, :n], q[i, :n] * pw[i], lo, hi, FAN_BINS)[0] for i, n in enumerate(npts)])


def test_fan_rows_are_the_reference_rows_times_the_power(z):
    """a power of two scales a ray's row exactly (family f apart: its subnormal steps do not scale)"""
    work = fan_work(z, 130)
    pw = dc.fan_powers(130)
    assert np.log10(np.abs(pw).max() / np.abs(pw).min()) >= 15.9 and (pw > 0).any() and (pw < 0).any()
    rows = z["rows_" + dc.key(FAN_GRID, FAN_BINS)]
    for i in range(130):
        if dc.FAMILIES[i % dc.NRAY] != "f":
            assert_bits(work[i], rows[i % dc.NRAY] * pw[i] + 0.0, f"ray {i}")   # (+ 0.0: an empty bin is +0.0)


def test_ordered_sum_data_is_order_sensitive(z):
    """The profile of the GPU tier's fans depends on the order of the sum: the ray-ordered running sum differs from
    the reversed one and from numpy's pairwise sum, so a kernel that reduced in any tree order would be caught."""
    for nray in (63, 64, 65, 513, 1100):
        work = fan_work(z, nray)
        seq = dr.profile_sum(work)
        assert (seq != dr.profile_sum(work[::-1])).any(), nray
        assert (seq != np.sum(np.ascontiguousarray(work.T), axis=1)).any(), nray   # (pairwise along the contiguous axis)
        # ... and from the sum taken in the kernel's 64-ray chunks, each reduced on its own first
        chunks = np.stack([dr.profile_sum(work[i:i + 64]) for i in range(0, nray, 64)])
        if nray > 128:
            assert (seq != dr.profile_sum(chunks)).any(), nray
    # continuing from a carry is the same running sum
    work = fan_work(z, 1100)
    for cut in (1, 512, 513, 1099):
        assert_bits(dr.profile_sum(work[cut:], dr.profile_sum(work[:cut])), dr.profile_sum(work))


# ---- the update one element past the row -------------------------------------------------

def test_undefined_edge_list_is_what_it_says(z):
    edges = dc.edge_list_of_fixture(z)
    assert len(edges) >= 8
    for lo, hi, nb, x, q in edges:
        assert dc.has_undefined_segment(x, lo, hi, nb)
        with pytest.raises(IndexError, match=rf"binned_Q\({nb + 1}\)"):   # the reference's statements, unguarded
            dr.bin_ray(x, q, lo, hi, nb, guard=False)
        row, _ = dr.bin_ray(x, q, lo, hi, nb)
        assert np.isfinite(row).all() and row.any()


def build_sanitized_binner():
    """tests/hip_emul/emul_deposition_main.cpp + the product header under ASan + UBSan, the sanitizer runtimes linked
    into the executable"""
    exe = os.path.join(EMUL_DIR, "emul_deposition_san")
    srcs = [os.path.join(EMUL_DIR, "emul_deposition_main.cpp"), os.path.join(EMUL_DIR, "hip", "hip_runtime.h")]
    srcs += [os.path.join(ROOT, "rays_amd", "csrc", f) for f in
             ("rays_deposition.hpp", "rays_device.hpp", "rays_device_arith.inc", "rays_libm.hpp", "rays_libm_tables.inc")]
    srcs.append(os.path.join(ROOT, "include", "rays_hip.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                               "-static-libasan", "-static-libubsan", "-I", EMUL_DIR, srcs[0], "-o", exe])
    return exe


def test_sanitized_binner_is_clean_and_equals_the_reference(z, tmp_path):
    """Every case, the undefined-edge list included, binned into a heap row of exactly n_bins doubles under
    AddressSanitizer + UBSan in a child process: no report, a clean exit, and the rows of the reference (the guarded
    restatement for the undefined-edge list).  Without the guard in deposit_ray the first undefined-edge case ends this
    with a heap-buffer-overflow report."""
    exe = build_sanitized_binner()
    cases, edges = dc.case_list_of_fixture(z), dc.edge_list_of_fixture(z)
    dc.write_case_file(str(tmp_path / "cases.bin"), cases + edges)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"
    r = subprocess.run([exe, "cases.bin", "rows.bin"], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows, _ = dc.read_result_file(str(tmp_path / "rows.bin"), cases + edges)
    i = 0
    for ig, lo, hi, nb in combos(z):
        assert_bits(np.stack(rows[i:i + dc.NRAY]), z["rows_" + dc.key(ig, nb)], f"grid {ig} n_bins {nb}")
        i += dc.NRAY
    for (lo, hi, nb, x, q), row in zip(edges, rows[i:]):
        assert_bits(row, dr.bin_ray(x, q, lo, hi, nb)[0], f"undefined-edge case [{lo}, {hi}] n_bins {nb}")


def test_product_source_on_host_equals_the_guarded_restatement_on_the_undefined_edges(z):
    none, none4 = np.zeros(1), np.zeros(4)
    for lo, hi, nb, x, q in dc.edge_list_of_fixture(z):
        p = dc.slab_params(lo, hi)
        xs, qs = np.zeros((2, dc.NPT)), np.zeros((2, dc.NPT))     # + an empty ray behind it: the row past the first one
        xs[0, :len(x)], qs[0, :len(x)] = x, q
        work, _ = emul_lib.deposition(p, 2, nb, dc.ray_vec_of(xs, qs, p.nv), np.array([len(x), 0], dtype=np.int32),
                                      np.ones(2), none, none4)
        assert_bits(work[0], dr.bin_ray(x, q, lo, hi, nb)[0])
        assert not work[1].any()
