#!/usr/bin/env python3
"""Generate tests/golden/ox_conv_cases.npz: the cases of tests/ox_conv_expect.py and the expected records of the O-X
conversion analysis, from the REFERENCE binaries (oracle/build_ref.sh):

  - the rays of a T case are the reference's own trace of the case's namelist (oracle/_ref/rays_ref_dump), those of an
    S case are hand-made (tests/ox_conv_expect.py: build_synthetic);
  - every equilibrium value is the reference's: oracle/_ref/ref_states (oracle/ref_states_driver.f90: the reference's
    `equilibrium` at states read from a file) is run once on all recorded points for the alpha records, and once per
    ascent iteration on the iterates of all rays still under way;
  - the formulae of post_process_lib/OX_conv_analysis_m.f90 are those of tests/ox_conv_expect.py.

Per case the fixture stores the namelist text (the parameters), the rays clipped to one chunk of the scan kernel past the
first decrease (step_number + 66 points, npoints clipped alike), the alpha records and the expected result arrays.

    python tests/golden/make_ox_conv_cases.py            (re)generate
    python tests/golden/make_ox_conv_cases.py --check    regenerate into a scratch directory and compare bit for bit
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import ox_conv_expect as ox  # noqa: E402
from tests.golden.make_golden import REF, REF_STATES, same_bits  # noqa: E402
from tests.refdump import read_dump, read_states, write_states  # noqa: E402


def _workdir(d, text):
    with open(os.path.join(d, "rays.in"), "w") as f:
        f.write(text)
    for f in os.listdir(os.path.join(ROOT, "configs")):
        if f.endswith(".geqdsk"):
            shutil.copy(os.path.join(ROOT, "configs", f), d)


def reference_trace(text):
    """(ray_vec[nray][npt][nv], npoints) of the reference's own trace of a namelist"""
    with tempfile.TemporaryDirectory() as d:
        _workdir(d, text)
        env = dict(os.environ, RAYS_DUMP_FILE="dump.bin", RAYS_DUMP_PROBE="0", OMP_NUM_THREADS="1")
        subprocess.run([REF], cwd=d, env=env, check=True, stdout=subprocess.DEVNULL)
        ref = read_dump(os.path.join(d, "dump.bin"))
    return np.array(ref["ray_vec"]), np.array(ref["npoints"], dtype=np.int32)


def reference_equilibrium(text, v):
    """(refused[n], eq[n][neq]) of the reference's equilibrium at the states v[n][nv]"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    if not len(v):
        return np.zeros(0, dtype=bool), np.zeros((0, 0))
    with tempfile.TemporaryDirectory() as d:
        _workdir(d, text)
        write_states(os.path.join(d, "states.bin"), v, np.zeros(len(v)))
        env = dict(os.environ, RAYS_STATES_IN="states.bin", RAYS_STATES_OUT="records.bin", OMP_NUM_THREADS="1")
        run = subprocess.run([REF_STATES], cwd=d, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        assert run.returncode == 0, f"the reference stopped (exit status {run.returncode}): drop or move a state"
        probe, _ = read_states(os.path.join(d, "records.bin"))
    assert len(probe) == len(v) and same_bits(probe["v"], v)
    return probe["eq_flag"] != b"", np.array(probe["eq"])


def case_record(case):
    from rays_amd.namelist import parse_namelist
    from rays_amd.params import params_from_namelist
    from tests.common import load_golden
    text = ox.namelist_text(case)
    g, _, _ = load_golden(case.base)
    tab = {k[4:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("axi_")}
    p = params_from_namelist(parse_namelist(text), tab or None)
    nv = p.nv
    out = dict(namelist=np.array(text))

    def state_rows(x, k):
        v = np.zeros((len(x), nv))
        v[:, 0:3], v[:, 3:6] = x, k
        return v

    if case.cls == "T":
        ray_vec, npoints = reference_trace(text)
    else:
        k_row = p.k0 * np.array([0.3, 0.02, -0.6])
        _, eq0 = reference_equilibrium(text, state_rows(np.zeros((1, 3)), k_row[None, :]))
        alpha0 = ox.eq_fields(eq0[0])["alpha0"]
        x_cutoff = float(p.slab.Ln_scale) * (1.0 / alpha0 - 1.0)        # alpha = alpha0 (1 + x/Ln)
        names, ray_vec, npoints = ox.build_synthetic(p, k_row, x_cutoff, capped=case.name == "S.capped")
        out["names"] = np.array(names)
    nray, npt = ray_vec.shape[:2]
    # the alpha records: the reference's equilibrium at every recorded point
    idx = [(r, j) for r in range(nray) for j in range(int(npoints[r]))]
    bad, eqs = reference_equilibrium(text, np.array([ray_vec[r, j] for r, j in idx]).reshape(len(idx), nv))
    alpha, refused = np.zeros((nray, npt)), np.zeros((nray, npt), dtype=bool)
    for n, (r, j) in enumerate(idx):
        refused[r, j] = bad[n]
        alpha[r, j] = 0.0 if bad[n] else ox.eq_fields(eqs[n])["alpha0"]   # (a refused point's record is undefined)
    rec = ox.expected_records(p.k0, ray_vec, npoints, alpha, refused,
                              lambda x, k: reference_equilibrium(text, state_rows(x, k)))
    # clip to one chunk past the first decrease
    keep = np.array([min(int(npoints[r]), int(rec["step_number"][r]) + ox.CHUNK + 2) if rec["status"][r] & ox.FOUND_MAX
                     else int(npoints[r]) for r in range(nray)], dtype=np.int32)
    width = max(int(keep.max()) if nray else 1, 1)
    rv = np.zeros((nray, width, nv))
    al, rf = np.zeros((nray, width)), np.zeros((nray, width), dtype=bool)
    for r in range(nray):
        rv[r, :keep[r]], al[r, :keep[r]], rf[r, :keep[r]] = ray_vec[r, :keep[r]], alpha[r, :keep[r]], refused[r, :keep[r]]
    out.update(ray_vec=rv, npoints=keep, alpha=al, refused=rf)
    out.update(rec)
    return out


def check_conditions(records):
    """The generator's assertions: conditions the cases have to meet, not measurements."""
    n_refused_S = n_S = 0
    for name, rec in records.items():
        st = rec["status"]
        both = (st & (ox.FOUND_MAX | ox.FOUND_CUTOFF)) == (ox.FOUND_MAX | ox.FOUND_CUTOFF)
        conv = (st & ox.CONVERTED) != 0
        c = rec["conv_coeff"][both]
        assert not (np.abs(c / ox.THRESHOLD - 1.0) < 1e-6).any(), f"{name}: a coefficient within 1e-6 of the threshold"
        if name.startswith("T."):
            assert 4 * int(both.sum()) >= len(st), f"{name}: fewer than a quarter of the rays have a maximum and a cutoff"
            assert int(conv.sum()) >= 3 and int((both & ~conv).sum()) >= 3, \
                f"{name}: {int(conv.sum())} converted, {int((both & ~conv).sum())} not: three of each are needed"
            assert not (st & ox.EQ_REFUSED).any(), f"{name}: a refused ray in a traced case"
        else:
            n_S += len(st)
            n_refused_S += int(((st & ox.EQ_REFUSED) != 0).sum())
    assert 10 * n_refused_S <= n_S, f"S: {n_refused_S} of {n_S} rays refused, more than 10 %"
    # the figures the slab cases were chosen for
    ox_, x_ = records["T.slab_ox"], records["T.slab_x"]
    assert len(ox_["status"]) == 48 and ((ox_["status"] & 3) == 3).all() and len(ox_["converted"]) == 31, "T.slab_ox"
    assert int(ox_["step_number"].min()) == 124 and int(ox_["step_number"].max()) == 187, "T.slab_ox: step numbers"
    assert (x_["iterations"] == 8).all() and len(x_["converted"]) == 31, "T.slab_x"
    syn = dict(zip((str(n) for n in records["S.synthetic"]["names"]), range(len(records["S.synthetic"]["names"]))))
    s = records["S.synthetic"]
    for n in (1, 2, 63, 64, 65, 128):
        assert s["step_number"][syn[f"decrease_{n}_{n + 1}"]] == n
    assert s["step_number"][syn["decrease_at_the_end_of_130"]] == 129
    assert s["step_number"][syn["plateau_then_decrease"]] == 70 and s["step_number"][syn["adjacent_doubles_descending"]] == 30
    assert s["step_number"][syn["second_larger_maximum"]] == 20 and s["status"][syn["refused_after_the_decrease"]] & ox.FOUND_MAX
    for n in ("refused_before_the_decrease", "refused_first_point"):
        assert s["status"][syn[n]] == ox.EQ_REFUSED
    for n in ("no_decrease_64", "no_decrease_65", "no_decrease_200", "npoints_0", "npoints_1", "npoints_2_rising"):
        assert s["status"][syn[n]] == 0
    assert s["iterations"][syn["maximum_within_the_tolerance"]] == 1
    cap = records["S.capped"]
    assert cap["iterations"][0] == 11 and cap["status"][0] == ox.FOUND_MAX and cap["status"][1] & ox.FOUND_CUTOFF


def generate(out_root):
    records = {c.name: case_record(c) for c in ox.CASES}
    check_conditions(records)
    out = {"cases": np.array([c.name for c in ox.CASES])}
    for name, rec in records.items():
        for k, v in rec.items():
            out[name + ":" + k] = v
    path = os.path.join(out_root, ox.FIXTURE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    for name, rec in records.items():
        st = rec["status"]
        print(f"{name}: {len(st)} rays, {int(((st & 3) == 3).sum())} with maximum and cutoff, {len(rec['converted'])} converted, "
              f"{int(((st & ox.EQ_REFUSED) != 0).sum())} refused, iterations {sorted(set(rec['iterations'].tolist()))}, "
              f"{rec['ray_vec'].shape[1]} points kept")
    print(f"ox_conv_cases -> {os.path.getsize(path) / 1e3:.0f} kB")
    return path


def check():
    with tempfile.TemporaryDirectory() as d:
        a, b = np.load(generate(d)), np.load(os.path.join(ROOT, ox.FIXTURE))
        diffs = []
        if set(a.files) != set(b.files):
            diffs.append(f"keys differ: only regenerated {sorted(set(a.files) - set(b.files))}, "
                         f"only committed {sorted(set(b.files) - set(a.files))}")
        diffs += [f"'{k}' differs" for k in sorted(set(a.files) & set(b.files)) if not same_bits(a[k], b[k])]
    return diffs


def main():
    for exe in (REF, REF_STATES):
        if not os.path.exists(exe):
            sys.exit(f"{os.path.relpath(exe, ROOT)} missing: run `bash oracle/build_ref.sh` first")
    if "--check" in sys.argv[1:]:
        diffs = check()
        for x in diffs:
            print("DIFF", x)
        print("make_ox_conv_cases --check:", "the committed fixture is what this script produces" if not diffs
              else f"{len(diffs)} differences")
        sys.exit(1 if diffs else 0)
    generate(ROOT)


if __name__ == "__main__":
    main()
