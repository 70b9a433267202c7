"""The committed fixtures are what the committed generator produces: `make_golden.py --check` regenerates every
fixture from the reference binary into a scratch directory and compares it with tests/golden/ and the host
tables under configs/ bit for bit (the results file: up to its date / wall-time records).  Runs where the
reference binary exists (this container; it is built from /root/reference by oracle/build_ref.sh)."""
import math
import os
import sys

import pytest

from tests.common import ROOT

REF = os.path.join(ROOT, "oracle", "_ref", "rays_ref_dump")


def _make_golden():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_golden
    finally:
        sys.path.pop(0)
    return make_golden


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/rays_ref_dump not built (no /root/reference here)")
def test_committed_fixtures_are_what_the_generator_produces():
    diffs = _make_golden().check()
    assert not diffs, "\n".join(diffs)


def test_host_tables_are_the_union_of_the_eqdsk_cases():
    """configs/<eqdsk>.tables.npz carries every profile spline an eqdsk namelist of this repo selects on that file
    (65 x 65: ne_* for the damping fixtures, te_* / ti_* for the splined-temperature ones; 129 x 129, BASELINE config
    5's file, and the 49 x 65 file on the box whose spacings are no powers of two: all three): no case's tables overwrite
    another's."""
    import numpy as np
    for f, nr, nz in (("solovev_65x65.geqdsk", 65, 65), ("solovev_129x129.geqdsk", 129, 129), ("solovev_49x65.geqdsk", 49, 65)):
        z = np.load(os.path.join(ROOT, _make_golden().tables_path(f)))
        for k in ("r_grid", "z_grid", "psi_fspl", "rb_grid", "rb_fspl", "ne_grid", "ne_fspl", "te_grid", "te_fspl",
                  "ti_grid", "ti_fspl", "rho_grid", "rho_fspl"):
            assert k in z.files and z[k].size, (f, k)
        assert len(z["r_grid"]) == nr and len(z["z_grid"]) == nz


def test_cfg5_equilibrium_file_is_what_the_references_own_tool_writes(tmp_path):
    """BASELINE config 5: "eqdsk 129 x 129 written by solovev_2_eqdsk".  configs/solovev_129x129.geqdsk
    must be the output of oracle/_ref/solovev_2_eqdsk (the reference's program, compiled by oracle/build_ref.sh) on
    configs/solovev_2_eqdsk_129.in, byte for byte; cfg 5 and cfg 5b must name it and the splined temperature model.
    The same for configs/solovev_49x65.geqdsk (configs/solovev_2_eqdsk_49x65.in), whose R and Z spacings are no powers of
    two (1.08 / 48 and 1.48 / 64)."""
    import shutil
    import subprocess
    import numpy as np
    from rays_amd.namelist import read_namelist
    for cfg in ("cfg5_axisym256k_sg_damp.in", "cfg5b_axisym256k_rk4_damp.in"):
        nml = read_namelist(os.path.join(ROOT, "configs", cfg))
        assert nml["eqdsk_magnetics_spline_interp_list"]["eqdsk_file_name"].strip() == "solovev_129x129.geqdsk"
        m = nml["axisym_toroid_eq_list"]["temperature_prof_model"]   # scalar, list, or {species index: model}
        models = [m[k] for k in sorted(m)] if isinstance(m, dict) else list(np.atleast_1d(m))
        assert models and all(str(x).strip() == "temperature_spline_interp" for x in models), (cfg, m)
    tool = os.path.join(ROOT, "oracle", "_ref", "solovev_2_eqdsk")
    if not os.path.exists(tool):
        pytest.skip("oracle/_ref/solovev_2_eqdsk not built (needs /root/reference)")
    for namelist, eqdsk in (("solovev_2_eqdsk_129.in", "solovev_129x129.geqdsk"), ("solovev_2_eqdsk_49x65.in", "solovev_49x65.geqdsk")):
        shutil.copy(os.path.join(ROOT, "configs", namelist), tmp_path / "rays.in")
        subprocess.run([tool], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        assert (tmp_path / eqdsk).read_bytes() == open(os.path.join(ROOT, "configs", eqdsk), "rb").read(), eqdsk
    z = np.load(os.path.join(ROOT, _make_golden().tables_path("solovev_49x65.geqdsk")))
    for grid in (z["r_grid"], z["z_grid"]):       # no power of two: the quotient of the cell estimate is inexact
        h = float(grid[1] - grid[0])
        assert math.frexp(h)[0] != 0.5


REF_LAUNCH = os.path.join(ROOT, "oracle", "_ref", "ref_launch")


@pytest.mark.skipif(not os.path.exists(REF_LAUNCH), reason="oracle/_ref/ref_launch not built (no /root/reference here)")
def test_launch_fixture_is_what_the_references_launchers_produce(tmp_path):
    """tests/golden/launch_cases.npz regenerated from oracle/_ref/ref_launch (the reference's initialize on the namelists
    of tests/launch_cases.py): the same entries, each the same dtype, shape and bytes."""
    import numpy as np
    from tests import launch_cases as lc
    lc.generate(str(tmp_path), REF_LAUNCH)
    a, b = np.load(tmp_path / lc.FIXTURE), np.load(os.path.join(ROOT, lc.FIXTURE))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
