"""CPU tier: the ray launchers against the reference's own launchers on the launches of tests/launch_cases.py -- every
wave mode and sign, every compaction shape, fan members one spacing of doubles apart across the evanescent thresholds,
degenerate launch points (tests/golden/launch_cases.npz, cut from oracle/_ref/ref_launch).  Two implementations, bit for
bit, NaN equal to NaN, no tolerance:
  * the device header's fan_member (rays_ray_init.hpp) and the host fan setup (rays_fan_setup.inc) compiled for the host
    (tests/hip_emul), members visited in the reference's loop order;
  * the Python host mirror rays_amd/ray_init.py, for the launchers it restates.
The three kernels around fan_member (candidates, block scan, ordered scatter) run on the GPU tier only
(tests/test_gpu_launch_cases.py): the one-lane host emulation has no block-level __syncthreads / __ballot."""
import numpy as np
import pytest

from rays_amd.params import ConfigError
from rays_amd.ray_init import initialize_ray_init
from tests import emul_lib
from tests import launch_cases as lc

ALL = [c.name for c in lc.CASES]


@pytest.mark.parametrize("name", ALL)
def test_fan_member_on_host_equals_reference(name):
    case, nml, p, fan, nray_max, tab = lc.load_case(name)
    rec = lc.load_fixture(name)
    r0, n0 = emul_lib.ray_init(p, fan, nray_max)
    if "stop" in rec:          # the reference stopped: nothing launched (the text is the C ABI's: GPU tier, and below)
        assert len(r0) == 0, f"{name}: {len(r0)} rays where the reference stops with {str(rec['stop'])!r}"
        return
    lc.compare_fan(name, rec, r0, n0, None, "fan_member on the host")


# rays_amd/ray_init.py restates no fields for 'solovev_magnetics' and 'eqdsk_magnetics_lin_interp': there the device
# launcher is the Python host's too
MIRRORED = [c.name for c in lc.CASES if c.base not in (lc.B_AXI["solmag"], lc.B_AXI["eqlin"])]


@pytest.mark.parametrize("name", MIRRORED)
def test_python_mirror_equals_reference(name):
    case, nml, p, fan, nray_max, tab = lc.load_case(name)
    assert p.equilib_model != 2 or p.axisym.magnetics_model == 0
    rec = lc.load_fixture(name)
    if "stop" in rec:
        with pytest.raises(ConfigError) as e:
            initialize_ray_init(p, nml, tab)
        assert str(e.value) == str(rec["stop"])
        return
    r0, n0, w = initialize_ray_init(p, nml, tab)
    lc.compare_fan(name, rec, r0, n0, w, "rays_amd/ray_init.py")


# ---- the fixture itself: a file of fans that all keep everything would prove nothing ----
def test_fixture_holds_every_case_and_nothing_else():
    import os
    z = np.load(os.path.join(lc.ROOT, lc.FIXTURE), allow_pickle=False)
    assert [str(x) for x in z["cases"]] == ALL
    assert {k.split(":")[0] for k in z.files if ":" in k} == set(ALL)
    assert os.path.getsize(os.path.join(lc.ROOT, lc.FIXTURE)) < 1_000_000


@pytest.mark.parametrize("cls", ["A", "B", "C", "D"])
def test_every_class_keeps_some_and_drops_some(cls):
    mixed = [n for n in lc.of_class(cls) if 0 < int(lc.load_fixture(n)["nray"]) < lc.n_candidates(lc.BY_NAME[n])]
    assert mixed, f"class {cls}: no fan both keeps and drops"
    if cls == "A":    # every launcher x magnetics model x mode x sign, and every species count
        for n in lc.of_class("A"):
            assert n in mixed, f"{n}: {int(lc.load_fixture(n)['nray'])} of {lc.n_candidates(lc.BY_NAME[n])} kept"
    if cls == "B":
        kept_all = [n for n in lc.of_class("B") if int(lc.load_fixture(n)["nray"]) == lc.n_candidates(lc.BY_NAME[n])]
        sizes = {lc.n_candidates(lc.BY_NAME[n]) for n in kept_all}
        assert {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025} <= sizes
        assert {63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 15295} <= {lc.n_candidates(lc.BY_NAME[n]) for n in mixed}


def test_class_E_is_the_references_stop():
    for n in lc.of_class("E"):
        rec = lc.load_fixture(n)
        assert int(rec["nray"]) == 0 and int(rec["exit"]) == 0 and str(rec["stop"]) == lc.STOP_TEXT, n
    launchers = {lc._launcher_of(lc.BY_NAME[n].base) for n in lc.of_class("E")}
    assert launchers == {lc.SLAB, lc.SOLOVEV, lc.AXISYM}


def _slab_member_index(case, rec):
    """index in the 16-member fan of each survivor of a slab threshold case, from the recorded (ny, nz)"""
    from rays_amd.namelist import parse_namelist
    g = parse_namelist(lc.namelist_text(case))["simple_slab_ray_init_list"]
    scan_y = int(g["n_ky_launch"]) == 16
    a0, da = (float(g["rindex_y0"]), float(g["delta_rindex_y0"])) if scan_y else (float(g["rindex_z0"]), float(g["delta_rindex_z0"]))
    vals = [a0 + i * da for i in range(16)]
    assert len(set(vals)) == 16
    return [vals.index(float(v)) for v in rec["rindex_vec0"][:, 1 if scan_y else 2]]


@pytest.mark.parametrize("name", lc.of_class("C"))
def test_threshold_fans_straddle_their_threshold(name):
    """Survivors and drops next to each other in the fan, i.e. one spacing of doubles apart; the reference's own cut
    falls inside the fan, not at its end (the bisection aimed 8 members at either side)."""
    case, rec = lc.BY_NAME[name], lc.load_fixture(name)
    n = int(rec["nray"])
    assert lc.n_candidates(case) == 16 and 0 < n < 16, f"{name}: {n} of 16 kept"
    if lc._launcher_of(case.base) == lc.SLAB:
        kept = _slab_member_index(case, rec)
        assert kept == sorted(kept) and len(set(kept)) == n
        assert any((i + 1 in kept) != (i in kept) for i in range(15))
    elif "phi" in name:     # the y component of a launch at y = 0 is rindex_phi itself
        from rays_amd.namelist import parse_namelist
        g = parse_namelist(lc.namelist_text(case))["solovev_ray_init_nphi_ktheta_list"]
        vals = [float(g["rindex_phi0"]) + i * float(g["delta_rindex_phi"]) for i in range(16)]
        kept = [vals.index(float(v)) for v in rec["rindex_vec0"][:, 1]]
        assert kept == sorted(kept) and any((i + 1 in kept) != (i in kept) for i in range(15))


def test_solovev_weights_are_compared_where_the_reference_sets_them():
    """ray_pwr_wt of a Solovev record: 1 / nray at (survivor count after each r loop) - 1 and compared there only; the big fan's
    fifth r position is the magnetic axis (0.3 - 4 * 0.075 = 0), which adds no survivor: four distinct counts"""
    for n in lc.of_class("A", "B", "C", "D"):
        rec = lc.load_fixture(n)
        if lc._launcher_of(lc.BY_NAME[n].base) != lc.SOLOVEV or "stop" in rec:
            continue
        i = rec["wt_index"]
        assert len(i) >= 1 and int(i[-1]) == int(rec["nray"]) - 1 and (rec["ray_pwr_wt"][i] == 1.0 / int(rec["nray"])).all(), n
    rec = lc.load_fixture("B.solovev.big.minus")
    assert len(rec["wt_index"]) == 4 and not np.isnan(rec["rindex_vec0"]).any()
