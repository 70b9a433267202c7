"""GPU tier: the three launcher kernels (rays_ray_init.hip: candidates, block scan, ordered scatter) and the C ABI
around them against the reference's own launchers on the launches of tests/launch_cases.py
(tests/golden/launch_cases.npz, cut from oracle/_ref/ref_launch): ray count, ray order, values and weights bit for bit,
NaN equal to NaN, no tolerance anywhere.  The largest fan has 15 295 candidates."""
import numpy as np
import pytest

from rays_amd import hip
from tests import launch_cases as lc

pytestmark = pytest.mark.gpu

ALL = [c.name for c in lc.CASES]
SENTINEL = -7.25e300     # no launch position or index component of any case


def _expect_stop(rec, call):
    with pytest.raises(hip.RaysHipError) as e:
        call()
    assert hip.last_error() == str(rec["stop"]) and str(e.value).endswith(": " + str(rec["stop"]))


@pytest.mark.parametrize("name", ALL)
def test_ray_init_host_equals_reference(name):
    """rays_hip_ray_init: arrays, order, count and ray_pwr_wt (Solovev: at the entries the reference sets)"""
    case, nml, p, fan, nray_max, tab = lc.load_case(name)
    rec = lc.load_fixture(name)
    if "stop" in rec:
        _expect_stop(rec, lambda: hip.ray_init_host(p, fan, nray_max))
        return
    r0, n0, w = hip.ray_init_host(p, fan, nray_max)
    lc.compare_fan(name, rec, r0, n0, w, "rays_hip_ray_init")


def _device_call(name, calls):
    """rays_hip_ray_init_device on a stream of its own into arrays of nray_max rows filled with a sentinel, `calls` times
    into the same arrays -> the arrays and nray of each call (None: the call raised with the reference's stop text)"""
    import torch
    case, nml, p, fan, nray_max, tab = lc.load_case(name)
    rec = lc.load_fixture(name)
    stream = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(stream):
        d_r = torch.full((nray_max, 3), SENTINEL, dtype=torch.float64, device="cuda")
        d_n = torch.full((nray_max, 3), SENTINEL, dtype=torch.float64, device="cuda")
        for _ in range(calls):
            run = lambda: hip.ray_init_device(p, fan, nray_max, d_r.data_ptr(), d_n.data_ptr(), stream.cuda_stream)
            if "stop" in rec:
                _expect_stop(rec, run)
                nray = None
            else:
                nray = run()
            stream.synchronize()
            out.append((nray, d_r.cpu().numpy(), d_n.cpu().numpy()))
    return rec, out


def _check_device_arrays(name, rec, nray, r, n):
    want = int(rec["nray"])
    assert (nray or 0) == want, f"{name}: nray = {nray}, the reference launched {want}"
    if want:
        lc.compare_fan(name, rec, r[:want], n[:want], None, "rays_hip_ray_init_device")
    for key, a in (("rvec0", r), ("rindex_vec0", n)):      # nothing written past the survivors
        assert (a[want:] == SENTINEL).all(), f"{name}: {key} written at row {want + int(np.argmax((a[want:] != SENTINEL).any(axis=1)))} >= nray = {want}"


@pytest.mark.parametrize("name", lc.of_class("B", "D"))
def test_ray_init_device_on_a_stream_writes_the_survivors_and_nothing_else(name):
    rec, ((nray, r, n),) = _device_call(name, 1)
    _check_device_arrays(name, rec, nray, r, n)


@pytest.mark.parametrize("name", lc.of_class("B", "D"))
def test_ray_init_device_twice_into_the_same_arrays(name):
    rec, (first, second) = _device_call(name, 2)
    _check_device_arrays(name, rec, *second)
    assert first[0] == second[0]
    for a, b in zip(first[1:], second[1:]):
        assert lc.same_bits(a, b)


@pytest.mark.parametrize("name", lc.of_class("E"))
def test_nothing_survives_is_the_references_stop(name):
    case, nml, p, fan, nray_max, tab = lc.load_case(name)
    rec = lc.load_fixture(name)
    assert str(rec["stop"]) == lc.STOP_TEXT
    _expect_stop(rec, lambda: hip.ray_init_host(p, fan, nray_max))
