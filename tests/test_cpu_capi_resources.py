"""CPU tier: rays_amd/csrc/rays_capi_resources.hpp -- the owners of the C ABI's device resources -- alone, as a
stand-alone program on the emulated HIP runtime with four devices (tests/hip_emul/emul_capi_resources_main.cpp), built
with AddressSanitizer + UBSan linked into the executable and run as a child process with leak detection on: a
workspace that grows, shrinks its request and grows again on two streams of two devices; a table uploaded on two
devices, re-versioned, released and fetched again; a DeviceBuffers destroyed on an early exit with blocks allocated
and one detached; a cache slot claimed for another device while a block from it is out; everything released, nothing
of the runtime left alive."""
import os
import subprocess

from tests.common import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "hip_emul")


def build_sanitized_resources():
    exe = os.path.join(EMUL_DIR, "emul_capi_resources_san")
    srcs = [os.path.join(EMUL_DIR, "emul_capi_resources_main.cpp"), os.path.join(EMUL_DIR, "hip", "hip_runtime.h"),
            os.path.join(EMUL_DIR, "hip", "hip_runtime_api_emul.h"), os.path.join(EMUL_DIR, "emul_capi_check.hpp"),
            os.path.join(ROOT, "rays_amd", "csrc", "rays_capi_resources.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                               "-static-libubsan", "-I", EMUL_DIR, srcs[0], "-o", exe, "-lpthread"])
    return exe


def test_resource_owners_are_clean_under_asan_ubsan():
    exe = build_sanitized_resources()
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", RAYS_EMUL_DEVICES="4")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "capi resources ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
