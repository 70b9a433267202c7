// TEST INFRASTRUCTURE ONLY: the packed ray diagnostics' locator (rays_amd/csrc/rays_diag.hpp: diag_locate,
// diag_locate_from) compiled for the host and applied to every flat index.  Used by
// tests/test_cpu_ray_diagnostics_packed.py.
#include <hip/hip_runtime.h>
RAYS_EMUL_DEFINE_GLOBALS
#include "../../rays_amd/csrc/rays_diag.hpp"

// ray[j] = diag_locate(offsets, nray, j) for j = 0 .. offsets[nray] - 1
extern "C" void rays_emul_diag_locate(const long long* offsets, int nray, int* ray) {
  for (long long j = 0; j < offsets[nray]; j++) ray[j] = rays::diag_locate(offsets, nray, j);
}

// the kernel's two-step form: the first ray of the index's run of `wave` consecutive indices by bisection, the index's
// own ray from there
extern "C" void rays_emul_diag_locate_wave(const long long* offsets, int nray, int wave, int* ray) {
  for (long long j = 0; j < offsets[nray]; j++) {
    const int r0 = rays::diag_locate(offsets, nray, j - j % wave);
    ray[j] = rays::diag_locate_from(offsets, nray, r0, j);
  }
}
