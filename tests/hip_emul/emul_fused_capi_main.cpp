// TEST INFRASTRUCTURE ONLY: the host form of the fused trace + deposition (rays_hip_trace_deposition,
// rays_amd/csrc/rays_capi.hip) as a stand-alone program on the emulated HIP runtime with four devices -- for plain and
// for sanitizer runs (tests/hip_emul/Makefile.capi, target fused; tests/test_cpu_fused_deposition.py writes the case file and
// starts it).
//   emul_fused_capi <case file>
// Case file (native endianness): int32 nray, nv, n_bins, which, nx, sizeof(rays_params_t); the parameter block; real64
// x_min, x_max, fspl_re[nx][4] (the Z-function table); rvec0[nray][3], rindex_vec0[nray][3], power[nray]; then what the
// one-lane emulation of the fused kernel gave for these rays: npoints[nray], stop_code[nray] (int32),
// start_ray_vec[nray][nv], end_ray_vec[nray][nv], end_residuals[nray], max_residuals[nray], work[nray][n_bins].
// Every device list of 1 to 4 devices traces the first n rays for several n -- a ragged last block, blocks that are
// empty -- and must reproduce those bytes, with the profile the ray-ordered sum over the n rows: blocks chained over
// the devices equal the single block.  After rays_hip_finalize the emulated driver holds nothing.
#include <hip/hip_runtime.h>

#include "emul_capi_check.hpp"
#include "../../rays_amd/csrc/rays_deposition.hpp"

// The two launchers of rays_deposition.hip (not part of the emulated build: its kernels use wave intrinsics), on the host:
// the emulated runtime runs a kernel when it is launched, so they do their work here and now.
namespace rays {
hipError_t launch_dep_trace_args(const DepTraceArgs& T, DepTraceArgs* d_out, hipStream_t) {
  *d_out = T;
  return hipSuccess;
}
hipError_t launch_profile_sum(int n_bins, int nray, const double* work, const double* carry, double* profile, hipStream_t) {
  for (int b = 0; b < n_bins; b++) {
    double s = carry ? carry[b] : 0.;
    for (int r = 0; r < nray; r++) s = s + work[(size_t)b * nray + r];
    profile[b] = s;
  }
  return hipSuccess;
}
}  // namespace rays

extern "C" void rays_emul_runtime_stats(long long* launches, long long* wrong_device, long long* live_allocations);
extern "C" void rays_emul_runtime_live(long long* pinned, long long* streams, long long* events);

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t head[6];
  if (std::fread(head, sizeof head, 1, f) != 1 || head[5] != rays_hip_sizeof_params()) {
    std::fprintf(stderr, "case file does not match this library's rays_params_t\n");
    return 2;
  }
  const size_t nray = (size_t)head[0], nv = (size_t)head[1], nb = (size_t)head[2];
  const int which = head[3], nx = head[4];
  rays_params_t p;
  double zr[2];
  std::vector<double> zf, r0, n0, pw, start, end, eres, mres, work;
  std::vector<int32_t> np, sc;
  bool ok = std::fread(&p, sizeof p, 1, f) == 1 && std::fread(zr, sizeof zr, 1, f) == 1 && read_n(f, zf, 4 * (size_t)nx) &&
            read_n(f, r0, 3 * nray) && read_n(f, n0, 3 * nray) && read_n(f, pw, nray) && read_n(f, np, nray) &&
            read_n(f, sc, nray) && read_n(f, start, nv * nray) && read_n(f, end, nv * nray) && read_n(f, eres, nray) &&
            read_n(f, mres, nray) && read_n(f, work, nb * nray);
  std::fclose(f);
  if (!ok || (int)nv != p.nv) { std::fprintf(stderr, "short or inconsistent case file\n"); return 2; }
  if (rays_hip_device_count() < 4) { std::fprintf(stderr, "needs 4 emulated devices\n"); return 2; }
  CHECK(rays_hip_set_zfun_table(zf.data(), nx, zr[0], zr[1]) == 0);

  const int lists[][4] = {{0}, {2, 1}, {0, 1, 3}, {0, 1, 2, 3}};
  int calls = 0;
  for (int G = 1; G <= 4; G++) {
    CHECK(rays_hip_init_devices(G, lists[G - 1]) >= 0);
    // all rays (a ragged last block); G + 1 rays (an empty block with four devices); 1 ray (G - 1 empty blocks); none
    const size_t counts[] = {nray, (size_t)G + 1, 1, 0};
    for (size_t n : counts) {
      if (n > nray) continue;
      // the profile of the first n rays: the ray-ordered sum over their rows, as ONE block forms it
      std::vector<double> prof(nb, 0.);
      for (size_t b = 0; b < nb; b++)
        for (size_t r = 0; r < n; r++) prof[b] = prof[b] + work[r * nb + b];
      // poisoned outputs, one element longer than asked for: nothing behind the last ray may be touched
      std::vector<int32_t> o_np(n + 1, -7), o_sc(n + 1, -7);
      std::vector<double> o_start(nv * n + 1, -7.), o_end(nv * n + 1, -7.), o_er(n + 1, -7.), o_mr(n + 1, -7.);
      std::vector<double> o_work(nb * n + 1, -7.), o_prof(nb + 1, -7.);
      double elapsed = -1.;
      const int rc = rays_hip_trace_deposition(&p, (int)n, r0.data(), n0.data(), pw.data(), which, (int)nb, o_np.data(),
                                               o_sc.data(), o_start.data(), o_end.data(), o_er.data(), o_mr.data(),
                                               o_work.data(), o_prof.data(), &elapsed);
      if (rc) std::fprintf(stderr, "rays_hip_trace_deposition(G = %d, n = %zu): rc %d: %s\n", G, n, rc, last_error().c_str());
      CHECK(rc == 0 && elapsed >= 0.);
      CHECK(std::memcmp(o_np.data(), np.data(), sizeof(int32_t) * n) == 0 && o_np[n] == -7);
      CHECK(std::memcmp(o_sc.data(), sc.data(), sizeof(int32_t) * n) == 0 && o_sc[n] == -7);
      CHECK(std::memcmp(o_start.data(), start.data(), sizeof(double) * nv * n) == 0 && o_start[nv * n] == -7.);
      CHECK(std::memcmp(o_end.data(), end.data(), sizeof(double) * nv * n) == 0 && o_end[nv * n] == -7.);
      CHECK(std::memcmp(o_er.data(), eres.data(), sizeof(double) * n) == 0 && o_er[n] == -7.);
      CHECK(std::memcmp(o_mr.data(), mres.data(), sizeof(double) * n) == 0 && o_mr[n] == -7.);
      CHECK(std::memcmp(o_work.data(), work.data(), sizeof(double) * nb * n) == 0 && o_work[nb * n] == -7.);
      CHECK(std::memcmp(o_prof.data(), prof.data(), sizeof(double) * nb) == 0 && o_prof[nb] == -7.);
      // work and start_ray_vec are optional
      std::vector<double> q_prof(nb, -7.);
      CHECK(rays_hip_trace_deposition(&p, (int)n, r0.data(), n0.data(), pw.data(), which, (int)nb, o_np.data(), o_sc.data(),
                                      nullptr, o_end.data(), o_er.data(), o_mr.data(), nullptr, q_prof.data(), nullptr) == 0);
      CHECK(std::memcmp(q_prof.data(), prof.data(), sizeof(double) * nb) == 0);
      calls += 2;
    }
  }
  // refusals, by name
  std::vector<int32_t> i1(1);
  std::vector<double> d1(nv + nb);
  const char* who = "rays_hip_trace_deposition";
  CHECK(refused(rays_hip_trace_deposition(&p, -1, r0.data(), n0.data(), pw.data(), which, (int)nb, i1.data(), i1.data(), nullptr,
                                          d1.data(), d1.data(), d1.data(), nullptr, d1.data(), nullptr), "rays_hip_trace_deposition: nray < 0"));
  CHECK(refused(rays_hip_trace_deposition(&p, 1, r0.data(), n0.data(), pw.data(), which, 0, i1.data(), i1.data(), nullptr,
                                          d1.data(), d1.data(), d1.data(), nullptr, d1.data(), nullptr), "n_bins = 0 is outside 1..320"));
  CHECK(refused(rays_hip_trace_deposition(&p, 1, r0.data(), n0.data(), nullptr, which, (int)nb, i1.data(), i1.data(), nullptr,
                                          d1.data(), d1.data(), d1.data(), nullptr, d1.data(), nullptr), "rays_hip_trace_deposition: null array argument"));
  CHECK(refused(rays_hip_trace_deposition(&p, 1, r0.data(), n0.data(), pw.data(), RAYS_DEP_PTOTAL_X, (int)nb, i1.data(), i1.data(),
                                          nullptr, d1.data(), d1.data(), d1.data(), nullptr, d1.data(), nullptr), "unimplemented profile for this equilib_model"));
  CHECK(refused(rays_hip_trace_deposition_device(&p, 1, nullptr, nullptr, nullptr, which, (int)nb, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "rays_hip_trace_deposition_device: null device pointer"));
  (void)who;
  CHECK(std::strstr(rays_hip_deposition_kernel_name_for(&p, (int)nray), "rk4_trace_kernel<102, 2, 0, 8>") != nullptr);

  long long launches = 0, wrong = 0, live = -1, pinned = -1, streams = -1, events = -1;
  rays_emul_runtime_stats(&launches, &wrong, &live);
  CHECK(wrong == 0 && live > 0);   // (the entry's cached blocks, the argument blocks and the refill counters are still held)
  CHECK(rays_hip_finalize() == 0);
  rays_emul_runtime_stats(&launches, &wrong, &live);
  rays_emul_runtime_live(&pinned, &streams, &events);
  CHECK(live == 0 && pinned == 0 && streams == 0 && events == 0 && wrong == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("fused capi ok: %d calls, %lld launches\n", calls, launches);
  return 0;
}
