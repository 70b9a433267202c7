// TEST INFRASTRUCTURE ONLY: the host form of the fused deposition into two profiles (rays_hip_trace_profiles,
// rays_amd/csrc/rays_capi.hip) as a stand-alone program on the emulated HIP runtime with four devices -- for plain and
// for sanitizer runs (tests/hip_emul/Makefile.profiles, target profiles; tests/test_cpu_fused_profiles.py writes the case
// file and starts it).
//   emul_profiles_capi <case file>
// Case file (native endianness): int32 nray, nv, n_bins_a, n_bins_b, which_a, which_b, nx, sizeof(rays_params_t); the
// parameter block; real64 x_min, x_max, fspl_re[nx][4] (the Z-function table); int32 nr, nz, n_rb, n_ne, n_te, n_ti and
// the eleven arrays of rays_axisym_tables_t, each behind its int32 length; int32 n_rho, rho_grid[n_rho],
// rho_fspl[n_rho][4]; rvec0[nray][3], rindex_vec0[nray][3], power[nray]; then what the one-lane emulation of the
// two-profile kernel gave for these rays: npoints[nray], stop_code[nray] (int32), start_ray_vec[nray][nv],
// end_ray_vec[nray][nv], end_residuals[nray], max_residuals[nray], work_a[nray][n_bins_a], work_b[nray][n_bins_b].
// Every device list of 1 to 4 devices traces the first n rays for several n -- a ragged last block, blocks that are
// empty -- and must reproduce those bytes, with each profile the ray-ordered sum over its n rows: blocks chained over
// the devices equal the single block.  The refusals, by name.  After rays_hip_finalize the emulated driver holds nothing.
#include <hip/hip_runtime.h>

#include "emul_capi_check.hpp"
#include "../../rays_amd/csrc/rays_deposition.hpp"

// The launchers of rays_deposition.hip (not part of the emulated build: its kernels use wave intrinsics), on the host:
// the emulated runtime runs a kernel when it is launched, so they do their work here and now.
namespace rays {
hipError_t launch_dep_trace_args(const DepTraceArgs& T, DepTraceArgs* d_out, hipStream_t) {
  *d_out = T;
  return hipSuccess;
}
hipError_t launch_dep2_trace_args(const Dep2TraceArgs& T, Dep2TraceArgs* d_out, hipStream_t) {
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

static bool read_array(std::FILE* f, std::vector<double>& v) {
  int32_t n = 0;
  return std::fread(&n, sizeof n, 1, f) == 1 && n >= 0 && read_n(f, v, (size_t)n);
}
// the ray-ordered sum over the first n rows of work[nray][nb], as ONE block forms it
static std::vector<double> ordered_profile(const std::vector<double>& work, size_t nb, size_t n) {
  std::vector<double> prof(nb, 0.);
  for (size_t b = 0; b < nb; b++)
    for (size_t r = 0; r < n; r++) prof[b] = prof[b] + work[r * nb + b];
  return prof;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t head[8];
  if (std::fread(head, sizeof head, 1, f) != 1 || head[7] != rays_hip_sizeof_params()) {
    std::fprintf(stderr, "case file does not match this library's rays_params_t\n");
    return 2;
  }
  const size_t nray = (size_t)head[0], nv = (size_t)head[1];
  const size_t nb[2] = {(size_t)head[2], (size_t)head[3]};
  const int which[2] = {head[4], head[5]}, nx = head[6];
  rays_params_t p;
  double zr[2];
  int32_t tn[6], n_rho = 0;
  std::vector<double> zf, tab[11], rho_grid, rho_fspl, r0, n0, pw, start, end, eres, mres, work[2];
  std::vector<int32_t> np, sc;
  bool ok = std::fread(&p, sizeof p, 1, f) == 1 && std::fread(zr, sizeof zr, 1, f) == 1 && read_n(f, zf, 4 * (size_t)nx) &&
            std::fread(tn, sizeof tn, 1, f) == 1;
  for (int k = 0; ok && k < 11; k++) ok = read_array(f, tab[k]);
  ok = ok && std::fread(&n_rho, sizeof n_rho, 1, f) == 1 && read_n(f, rho_grid, (size_t)n_rho) &&
       read_n(f, rho_fspl, 4 * (size_t)n_rho) && read_n(f, r0, 3 * nray) && read_n(f, n0, 3 * nray) && read_n(f, pw, nray) &&
       read_n(f, np, nray) && read_n(f, sc, nray) && read_n(f, start, nv * nray) && read_n(f, end, nv * nray) &&
       read_n(f, eres, nray) && read_n(f, mres, nray) && read_n(f, work[0], nb[0] * nray) && read_n(f, work[1], nb[1] * nray);
  std::fclose(f);
  if (!ok || (int)nv != p.nv) { std::fprintf(stderr, "short or inconsistent case file\n"); return 2; }
  if (rays_hip_device_count() < 4) { std::fprintf(stderr, "needs 4 emulated devices\n"); return 2; }
  CHECK(rays_hip_set_zfun_table(zf.data(), nx, zr[0], zr[1]) == 0);
  rays_axisym_tables_t T;
  std::memset(&T, 0, sizeof T);
  T.nr = tn[0]; T.nz = tn[1]; T.n_rb = tn[2]; T.n_ne = tn[3]; T.n_te = tn[4]; T.n_ti = tn[5];
  auto ptr = [&](int k) -> const double* { return tab[k].empty() ? nullptr : tab[k].data(); };
  T.r_grid = ptr(0); T.z_grid = ptr(1); T.psi_fspl = ptr(2); T.rb_grid = ptr(3); T.rb_fspl = ptr(4); T.ne_grid = ptr(5);
  T.ne_fspl = ptr(6); T.te_grid = ptr(7); T.te_fspl = ptr(8); T.ti_grid = ptr(9); T.ti_fspl = ptr(10);
  CHECK(rays_hip_set_axisym_tables(&T) == 0);

  // before the rho table is set the equilibrium has one profile, and the rho record is refused by name
  int set[RAYS_DEP_MAX_PROFILES] = {-1, -1};
  CHECK(rays_hip_deposition_profile_set(&p, set) == 1 && set[0] == RAYS_DEP_PTOTAL_PSI);
  std::vector<int32_t> i1(2);
  std::vector<double> d1(2 * nv + nb[0] + nb[1]);
  rays_dep_profile_t rec[2] = {{which[0], (int)nb[0], nullptr, nullptr, d1.data()}, {which[1], (int)nb[1], nullptr, nullptr, d1.data()}};
  auto host = [&](int n, int n_profiles, const rays_dep_profile_t* r) {
    return rays_hip_trace_profiles(&p, n, r0.data(), n0.data(), pw.data(), n_profiles, r, i1.data(), i1.data(), nullptr,
                                   d1.data(), d1.data(), d1.data(), nullptr);
  };
  CHECK(refused(host(1, 2, rec), "Ptotal_rho needs rays_hip_set_rho_table() first"));
  CHECK(rays_hip_set_rho_table(rho_grid.data(), rho_fspl.data(), n_rho) == 0);
  CHECK(rays_hip_deposition_profile_set(&p, set) == 2 && set[0] == RAYS_DEP_PTOTAL_PSI && set[1] == RAYS_DEP_PTOTAL_RHO);

  const int lists[][4] = {{0}, {2, 1}, {0, 1, 3}, {0, 1, 2, 3}};
  int calls = 0;
  for (int G = 1; G <= 4; G++) {
    CHECK(rays_hip_init_devices(G, lists[G - 1]) >= 0);
    // all rays (a ragged last block); G + 1 rays (an empty block with four devices); 1 ray (G - 1 empty blocks); none
    const size_t counts[] = {nray, (size_t)G + 1, 1, 0};
    for (size_t n : counts) {
      if (n > nray) continue;
      const std::vector<double> prof[2] = {ordered_profile(work[0], nb[0], n), ordered_profile(work[1], nb[1], n)};
      // poisoned outputs, one element longer than asked for: nothing behind the last ray may be touched
      std::vector<int32_t> o_np(n + 1, -7), o_sc(n + 1, -7);
      std::vector<double> o_start(nv * n + 1, -7.), o_end(nv * n + 1, -7.), o_er(n + 1, -7.), o_mr(n + 1, -7.);
      std::vector<double> o_work[2] = {std::vector<double>(nb[0] * n + 1, -7.), std::vector<double>(nb[1] * n + 1, -7.)};
      std::vector<double> o_prof[2] = {std::vector<double>(nb[0] + 1, -7.), std::vector<double>(nb[1] + 1, -7.)};
      double elapsed = -1.;
      const rays_dep_profile_t r2[2] = {{which[0], (int)nb[0], o_work[0].data(), nullptr, o_prof[0].data()},
                                        {which[1], (int)nb[1], o_work[1].data(), nullptr, o_prof[1].data()}};
      const int rc = rays_hip_trace_profiles(&p, (int)n, r0.data(), n0.data(), pw.data(), 2, r2, o_np.data(), o_sc.data(),
                                             o_start.data(), o_end.data(), o_er.data(), o_mr.data(), &elapsed);
      if (rc) std::fprintf(stderr, "rays_hip_trace_profiles(G = %d, n = %zu): rc %d: %s\n", G, n, rc, last_error().c_str());
      CHECK(rc == 0 && elapsed >= 0.);
      CHECK(std::memcmp(o_np.data(), np.data(), sizeof(int32_t) * n) == 0 && o_np[n] == -7);
      CHECK(std::memcmp(o_sc.data(), sc.data(), sizeof(int32_t) * n) == 0 && o_sc[n] == -7);
      CHECK(std::memcmp(o_start.data(), start.data(), sizeof(double) * nv * n) == 0 && o_start[nv * n] == -7.);
      CHECK(std::memcmp(o_end.data(), end.data(), sizeof(double) * nv * n) == 0 && o_end[nv * n] == -7.);
      CHECK(std::memcmp(o_er.data(), eres.data(), sizeof(double) * n) == 0 && o_er[n] == -7.);
      CHECK(std::memcmp(o_mr.data(), mres.data(), sizeof(double) * n) == 0 && o_mr[n] == -7.);
      for (int i = 0; i < 2; i++) {
        CHECK(std::memcmp(o_work[i].data(), work[i].data(), sizeof(double) * nb[i] * n) == 0 && o_work[i][nb[i] * n] == -7.);
        CHECK(std::memcmp(o_prof[i].data(), prof[i].data(), sizeof(double) * nb[i]) == 0 && o_prof[i][nb[i]] == -7.);
      }
      // work and start_ray_vec are optional; the records in the other order give the same rows
      std::vector<double> q_prof[2] = {std::vector<double>(nb[0], -7.), std::vector<double>(nb[1], -7.)};
      const rays_dep_profile_t r3[2] = {{which[1], (int)nb[1], nullptr, nullptr, q_prof[1].data()},
                                        {which[0], (int)nb[0], nullptr, nullptr, q_prof[0].data()}};
      CHECK(rays_hip_trace_profiles(&p, (int)n, r0.data(), n0.data(), pw.data(), 2, r3, o_np.data(), o_sc.data(), nullptr,
                                    o_end.data(), o_er.data(), o_mr.data(), nullptr) == 0);
      for (int i = 0; i < 2; i++) CHECK(std::memcmp(q_prof[i].data(), prof[i].data(), sizeof(double) * nb[i]) == 0);
      // one record: rays_hip_trace_deposition itself
      std::vector<double> s_work(nb[1] * n + 1, -7.), s_prof(nb[1] + 1, -7.);
      const rays_dep_profile_t r1 = {which[1], (int)nb[1], s_work.data(), nullptr, s_prof.data()};
      CHECK(rays_hip_trace_profiles(&p, (int)n, r0.data(), n0.data(), pw.data(), 1, &r1, o_np.data(), o_sc.data(), nullptr,
                                    o_end.data(), o_er.data(), o_mr.data(), nullptr) == 0);
      CHECK(std::memcmp(s_work.data(), work[1].data(), sizeof(double) * nb[1] * n) == 0 && s_work[nb[1] * n] == -7.);
      CHECK(std::memcmp(s_prof.data(), prof[1].data(), sizeof(double) * nb[1]) == 0 && s_prof[nb[1]] == -7.);
      calls += 3;
    }
  }

  // refusals, by name; nothing is written
  std::fill(d1.begin(), d1.end(), -7.);
  CHECK(refused(host(1, 0, rec), "n_profiles = 0 is outside 1..2"));
  CHECK(refused(host(1, 3, rec), "n_profiles = 3 is outside 1..2"));
  CHECK(refused(host(1, 2, nullptr), "rays_hip_trace_profiles: null profile list"));
  CHECK(refused(host(-1, 2, rec), "rays_hip_trace_profiles: nray < 0"));
  {
    rays_dep_profile_t r[2] = {rec[0], rec[0]};
    CHECK(refused(host(1, 2, r), "rays_hip_trace_profiles: the same profile twice"));
    r[1] = rec[1]; r[1].n_bins = 0;
    CHECK(refused(host(1, 2, r), "n_bins = 0 is outside 1..320"));
    r[1] = rec[1]; r[1].n_bins = RAYS_DEP_MAX_BINS + 1;
    CHECK(refused(host(1, 2, r), "n_bins = 321 is outside 1..320"));
    r[1] = rec[1]; r[1].which = RAYS_DEP_PTOTAL_X;
    CHECK(refused(host(1, 2, r), "unimplemented profile for this equilib_model"));
    r[1] = rec[1]; r[1].profile_in = d1.data();
    CHECK(refused(host(1, 2, r), "rays_hip_trace_profiles: profile_in is for the device form"));
    r[1] = rec[1]; r[1].profile = nullptr;
    CHECK(refused(host(1, 2, r), "rays_hip_trace_profiles: null array argument"));
    CHECK(refused(rays_hip_trace_profiles(&p, 1, r0.data(), n0.data(), nullptr, 2, rec, i1.data(), i1.data(), nullptr, d1.data(),
                                          d1.data(), d1.data(), nullptr), "rays_hip_trace_profiles: null array argument"));
    // the device form: work and profile are required in every record
    auto dev = [&](int n_profiles, const rays_dep_profile_t* q) {
      return rays_hip_trace_profiles_device(&p, 1, d1.data(), d1.data(), d1.data(), n_profiles, q, i1.data(), i1.data(), nullptr,
                                            d1.data(), d1.data(), d1.data(), nullptr);
    };
    CHECK(refused(dev(2, rec), "rays_hip_trace_profiles_device: null work or profile"));
    CHECK(refused(dev(1, rec), "rays_hip_trace_profiles_device: null work or profile"));
    r[0] = rec[0]; r[1] = rec[1]; r[0].work = r[1].work = d1.data(); r[1].profile = nullptr;
    CHECK(refused(dev(2, r), "rays_hip_trace_profiles_device: null work or profile"));
    r[1].profile = d1.data();
    CHECK(refused(rays_hip_trace_profiles_device(&p, 1, nullptr, nullptr, nullptr, 2, r, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr), "rays_hip_trace_profiles_device: null device pointer"));
    CHECK(refused(rays_hip_trace_profiles_device(nullptr, 1, nullptr, nullptr, nullptr, 2, r, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, nullptr), "rays_hip_trace_profiles_device: null parameter block"));
    // two profiles on a configuration that has one: the single-profile entry's own message for the record it lacks
    rays_params_t q = p;
    q.axisym.magnetics_model = RAYS_AXI_MAG_EQDSK_LIN;
    if (rays_hip_check_params(&q) == 0) {
      CHECK(rays_hip_deposition_profile_set(&q, set) == 1 && set[0] == RAYS_DEP_PTOTAL_PSI);
      CHECK(refused(rays_hip_trace_profiles(&q, 1, r0.data(), n0.data(), pw.data(), 2, rec, i1.data(), i1.data(), nullptr,
                                            d1.data(), d1.data(), d1.data(), nullptr),
                    "axisym_toroid_rho: rho is only implemented for eqdsk_magnetics_spline_interp"));
    } else {
      std::fprintf(stderr, "the eqdsk_magnetics_lin_interp twin of the case is refused: %s\n", last_error().c_str());
      failures++;
    }
  }
  for (double x : d1) CHECK(x == -7.);
  CHECK(std::strcmp(rays_hip_profiles_kernel_name_for(&p, (int)nray, 2), "rk4_trace_kernel<358, 2, 0, 8>") == 0);
  CHECK(std::strcmp(rays_hip_profiles_kernel_name_for(&p, (int)nray, 1), "rk4_trace_kernel<102, 2, 0, 8>") == 0);
  CHECK(std::strcmp(rays_hip_profiles_kernel_name_for(&p, (int)nray, 3), "") == 0);

  long long launches = 0, wrong = 0, live = -1, pinned = -1, streams = -1, events = -1;
  rays_emul_runtime_stats(&launches, &wrong, &live);
  CHECK(wrong == 0 && live > 0);   // (the entry's cached blocks, the argument blocks and the refill counters are still held)
  CHECK(rays_hip_finalize() == 0);
  rays_emul_runtime_stats(&launches, &wrong, &live);
  rays_emul_runtime_live(&pinned, &streams, &events);
  CHECK(live == 0 && pinned == 0 && streams == 0 && events == 0 && wrong == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("profiles capi ok: %d calls, %lld launches\n", calls, launches);
  return 0;
}
