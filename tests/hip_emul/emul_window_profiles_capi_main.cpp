// TEST INFRASTRUCTURE ONLY: deposition windows through the product's C ABI (rays_hip_trace_window_profiles_device,
// rays_amd/csrc/rays_capi.hip) as a stand-alone program on the emulated HIP runtime -- for plain and for sanitizer runs
// (tests/hip_emul/Makefile.window_profiles, target window_profiles; tests/test_cpu_window_deposition.py writes the case
// file and starts it).
//   emul_window_profiles_capi <case file>
// Case file: the one of emul_profiles_capi_main.cpp (tests/test_cpu_fused_profiles.py: _case_file) -- the parameter
// block, the tables, the rays with their powers, and what the one-lane emulation of the ONE-SHOT two-profile kernel gave
// for them: the summaries and work_a[nray][n_bins_a], work_b[nray][n_bins_b].
// From rays_hip_state_init_device and zeroed works, windows of 7, 1 and 13 steps (cycled) to the end of every ray must
// reproduce those bytes -- with two records, and with one record for either profile -- in work rows that are allocated
// to their exact size (a store behind a row is the sanitizer's, or the poisoned neighbour's, to find); the profile is
// summed only where the record asks for it; calls after every ray has ended change nothing; every refusal is checked
// by its message and writes nothing; after rays_hip_finalize the emulated driver holds nothing.
#define RAYS_EMUL_RUNTIME 1
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

static const double kPoison = -7.;
static bool read_array(std::FILE* f, std::vector<double>& v) {
  int32_t n = 0;
  return std::fread(&n, sizeof n, 1, f) == 1 && n >= 0 && read_n(f, v, (size_t)n);
}
template <class T>
static T* dev_alloc(size_t n) {
  T* p = nullptr;
  if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); std::exit(2); }
  return p;
}
// the saved state, every array poisoned and exactly sized
struct State {
  rays_ray_state_t S;
  size_t n, nv;
  State(size_t n_, size_t nv_) : n(n_), nv(nv_) {
    S.v = dev_alloc<double>(nv * n); S.s = dev_alloc<double>(n); S.nstep = dev_alloc<int32_t>(n);
    S.stop_code = dev_alloc<int32_t>(n); S.resid = dev_alloc<double>(3 * n); S.sg_err = dev_alloc<double>(2 * n);
    S.flags = dev_alloc<int32_t>(n);
    std::memset(S.v, 0x7f, 8 * nv * n); std::memset(S.s, 0x7f, 8 * n); std::memset(S.nstep, 0x7f, 4 * n);
    std::memset(S.stop_code, 0x7f, 4 * n); std::memset(S.resid, 0x7f, 24 * n); std::memset(S.sg_err, 0x7f, 16 * n);
    std::memset(S.flags, 0x7f, 4 * n);
  }
  ~State() {
    hipFree(S.v); hipFree(S.s); hipFree(S.nstep); hipFree(S.stop_code); hipFree(S.resid); hipFree(S.sg_err); hipFree(S.flags);
  }
  std::string bytes() const {
    std::string b;
    b.append((const char*)S.v, 8 * nv * n); b.append((const char*)S.s, 8 * n); b.append((const char*)S.nstep, 4 * n);
    b.append((const char*)S.stop_code, 4 * n); b.append((const char*)S.resid, 24 * n); b.append((const char*)S.sg_err, 16 * n);
    b.append((const char*)S.flags, 4 * n);
    return b;
  }
  bool under_way() const {
    for (size_t i = 0; i < n; i++)
      if (S.stop_code[i] == RAYS_STOP_NONE) return true;
    return false;
  }
};
// work[nray][nb] (the case file's layout) against the device's bin-major rows of the first n rays
static bool same_rows(const std::vector<double>& ref, const double* work, size_t nb, size_t n) {
  for (size_t r = 0; r < n; r++)
    for (size_t b = 0; b < nb; b++)
      if (std::memcmp(&ref[r * nb + b], &work[b * n + r], sizeof(double)) != 0) return false;
  return true;
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
  CHECK(rays_hip_set_zfun_table(zf.data(), nx, zr[0], zr[1]) == 0);
  rays_axisym_tables_t T;
  std::memset(&T, 0, sizeof T);
  T.nr = tn[0]; T.nz = tn[1]; T.n_rb = tn[2]; T.n_ne = tn[3]; T.n_te = tn[4]; T.n_ti = tn[5];
  auto ptr = [&](int k) -> const double* { return tab[k].empty() ? nullptr : tab[k].data(); };
  T.r_grid = ptr(0); T.z_grid = ptr(1); T.psi_fspl = ptr(2); T.rb_grid = ptr(3); T.rb_fspl = ptr(4); T.ne_grid = ptr(5);
  T.ne_fspl = ptr(6); T.te_grid = ptr(7); T.te_fspl = ptr(8); T.ti_grid = ptr(9); T.ti_fspl = ptr(10);
  CHECK(rays_hip_set_axisym_tables(&T) == 0);
  const int one[] = {0};
  CHECK(rays_hip_init_devices(1, one) >= 0);
  CHECK(hipSetDevice(0) == hipSuccess);

  const size_t n = nray;
  double *d_r0 = dev_alloc<double>(3 * n), *d_n0 = dev_alloc<double>(3 * n), *d_pw = dev_alloc<double>(n);
  CHECK(hipMemcpy(d_r0, r0.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_n0, n0.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_pw, pw.data(), sizeof(double) * n, hipMemcpyHostToDevice) == hipSuccess);
  int32_t* d_npw = dev_alloc<int32_t>(n);
  // exactly sized work rows and profiles (a store behind them is out of the allocation)
  double* d_work[2] = {dev_alloc<double>(nb[0] * n), dev_alloc<double>(nb[1] * n)};
  double* d_prof[2] = {dev_alloc<double>(nb[0]), dev_alloc<double>(nb[1])};

  // before the rho table is set the rho record is refused by name
  {
    State st(n, nv);
    const rays_dep_profile_t rec[2] = {{which[0], (int)nb[0], d_work[0], nullptr, d_prof[0]},
                                       {which[1], (int)nb[1], d_work[1], nullptr, d_prof[1]}};
    CHECK(refused(rays_hip_trace_window_profiles_device(&p, (int)n, &st.S, 5, d_pw, 2, rec, d_npw, nullptr),
                  "Ptotal_rho needs rays_hip_set_rho_table() first"));
  }
  CHECK(rays_hip_set_rho_table(rho_grid.data(), rho_fspl.data(), n_rho) == 0);

  int windows_run = 0;
  // records: both profiles, both in the other order, each alone
  const int sets[][2] = {{0, 1}, {1, 0}, {0, -1}, {1, -1}};
  for (const auto& set : sets) {
    const int k = set[1] < 0 ? 1 : 2;
    State st(n, nv);
    std::vector<double> o_start(nv * n + 1, kPoison);
    double* d_start = dev_alloc<double>(nv * n);
    CHECK(rays_hip_state_init_device(&p, (int)n, d_r0, d_n0, &st.S, d_start, nullptr) == 0);
    CHECK(std::memcmp(d_start, start.data(), sizeof(double) * nv * n) == 0);
    CHECK(hipFree(d_start) == hipSuccess);
    for (int i = 0; i < 2; i++) {
      std::memset(d_work[i], 0, sizeof(double) * nb[i] * n);
      for (size_t b = 0; b < nb[i]; b++) d_prof[i][b] = kPoison;
    }
    const int sizes[] = {7, 1, 13};
    std::vector<long long> have(n, 1);
    int w = 0;
    for (; st.under_way() && w < 100000; w++) {
      // the profile is summed in every third window only; elsewhere the record's profile is null and stays untouched
      const bool sum = w % 3 == 2;
      rays_dep_profile_t rec[2];
      for (int j = 0; j < k; j++)
        rec[j] = rays_dep_profile_t{which[set[j]], (int)nb[set[j]], d_work[set[j]], nullptr, sum ? d_prof[set[j]] : nullptr};
      std::vector<double> prof_before(d_prof[set[0]], d_prof[set[0]] + nb[set[0]]);
      const int rc = rays_hip_trace_window_profiles_device(&p, (int)n, &st.S, sizes[w % 3], d_pw, k, rec, d_npw, nullptr);
      if (rc) std::fprintf(stderr, "rays_hip_trace_window_profiles_device: rc %d: %s\n", rc, last_error().c_str());
      CHECK(rc == 0);
      if (rc) break;
      if (!sum) CHECK(std::memcmp(prof_before.data(), d_prof[set[0]], sizeof(double) * nb[set[0]]) == 0);
      for (size_t i = 0; i < n; i++) {
        CHECK(d_npw[i] >= 0 && d_npw[i] <= sizes[w % 3]);
        have[i] += d_npw[i];
      }
    }
    windows_run += w;
    CHECK(w >= 3);
    for (size_t i = 0; i < n; i++) CHECK(have[i] == np[i]);
    // the works equal the one-shot pass's; the profile of a last summing call is the ray-ordered sum
    rays_dep_profile_t rec[2];
    for (int j = 0; j < k; j++)
      rec[j] = rays_dep_profile_t{which[set[j]], (int)nb[set[j]], d_work[set[j]], nullptr, d_prof[set[j]]};
    const std::string before = st.bytes();
    std::vector<double> w_before[2] = {std::vector<double>(d_work[0], d_work[0] + nb[0] * n),
                                       std::vector<double>(d_work[1], d_work[1] + nb[1] * n)};
    // calls after every ray has ended: no byte of the state or the works changes, npoints_win = 0
    for (int again = 0; again < 2; again++) {
      CHECK(rays_hip_trace_window_profiles_device(&p, (int)n, &st.S, 5, d_pw, k, rec, d_npw, nullptr) == 0);
      for (size_t i = 0; i < n; i++) CHECK(d_npw[i] == 0);
      CHECK(st.bytes() == before);
      for (int j = 0; j < k; j++)
        CHECK(std::memcmp(w_before[set[j]].data(), d_work[set[j]], sizeof(double) * nb[set[j]] * n) == 0);
    }
    for (int j = 0; j < k; j++) {
      const int i = set[j];
      CHECK(same_rows(work[i], d_work[i], nb[i], n));
      for (size_t b = 0; b < nb[i]; b++) {
        double s = 0.;
        for (size_t r = 0; r < n; r++) s = s + work[i][r * nb[i] + b];
        CHECK(std::memcmp(&s, &d_prof[i][b], sizeof s) == 0);
      }
    }
    // the state's summaries are the one-shot pass's
    std::vector<int32_t> o_np(n), o_sc(n);
    std::vector<double> o_end(nv * n), o_er(n), o_mr(n);
    int32_t *d_np = dev_alloc<int32_t>(n), *d_sc = dev_alloc<int32_t>(n);
    double *d_end = dev_alloc<double>(nv * n), *d_er = dev_alloc<double>(n), *d_mr = dev_alloc<double>(n);
    CHECK(rays_hip_state_summary_device(&p, (int)n, &st.S, d_np, d_sc, d_end, d_er, d_mr, nullptr) == 0);
    CHECK(std::memcmp(d_np, np.data(), 4 * n) == 0 && std::memcmp(d_sc, sc.data(), 4 * n) == 0);
    CHECK(std::memcmp(d_end, end.data(), 8 * nv * n) == 0 && std::memcmp(d_er, eres.data(), 8 * n) == 0 &&
          std::memcmp(d_mr, mres.data(), 8 * n) == 0);
    hipFree(d_np); hipFree(d_sc); hipFree(d_end); hipFree(d_er); hipFree(d_mr);
  }

  // refusals, by name; nothing is written
  {
    State st(n, nv);
    const std::string before = st.bytes();
    for (int i = 0; i < 2; i++) {
      for (size_t b = 0; b < nb[i] * n; b++) d_work[i][b] = kPoison;
      for (size_t b = 0; b < nb[i]; b++) d_prof[i][b] = kPoison;
    }
    for (size_t i = 0; i < n; i++) d_npw[i] = -7;
    const rays_dep_profile_t rec[2] = {{which[0], (int)nb[0], d_work[0], nullptr, d_prof[0]},
                                       {which[1], (int)nb[1], d_work[1], nullptr, d_prof[1]}};
    const char* who = "rays_hip_trace_window_profiles_device";
    auto call = [&](int nr, const rays_ray_state_t* S, int n_steps, const double* power, int k, const rays_dep_profile_t* r,
                    int32_t* npw) { return rays_hip_trace_window_profiles_device(&p, nr, S, n_steps, power, k, r, npw, nullptr); };
    auto named = [&](const char* tail) { return std::string(who) + tail; };
    CHECK(refused(call((int)n, &st.S, 5, d_pw, 0, rec, d_npw), "n_profiles = 0 is outside 1..2"));
    CHECK(refused(call((int)n, &st.S, 5, d_pw, 3, rec, d_npw), "n_profiles = 3 is outside 1..2"));
    CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, nullptr, d_npw), named(": null profile list").c_str()));
    CHECK(refused(call(-1, &st.S, 5, d_pw, 2, rec, d_npw), named(": nray < 0").c_str()));
    CHECK(refused(call((int)n, &st.S, 0, d_pw, 2, rec, d_npw), named(": n_steps < 1").c_str()));
    CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, rec, nullptr), named(": null device pointer").c_str()));
    CHECK(refused(call((int)n, &st.S, 5, nullptr, 2, rec, d_npw), named(": null initial_ray_power").c_str()));
    CHECK(refused(call((int)n, nullptr, 5, d_pw, 2, rec, d_npw), named(": null pointer in the ray state").c_str()));
    CHECK(refused(call((int)n, &st.S, 0x7fffffff, d_pw, 2, rec, d_npw), named(": nray * n_steps exceeds 2^31 - 1").c_str()));
    {
      rays_ray_state_t S = st.S;
      S.resid = nullptr;
      CHECK(refused(call((int)n, &S, 5, d_pw, 2, rec, d_npw), named(": null pointer in the ray state").c_str()));
      rays_dep_profile_t r[2] = {rec[0], rec[0]};
      CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, r, d_npw), named(": the same profile twice").c_str()));
      r[1] = rec[1]; r[1].n_bins = 0;
      CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, r, d_npw), "n_bins = 0 is outside 1..320"));
      r[1] = rec[1]; r[1].n_bins = RAYS_DEP_MAX_BINS + 1;
      CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, r, d_npw), "n_bins = 321 is outside 1..320"));
      r[1] = rec[1]; r[1].which = RAYS_DEP_PTOTAL_X;
      CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, r, d_npw), "unimplemented profile for this equilib_model"));
      r[1] = rec[1]; r[1].work = nullptr;
      CHECK(refused(call((int)n, &st.S, 5, d_pw, 2, r, d_npw), named(": null work").c_str()));
      CHECK(refused(call((int)n, &st.S, 5, d_pw, 1, &r[1], d_npw), named(": null work").c_str()));
    }
    CHECK(refused(rays_hip_trace_window_profiles_device(nullptr, (int)n, &st.S, 5, d_pw, 2, rec, d_npw, nullptr),
                  named(": null parameter block").c_str()));
    {  // no damping row: the fused entries' own refusal
      rays_params_t q = p;
      q.damping_model = 0;
      q.nv = p.nv - 1;
      CHECK(rays_hip_trace_window_profiles_device(&q, (int)n, &st.S, 5, d_pw, 1, rec, d_npw, nullptr) != 0);
    }
    CHECK(st.bytes() == before);
    for (size_t i = 0; i < n; i++) CHECK(d_npw[i] == -7);
    for (int i = 0; i < 2; i++) {
      for (size_t b = 0; b < nb[i] * n; b++) CHECK(d_work[i][b] == kPoison);
      for (size_t b = 0; b < nb[i]; b++) CHECK(d_prof[i][b] == kPoison);
    }
  }
  CHECK(std::strcmp(rays_hip_window_profiles_kernel_name_for(&p, (int)nray, 1), "rk4_trace_kernel<230, 2, 0, 8>") == 0);
  CHECK(std::strcmp(rays_hip_window_profiles_kernel_name_for(&p, (int)nray, 2), "rk4_trace_kernel<486, 2, 0, 8>") == 0);
  CHECK(std::strcmp(rays_hip_window_profiles_kernel_name_for(&p, (int)nray, 3), "") == 0);
  // the one-shot names do not move
  CHECK(std::strcmp(rays_hip_profiles_kernel_name_for(&p, (int)nray, 2), "rk4_trace_kernel<358, 2, 0, 8>") == 0);
  CHECK(std::strcmp(rays_hip_window_kernel_name_for(&p, (int)nray, 0), "rk4_trace_kernel<166, 2, 0, 8>") == 0);

  hipFree(d_r0); hipFree(d_n0); hipFree(d_pw); hipFree(d_npw);
  for (int i = 0; i < 2; i++) { hipFree(d_work[i]); hipFree(d_prof[i]); }
  long long launches = 0, wrong = 0, live = -1, pinned = -1, streams = -1, events = -1;
  rays_emul_runtime_stats(&launches, &wrong, &live);
  CHECK(wrong == 0 && live > 0);   // (the argument blocks and the refill counters are still held)
  CHECK(rays_hip_finalize() == 0);
  rays_emul_runtime_stats(&launches, &wrong, &live);
  rays_emul_runtime_live(&pinned, &streams, &events);
  CHECK(live == 0 && pinned == 0 && streams == 0 && events == 0 && wrong == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("window profiles capi ok: %d windows, %lld launches\n", windows_run, launches);
  return 0;
}
