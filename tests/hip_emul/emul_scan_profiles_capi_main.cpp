// TEST INFRASTRUCTURE ONLY: segmented deposition (rays_hip_scan_profiles_device, rays_hip_trace_profiles_segments_device,
// rays_hip_profile_sum_segments_device; rays_amd/csrc/rays_capi.hip) as a stand-alone program on the emulated HIP runtime
// -- for plain and for sanitizer runs (tests/hip_emul/Makefile.scan_profiles, target scan_profiles;
// tests/test_cpu_scan_profiles.py writes the case file, starts the program and compares what it wrote).
//   emul_scan_profiles_capi <case file> <output file>
// Case file (native endianness): int32 nray, nv, n_profiles, n_bins_a, n_bins_b, which_a, which_b, nx,
// sizeof(rays_params_t), n_runs, axisym, n_seg; the parameter block; real64 x_min, x_max, fspl_re[nx][4] (the Z-function
// table); if axisym: int32 nr, nz, n_rb, n_ne, n_te, n_ti and the eleven arrays of rays_axisym_tables_t, each behind its
// int32 length; int32 n_rho, rho_grid[n_rho], rho_fspl[n_rho][4]; rvec0[nray][3], rindex_vec0[nray][3], power[nray],
// ds[n_runs], int32 seg_offsets[n_seg + 1].
// Output file: (1) the scan: npoints, stop_code (int32), start_ray_vec, end_ray_vec, end_residuals, max_residuals, each
// [n_runs * nray] rows, then per record work[n_bins][n_runs * nray] and profile[n_runs][n_bins]; (2) per record the
// profile[n_runs][n_bins] of the scan of the last 3/8 of the members continued from the scan of the first 5/8; (3) the
// segments call: the six summaries [nray], then per record work[n_bins][nray] and profile[n_seg][n_bins].
// The program itself checks what needs no expected values: nothing behind the arrays' ends is touched, n_runs == 0 and
// nray == 0, a repeated call allocates nothing, the refusals by name with every output left alone, and after
// rays_hip_finalize the emulated driver holds nothing.
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
hipError_t launch_profile_sum_segments(int n_bins, int nray, int n_seg, const int* d_off, int rays_per_seg,
                                       const double* work, const double* carry, double* profile, hipStream_t) {
  for (int sg = 0; sg < n_seg; sg++) {
    long long r0 = d_off ? d_off[sg] : (long long)sg * rays_per_seg;
    long long r1 = d_off ? d_off[sg + 1] : r0 + rays_per_seg;
    r0 = r0 < 0 ? 0 : r0 > nray ? nray : r0;
    r1 = r1 < 0 ? 0 : r1 > nray ? nray : r1;
    if (r1 < r0) r1 = r0;
    for (int b = 0; b < n_bins; b++) {
      double s = carry ? carry[(size_t)sg * n_bins + b] : 0.;
      for (long long r = r0; r < r1; r++) s = s + work[(size_t)b * nray + r];
      profile[(size_t)sg * n_bins + b] = s;
    }
  }
  return hipSuccess;
}
hipError_t launch_tile_power(int nray, long long total, const double* power, double* power_runs, hipStream_t) {
  for (long long i = 0; i < total; i++) power_runs[i] = power[i % nray];
  return hipSuccess;
}
}  // namespace rays

extern "C" void rays_emul_runtime_stats(long long* launches, long long* wrong_device, long long* live_allocations);
extern "C" void rays_emul_runtime_live(long long* pinned, long long* streams, long long* events);

static bool read_array(std::FILE* f, std::vector<double>& v) {
  int32_t n = 0;
  return std::fread(&n, sizeof n, 1, f) == 1 && n >= 0 && read_n(f, v, (size_t)n);
}

// n elements of emulated device memory + one behind them, all holding `fill`; host() copies them back
template <class T>
struct Dev {
  T* p = nullptr;
  size_t n = 0;
  T fill;
  Dev(size_t n_, T fill_) : n(n_), fill(fill_) {
    std::vector<T> h(n + 1, fill);
    CHECK(hipMalloc(&p, sizeof(T) * (n + 1)) == hipSuccess);
    CHECK(hipMemcpy(p, h.data(), sizeof(T) * (n + 1), hipMemcpyHostToDevice) == hipSuccess);
  }
  explicit Dev(const std::vector<T>& h) : n(h.size()), fill(T()) {
    CHECK(hipMalloc(&p, sizeof(T) * (n + 1)) == hipSuccess);
    CHECK(hipMemcpy(p, h.data(), sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(p + n, &fill, sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  }
  ~Dev() { (void)hipFree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  std::vector<T> host() const {
    std::vector<T> h(n + 1);
    CHECK(hipMemcpy(h.data(), p, sizeof(T) * (n + 1), hipMemcpyDeviceToHost) == hipSuccess);
    return h;
  }
  bool untouched() const {
    for (const T& x : host())
      if (std::memcmp(&x, &fill, sizeof(T)) != 0) return false;
    return true;
  }
  // the n elements to `f`; the one behind them still holds the fill
  void write(std::FILE* f) const {
    const std::vector<T> h = host();
    CHECK(std::memcmp(&h[n], &fill, sizeof(T)) == 0);
    CHECK(n == 0 || std::fwrite(h.data(), sizeof(T), n, f) == n);
  }
};

// the six summaries of `rows` rays
struct Summaries {
  Dev<int32_t> np, sc;
  Dev<double> start, end, er, mr;
  Summaries(size_t rows, size_t nv) : np(rows, -7), sc(rows, -7), start(rows * nv, -7.), end(rows * nv, -7.), er(rows, -7.), mr(rows, -7.) {}
  void write(std::FILE* f) const { np.write(f); sc.write(f); start.write(f); end.write(f); er.write(f); mr.write(f); }
  bool untouched() const {
    return np.untouched() && sc.untouched() && start.untouched() && end.untouched() && er.untouched() && mr.untouched();
  }
};

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <output file>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t head[12];
  if (std::fread(head, sizeof head, 1, f) != 1 || head[8] != rays_hip_sizeof_params()) {
    std::fprintf(stderr, "case file does not match this library's rays_params_t\n");
    return 2;
  }
  const size_t nray = (size_t)head[0], nv = (size_t)head[1];
  const int n_prof = head[2], which[2] = {head[5], head[6]}, nx = head[7], n_runs = head[9], n_seg = head[11];
  const size_t nb[2] = {(size_t)head[3], (size_t)head[4]};
  const bool axisym = head[10] != 0;
  rays_params_t p;
  double zr[2];
  int32_t tn[6] = {0, 0, 0, 0, 0, 0}, n_rho = 0;
  std::vector<double> zf, tab[11], rho_grid, rho_fspl, r0, n0, pw, ds;
  std::vector<int32_t> seg;
  bool ok = std::fread(&p, sizeof p, 1, f) == 1 && std::fread(zr, sizeof zr, 1, f) == 1 && read_n(f, zf, 4 * (size_t)nx);
  if (ok && axisym) {
    ok = std::fread(tn, sizeof tn, 1, f) == 1;
    for (int k = 0; ok && k < 11; k++) ok = read_array(f, tab[k]);
  }
  ok = ok && std::fread(&n_rho, sizeof n_rho, 1, f) == 1 && read_n(f, rho_grid, (size_t)n_rho) &&
       read_n(f, rho_fspl, 4 * (size_t)n_rho) && read_n(f, r0, 3 * nray) && read_n(f, n0, 3 * nray) && read_n(f, pw, nray) &&
       read_n(f, ds, (size_t)n_runs) && read_n(f, seg, (size_t)n_seg + 1);
  std::fclose(f);
  if (!ok || (int)nv != p.nv || n_prof < 1 || n_prof > 2 || n_runs < 1) { std::fprintf(stderr, "short or inconsistent case file\n"); return 2; }
  CHECK(rays_hip_set_zfun_table(zf.data(), nx, zr[0], zr[1]) == 0);
  if (axisym) {
    rays_axisym_tables_t T;
    std::memset(&T, 0, sizeof T);
    T.nr = tn[0]; T.nz = tn[1]; T.n_rb = tn[2]; T.n_ne = tn[3]; T.n_te = tn[4]; T.n_ti = tn[5];
    auto ptr = [&](int k) -> const double* { return tab[k].empty() ? nullptr : tab[k].data(); };
    T.r_grid = ptr(0); T.z_grid = ptr(1); T.psi_fspl = ptr(2); T.rb_grid = ptr(3); T.rb_fspl = ptr(4); T.ne_grid = ptr(5);
    T.ne_fspl = ptr(6); T.te_grid = ptr(7); T.te_fspl = ptr(8); T.ti_grid = ptr(9); T.ti_fspl = ptr(10);
    CHECK(rays_hip_set_axisym_tables(&T) == 0);
  }
  if (n_rho > 0) CHECK(rays_hip_set_rho_table(rho_grid.data(), rho_fspl.data(), n_rho) == 0);
  CHECK(rays_hip_init(1) >= 0);
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }

  const size_t R = (size_t)n_runs, total = R * nray;
  long long launches = 0, wrong = 0, live = -1, live2 = -1;
  {
    Dev<double> d_r0(r0), d_n0(n0), d_pw(pw), d_ds(ds);
    Dev<int32_t> d_seg(seg);
    // ---- (1) the scan, twice: the second call has every block it needs and allocates nothing
    {
      Summaries S(total, nv);
      Dev<double> work[2] = {Dev<double>(nb[0] * total, -7.), Dev<double>(n_prof == 2 ? nb[1] * total : 0, -7.)};
      Dev<double> prof[2] = {Dev<double>(R * nb[0], -7.), Dev<double>(n_prof == 2 ? R * nb[1] : 0, -7.)};
      rays_dep_profile_t rec[2];
      for (int i = 0; i < n_prof; i++) rec[i] = {which[i], (int)nb[i], work[i].p, nullptr, prof[i].p};
      for (int pass = 0; pass < 2; pass++) {
        const int rc = rays_hip_scan_profiles_device(&p, n_runs, d_ds.p, (int)nray, d_r0.p, d_n0.p, d_pw.p, n_prof, rec, S.np.p,
                                                     S.sc.p, S.start.p, S.end.p, S.er.p, S.mr.p, nullptr);
        if (rc) std::fprintf(stderr, "rays_hip_scan_profiles_device: rc %d: %s\n", rc, last_error().c_str());
        CHECK(rc == 0);
        rays_emul_runtime_stats(&launches, &wrong, pass == 0 ? &live : &live2);
      }
      CHECK(live == live2 && wrong == 0);
      S.write(out);
      for (int i = 0; i < n_prof; i++) { work[i].write(out); prof[i].write(out); }
    }
    // ---- (2) member blocks chained per run: the first 5/8 of the members, then the rest continued from their profiles
    {
      const size_t h = nray * 5 / 8, rest = nray - h;
      Dev<double> prof[2] = {Dev<double>(R * nb[0], -7.), Dev<double>(n_prof == 2 ? R * nb[1] : 0, -7.)};
      for (int part = 0; part < 2; part++) {
        const size_t n = part == 0 ? h : rest, at = part == 0 ? 0 : h;
        Summaries S(R * n, nv);
        Dev<double> work[2] = {Dev<double>(nb[0] * R * n, -7.), Dev<double>(n_prof == 2 ? nb[1] * R * n : 0, -7.)};
        rays_dep_profile_t rec[2];
        // (in place: profile_in == profile from the second block on)
        for (int i = 0; i < n_prof; i++) rec[i] = {which[i], (int)nb[i], work[i].p, part == 0 ? nullptr : prof[i].p, prof[i].p};
        CHECK(rays_hip_scan_profiles_device(&p, n_runs, d_ds.p, (int)n, d_r0.p + 3 * at, d_n0.p + 3 * at, d_pw.p + at, n_prof, rec,
                                            S.np.p, S.sc.p, nullptr, S.end.p, S.er.p, S.mr.p, nullptr) == 0);
        CHECK(S.start.untouched());   // start_ray_vec is optional
      }
      for (int i = 0; i < n_prof; i++) prof[i].write(out);
    }
    // ---- (3) one profile per segment of the fan at the run's own ds
    {
      Summaries S(nray, nv);
      Dev<double> work[2] = {Dev<double>(nb[0] * nray, -7.), Dev<double>(n_prof == 2 ? nb[1] * nray : 0, -7.)};
      Dev<double> prof[2] = {Dev<double>((size_t)n_seg * nb[0], -7.), Dev<double>(n_prof == 2 ? (size_t)n_seg * nb[1] : 0, -7.)};
      rays_dep_profile_t rec[2];
      for (int i = 0; i < n_prof; i++) rec[i] = {which[i], (int)nb[i], work[i].p, nullptr, prof[i].p};
      const int rc = rays_hip_trace_profiles_segments_device(&p, (int)nray, d_r0.p, d_n0.p, d_pw.p, n_prof, rec, n_seg, d_seg.p, 0,
                                                             S.np.p, S.sc.p, S.start.p, S.end.p, S.er.p, S.mr.p, nullptr);
      if (rc) std::fprintf(stderr, "rays_hip_trace_profiles_segments_device: rc %d: %s\n", rc, last_error().c_str());
      CHECK(rc == 0);
      S.write(out);
      for (int i = 0; i < n_prof; i++) { work[i].write(out); prof[i].write(out); }
      // the sum on its own, from the work just written: the same rows
      for (int i = 0; i < n_prof; i++) {
        Dev<double> again((size_t)n_seg * nb[i], -7.);
        CHECK(rays_hip_profile_sum_segments_device((int)nb[i], (int)nray, n_seg, d_seg.p, 0, work[i].p, nullptr, again.p, nullptr) == 0);
        const std::vector<double> a = again.host(), b = prof[i].host();
        CHECK(std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
      }
    }
    // ---- no run: nothing is written; no ray: the carried profiles, or zeros
    {
      Summaries S(4, nv);
      Dev<double> work(nb[0] * 4, -7.), prof(2 * nb[0], -7.), carry(2 * nb[0], 1.5);
      rays_dep_profile_t rec[2] = {{which[0], (int)nb[0], work.p, nullptr, prof.p}, {which[1], (int)nb[1], work.p, nullptr, prof.p}};
      CHECK(rays_hip_scan_profiles_device(&p, 0, nullptr, 2, d_r0.p, d_n0.p, d_pw.p, 1, rec, S.np.p, S.sc.p, S.start.p, S.end.p,
                                          S.er.p, S.mr.p, nullptr) == 0);
      CHECK(S.untouched() && work.untouched() && prof.untouched());
      CHECK(rays_hip_scan_profiles_device(&p, 2, d_ds.p, 0, nullptr, nullptr, nullptr, 1, rec, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr) == 0);
      std::vector<double> h = prof.host();
      for (size_t k = 0; k < 2 * nb[0]; k++) CHECK(h[k] == 0. && !std::signbit(h[k]));
      CHECK(h[2 * nb[0]] == -7.);
      rec[0].profile_in = carry.p;
      CHECK(rays_hip_scan_profiles_device(&p, 2, d_ds.p, 0, nullptr, nullptr, nullptr, 1, rec, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr) == 0);
      h = prof.host();
      for (size_t k = 0; k < 2 * nb[0]; k++) CHECK(h[k] == 1.5);
      CHECK(S.untouched() && work.untouched());
    }
    // ---- refusals, by name; nothing is written
    {
      Summaries S(4, nv);
      Dev<double> d(nb[0] + nb[1] + 64, -7.);
      const rays_dep_profile_t good[2] = {{which[0], (int)nb[0], d.p, nullptr, d.p}, {which[1], (int)nb[1], d.p, nullptr, d.p}};
      auto scan = [&](int runs, int n, int n_profiles, const rays_dep_profile_t* r, const double* dsv) {
        return rays_hip_scan_profiles_device(&p, runs, dsv, n, d_r0.p, d_n0.p, d_pw.p, n_profiles, r, S.np.p, S.sc.p, S.start.p,
                                             S.end.p, S.er.p, S.mr.p, nullptr);
      };
      auto segs = [&](int n, int n_profiles, const rays_dep_profile_t* r, int ns, const int32_t* off, int per) {
        return rays_hip_trace_profiles_segments_device(&p, n, d_r0.p, d_n0.p, d_pw.p, n_profiles, r, ns, off, per, S.np.p, S.sc.p,
                                                       S.start.p, S.end.p, S.er.p, S.mr.p, nullptr);
      };
      CHECK(refused(scan(-1, 1, n_prof, good, d_ds.p), "rays_hip_scan_profiles_device: n_runs < 0"));
      CHECK(refused(scan(1 << 16, 1 << 15, n_prof, good, d_ds.p), "rays_hip_scan_profiles_device: n_runs * nray exceeds 2^31 - 1"));
      CHECK(refused(scan(2, 1, n_prof, good, nullptr), "rays_hip_scan_profiles_device: null d_ds_values"));
      CHECK(refused(scan(2, -1, n_prof, good, d_ds.p), "rays_hip_scan_profiles_device: nray < 0"));
      CHECK(refused(scan(2, 1, 0, good, d_ds.p), "rays_hip_scan_profiles_device: n_profiles = 0 is outside 1..2"));
      CHECK(refused(scan(2, 1, 3, good, d_ds.p), "rays_hip_scan_profiles_device: n_profiles = 3 is outside 1..2"));
      CHECK(refused(scan(2, 1, n_prof, nullptr, d_ds.p), "rays_hip_scan_profiles_device: null profile list"));
      CHECK(refused(rays_hip_scan_profiles_device(nullptr, 2, d_ds.p, 1, d_r0.p, d_n0.p, d_pw.p, n_prof, good, S.np.p, S.sc.p, S.start.p,
                                                  S.end.p, S.er.p, S.mr.p, nullptr), "rays_hip_scan_profiles_device: null parameter block"));
      CHECK(refused(rays_hip_scan_profiles_device(&p, 2, d_ds.p, 1, nullptr, d_n0.p, d_pw.p, n_prof, good, S.np.p, S.sc.p, S.start.p,
                                                  S.end.p, S.er.p, S.mr.p, nullptr), "rays_hip_scan_profiles_device: null device pointer"));
      rays_dep_profile_t r[2] = {good[0], good[1]};
      r[0].n_bins = 0;
      CHECK(refused(scan(2, 1, n_prof, r, d_ds.p), "n_bins = 0 is outside 1..320"));
      r[0].n_bins = RAYS_DEP_MAX_BINS + 1;
      CHECK(refused(scan(2, 1, n_prof, r, d_ds.p), "n_bins = 321 is outside 1..320"));
      r[0] = good[0]; r[0].which = axisym ? RAYS_DEP_PTOTAL_X : RAYS_DEP_PTOTAL_PSI;
      CHECK(refused(scan(2, 1, n_prof, r, d_ds.p), "unimplemented profile for this equilib_model"));
      r[0] = good[0]; r[0].work = nullptr;
      CHECK(refused(scan(2, 1, n_prof, r, d_ds.p), "rays_hip_scan_profiles_device: null work or profile"));
      r[0] = good[0]; r[0].profile = nullptr;
      CHECK(refused(scan(2, 1, n_prof, r, d_ds.p), "rays_hip_scan_profiles_device: null work or profile"));
      if (n_prof == 2) {
        r[0] = good[0]; r[1] = good[0];
        CHECK(refused(scan(2, 1, 2, r, d_ds.p), "rays_hip_scan_profiles_device: the same profile twice"));
      } else {   // a slab has one profile: the second record is refused with the single-profile entry's message
        r[0] = good[0]; r[1] = good[0]; r[1].which = RAYS_DEP_PTOTAL_PSI;
        CHECK(refused(scan(2, 1, 2, r, d_ds.p), "unimplemented profile for this equilib_model"));
      }
      CHECK(refused(segs(1, n_prof, good, -1, d_seg.p, 0), "rays_hip_trace_profiles_segments_device: n_seg < 0"));
      CHECK(refused(segs(1, n_prof, good, 2, nullptr, 0),
                    "rays_hip_trace_profiles_segments_device: neither segment offsets nor a positive rays_per_seg"));
      CHECK(refused(segs(1, n_prof, good, 2, nullptr, -4),
                    "rays_hip_trace_profiles_segments_device: neither segment offsets nor a positive rays_per_seg"));
      CHECK(refused(segs(-1, n_prof, good, 2, nullptr, 1), "rays_hip_trace_profiles_segments_device: nray < 0"));
      CHECK(refused(segs(1, 3, good, 2, nullptr, 1), "rays_hip_trace_profiles_segments_device: n_profiles = 3 is outside 1..2"));
      r[0] = good[0]; r[1] = good[1]; r[0].work = nullptr;
      CHECK(refused(segs(1, n_prof, r, 2, nullptr, 1), "rays_hip_trace_profiles_segments_device: null work or profile"));
      CHECK(refused(rays_hip_profile_sum_segments_device(4, 4, -1, nullptr, 1, d.p, nullptr, d.p, nullptr),
                    "rays_hip_profile_sum_segments_device: n_seg < 0"));
      CHECK(refused(rays_hip_profile_sum_segments_device(4, 4, 2, nullptr, 0, d.p, nullptr, d.p, nullptr),
                    "rays_hip_profile_sum_segments_device: neither segment offsets nor a positive rays_per_seg"));
      CHECK(refused(rays_hip_profile_sum_segments_device(0, 4, 2, nullptr, 1, d.p, nullptr, d.p, nullptr),
                    "rays_hip_profile_sum_segments_device: n_bins < 1"));
      CHECK(refused(rays_hip_profile_sum_segments_device(4, -1, 2, nullptr, 1, d.p, nullptr, d.p, nullptr),
                    "rays_hip_profile_sum_segments_device: nray < 0"));
      CHECK(refused(rays_hip_profile_sum_segments_device(4, 4, 2, nullptr, 1, nullptr, nullptr, d.p, nullptr),
                    "rays_hip_profile_sum_segments_device: null work or profile"));
      CHECK(S.untouched() && d.untouched());
    }
  }
  CHECK(std::fclose(out) == 0);
  long long pinned = -1, streams = -1, events = -1;
  rays_emul_runtime_stats(&launches, &wrong, &live);
  CHECK(wrong == 0 && live > 0);   // (the argument blocks with the tiled weights and the refill counters are still held)
  CHECK(rays_hip_finalize() == 0);
  rays_emul_runtime_stats(&launches, &wrong, &live);
  rays_emul_runtime_live(&pinned, &streams, &events);
  CHECK(live == 0 && pinned == 0 && streams == 0 && events == 0 && wrong == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("scan profiles capi ok: %lld launches\n", launches);
  return 0;
}
