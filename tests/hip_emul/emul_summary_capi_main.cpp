// TEST INFRASTRUCTURE ONLY: the host form of summary-only tracing (rays_hip_trace_summary, rays_amd/csrc/rays_capi.hip)
// as a stand-alone program on the emulated HIP runtime with four devices -- for plain and for sanitizer runs
// (tests/hip_emul/Makefile.capi, target summary; tests/test_cpu_summary_trace.py writes the case file and starts it).
//   emul_summary_capi <case file>
// Case file (native endianness): int32 nray, nv, sizeof(rays_params_t); the parameter block; rvec0[nray][3],
// rindex_vec0[nray][3]; then the oracle's summaries of these rays: npoints[nray], stop_code[nray] (int32),
// start_ray_vec[nray][nv], end_ray_vec[nray][nv], end_residuals[nray], max_residuals[nray]; then the oracle's trajectories
// of the same trace, packed to npoints points per ray: ray_vec[sum npoints][nv], residual[sum npoints].
// Every device list of 1 to 4 devices traces the first n rays for several n -- a ragged last block, blocks that are
// empty -- and must reproduce the oracle's bytes; after rays_hip_finalize the emulated driver holds nothing.
// rays_hip_trace does the same on these lists and on one that repeats a device, with and without the kept result, and
// rays_hip_trace_gather on one device: the block workers of both under the sanitizers without a Python host.
#include "emul_capi_check.hpp"

extern "C" void rays_emul_runtime_stats(long long* launches, long long* wrong_device, long long* live_allocations);
extern "C" void rays_emul_runtime_live(long long* pinned, long long* streams, long long* events);

static const double kPoison = -7.;

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t head[3];
  if (std::fread(head, sizeof head, 1, f) != 1 || head[2] != rays_hip_sizeof_params()) {
    std::fprintf(stderr, "case file does not match this library's rays_params_t\n");
    return 2;
  }
  const size_t nray = (size_t)head[0], nv = (size_t)head[1];
  rays_params_t p;
  std::vector<double> r0, n0, start, end, eres, mres;
  std::vector<int32_t> np, sc;
  bool ok = std::fread(&p, sizeof p, 1, f) == 1 && read_n(f, r0, 3 * nray) && read_n(f, n0, 3 * nray) &&
            read_n(f, np, nray) && read_n(f, sc, nray) && read_n(f, start, nv * nray) && read_n(f, end, nv * nray) &&
            read_n(f, eres, nray) && read_n(f, mres, nray);
  Case c;
  c.nv = nv;
  c.npt = (size_t)p.nstep_max + 1;
  c.offs.assign(nray + 1, 0);
  for (size_t i = 0; ok && i < nray; i++) {
    ok = np[i] >= 1 && (size_t)np[i] <= c.npt;
    c.offs[i + 1] = c.offs[i] + (size_t)np[i];
  }
  ok = ok && read_n(f, c.pv, nv * c.offs[nray]) && read_n(f, c.pr, c.offs[nray]);
  std::fclose(f);
  c.np = np; c.sc = sc; c.end = end; c.eres = eres; c.mres = mres;
  if (!ok || (int)nv != p.nv) { std::fprintf(stderr, "short or inconsistent case file\n"); return 2; }
  if (rays_hip_device_count() < 4) { std::fprintf(stderr, "needs 4 emulated devices\n"); return 2; }

  const int lists[][4] = {{0}, {2, 1}, {0, 1, 3}, {0, 1, 2, 3}};
  int calls = 0;
  for (int G = 1; G <= 4; G++) {
    CHECK(rays_hip_init_devices(G, lists[G - 1]) >= 0);
    // all rays (301 over 4 devices: 76, 76, 76, 73 -- a ragged last block); G + 1 rays (5 over 4: 2, 2, 1, 0 -- an
    // empty block); 1 ray (G - 1 empty blocks); none
    const size_t counts[] = {nray, (size_t)G + 1, 1, 0};
    for (size_t n : counts) {
      if (n > nray) continue;
      // poisoned outputs, one element longer than asked for: nothing behind the last ray may be touched
      std::vector<int32_t> o_np(n + 1, -7), o_sc(n + 1, -7);
      std::vector<double> o_start(nv * n + 1, -7.), o_end(nv * n + 1, -7.), o_er(n + 1, -7.), o_mr(n + 1, -7.);
      double elapsed = -1.;
      const int rc = rays_hip_trace_summary(&p, (int)n, r0.data(), n0.data(), o_np.data(), o_sc.data(), o_start.data(),
                                            o_end.data(), o_er.data(), o_mr.data(), &elapsed);
      if (rc) std::fprintf(stderr, "rays_hip_trace_summary(G = %d, n = %zu): rc %d: %s\n", G, n, rc, last_error().c_str());
      CHECK(rc == 0 && elapsed >= 0.);
      CHECK(std::memcmp(o_np.data(), np.data(), sizeof(int32_t) * n) == 0 && o_np[n] == -7);
      CHECK(std::memcmp(o_sc.data(), sc.data(), sizeof(int32_t) * n) == 0 && o_sc[n] == -7);
      CHECK(std::memcmp(o_start.data(), start.data(), sizeof(double) * nv * n) == 0 && o_start[nv * n] == -7.);
      CHECK(std::memcmp(o_end.data(), end.data(), sizeof(double) * nv * n) == 0 && o_end[nv * n] == -7.);
      CHECK(std::memcmp(o_er.data(), eres.data(), sizeof(double) * n) == 0 && o_er[n] == -7.);
      CHECK(std::memcmp(o_mr.data(), mres.data(), sizeof(double) * n) == 0 && o_mr[n] == -7.);
      // start_ray_vec is optional
      std::vector<int32_t> q_np(n + 1, -7);
      CHECK(rays_hip_trace_summary(&p, (int)n, r0.data(), n0.data(), q_np.data(), o_sc.data(), nullptr, o_end.data(),
                                   o_er.data(), o_mr.data(), nullptr) == 0);
      CHECK(std::memcmp(q_np.data(), np.data(), sizeof(int32_t) * n) == 0);
      calls += 2;
    }
  }
  long long summary_launches = 0, wrong = 0, live = -1;
  rays_emul_runtime_stats(&summary_launches, &wrong, &live);

  // rays_hip_trace on the same device lists and on one that repeats a device (three blocks, three slots, one device):
  // without the kept result, and with it switched on for the call and off again (the blocks' slabs stay on the devices
  // and go back to the slots' caches)
  const int trace_lists[][4] = {{0}, {2, 1}, {0, 1, 3}, {0, 1, 2, 3}, {0, 0, 0}};
  const int trace_G[] = {1, 2, 3, 4, 3};
  int trace_calls = 0;
  for (int l = 0; l < 5; l++) {
    const int G = trace_G[l];
    CHECK(rays_hip_init_devices(G, trace_lists[l]) >= 0);
    const size_t counts[] = {nray, (size_t)G + 1, 1, 0};
    for (size_t n : counts) {
      if (n > nray) continue;
      for (int keep = 0; keep < 2; keep++) {
        // poisoned outputs, one element longer than asked for; slots past npoints are not the entry's to write either
        std::vector<double> o_rv(c.npt * nv * n + 1, kPoison), o_res(c.npt * n + 1, kPoison);
        std::vector<int32_t> o_np(n + 1, -7), o_sc(n + 1, -7);
        std::vector<double> o_end(nv * n + 1, kPoison), o_er(n + 1, kPoison), o_mr(n + 1, kPoison);
        double elapsed = -1.;
        if (keep) CHECK(rays_hip_keep_last_result(1) == 0);
        const int rc = rays_hip_trace(&p, (int)n, r0.data(), n0.data(), o_rv.data(), o_res.data(), o_np.data(), o_sc.data(),
                                      o_end.data(), o_er.data(), o_mr.data(), &elapsed);
        if (keep) CHECK(rays_hip_keep_last_result(0) == 1);
        if (rc) std::fprintf(stderr, "rays_hip_trace(list %d, n = %zu, keep %d): rc %d: %s\n", l, n, keep, rc, last_error().c_str());
        CHECK(rc == 0 && elapsed >= 0.);
        CHECK(same_trajectories(c, n, o_rv.data(), o_res.data(), kPoison));
        CHECK(o_rv[c.npt * nv * n] == kPoison && o_res[c.npt * n] == kPoison);
        CHECK(same_summaries(c, n, o_np.data(), o_sc.data(), o_end.data(), o_er.data(), o_mr.data()));
        CHECK(o_np[n] == -7 && o_sc[n] == -7 && o_end[nv * n] == kPoison && o_er[n] == kPoison && o_mr[n] == kPoison);
        trace_calls++;
      }
    }
  }
  // rays_hip_trace_gather on one device (no RCCL) and rays_hip_result_to_host: the same trajectories, zeros past npoints
  const int one[] = {0};
  CHECK(rays_hip_init_devices(1, one) >= 0);
  const size_t gather_counts[] = {nray, 2, 1, 0};
  for (size_t n : gather_counts) {
    if (n > nray) continue;
    rays_device_result_t res;
    const int rc = rays_hip_trace_gather(&p, (int)n, r0.data(), n0.data(), &res);
    if (rc) std::fprintf(stderr, "rays_hip_trace_gather(n = %zu): rc %d: %s\n", n, rc, last_error().c_str());
    CHECK(rc == 0 && res.nray == (int)n && res.device == 0);
    std::vector<double> o_rv(c.npt * nv * n + 1, kPoison), o_res(c.npt * n + 1, kPoison);
    std::vector<int32_t> o_np(n + 1, -7), o_sc(n + 1, -7);
    std::vector<double> o_end(nv * n + 1, kPoison), o_er(n + 1, kPoison), o_mr(n + 1, kPoison);
    CHECK(rays_hip_result_to_host(&p, &res, o_rv.data(), o_res.data(), o_np.data(), o_sc.data(), o_end.data(), o_er.data(),
                                  o_mr.data()) == 0);
    CHECK(same_trajectories(c, n, o_rv.data(), o_res.data(), 0.));
    CHECK(o_rv[c.npt * nv * n] == kPoison && o_res[c.npt * n] == kPoison);
    CHECK(same_summaries(c, n, o_np.data(), o_sc.data(), o_end.data(), o_er.data(), o_mr.data()));
    CHECK(o_np[n] == -7 && o_sc[n] == -7 && o_end[nv * n] == kPoison && o_er[n] == kPoison && o_mr[n] == kPoison);
    trace_calls++;
  }

  // refusals, by name
  std::vector<int32_t> i1(1);
  std::vector<double> d1(nv);
  CHECK(rays_hip_trace_summary(&p, -1, r0.data(), n0.data(), i1.data(), i1.data(), nullptr, d1.data(), d1.data(), d1.data(), nullptr) != 0 &&
        last_error().find("rays_hip_trace_summary: nray < 0") != std::string::npos);
  CHECK(rays_hip_trace_summary(&p, 1, r0.data(), n0.data(), i1.data(), i1.data(), nullptr, nullptr, d1.data(), d1.data(), nullptr) != 0 &&
        last_error().find("rays_hip_trace_summary: null array argument") != std::string::npos);
  CHECK(rays_hip_trace_summary_device(&p, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0 &&
        last_error().find("rays_hip_trace_summary_device: null device pointer") != std::string::npos);
  CHECK(rays_hip_scan_summary_device(&p, 1 << 16, r0.data(), 1 << 16, r0.data(), n0.data(), i1.data(), i1.data(), nullptr, d1.data(),
                                     d1.data(), d1.data(), nullptr) != 0 &&
        last_error().find("n_runs * nray exceeds") != std::string::npos);
  CHECK(std::strstr(rays_hip_summary_kernel_name_for(&p, (int)nray), "rk4_trace_kernel<37, 2, 0, 7>") != nullptr);

  long long launches = 0, pinned = -1, streams = -1, events = -1;
  rays_emul_runtime_stats(&launches, &wrong, &live);
  CHECK(wrong == 0 && live > 0);   // (the entry's cached blocks and the refill counters are still held)
  CHECK(rays_hip_finalize() == 0);
  rays_emul_runtime_stats(&launches, &wrong, &live);
  rays_emul_runtime_live(&pinned, &streams, &events);
  CHECK(live == 0 && pinned == 0 && streams == 0 && events == 0 && wrong == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("summary capi ok: %d calls, %lld launches\n", calls, summary_launches);
  std::printf("trace capi ok: %d calls, %lld launches\n", trace_calls, launches - summary_launches);
  return 0;
}
