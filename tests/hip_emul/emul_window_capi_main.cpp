// TEST INFRASTRUCTURE ONLY: windowed tracing through the product's C ABI (rays_hip_state_init_device,
// rays_hip_trace_window_device, rays_hip_state_summary_device, rays_hip_trace_windowed; rays_amd/csrc/rays_capi.hip) as a
// stand-alone program on the emulated HIP runtime -- for plain and for sanitizer runs (tests/hip_emul/
// Makefile.capi, target window; tests/test_cpu_window_trace.py writes the case file and starts it).
//   emul_window_capi <case file>
// Case file (native endianness): int32 nray, nv, sizeof(rays_params_t); the parameter block; rvec0[nray][3],
// rindex_vec0[nray][3]; then the oracle's summaries of these rays: npoints[nray], stop_code[nray] (int32),
// end_ray_vec[nray][nv], end_residuals[nray], max_residuals[nray]; then the oracle's trajectories of the same trace,
// packed to npoints points per ray: ray_vec[sum npoints][nv], residual[sum npoints].
// The host form must reproduce the oracle's bytes for several window lengths into poisoned outputs of which nothing
// past npoints may be touched, and the device bytes in use during the call never exceed the state, two window slabs,
// the inputs and the summaries; the device entries do the same with recording and summary windows mixed; every
// refusal is checked by its message; after rays_hip_finalize the emulated driver holds nothing.
#define RAYS_EMUL_RUNTIME 1
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "emul_capi_check.hpp"

extern "C" void rays_emul_runtime_stats(long long* launches, long long* wrong_device, long long* live_allocations);
extern "C" void rays_emul_runtime_live(long long* pinned, long long* streams, long long* events);

static const double kPoison = -7.;
// device bytes the emulated driver has handed out and not got back
static long long live_device_bytes() {
  hip_emul::State& s = hip_emul::state();
  std::lock_guard<std::mutex> lk(s.mu);
  long long b = 0;
  for (const auto& kv : s.allocs) b += (long long)kv.second.bytes;
  return b;
}
template <class T>
static T* dev_alloc(size_t n) {
  T* p = nullptr;
  if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); std::exit(2); }
  return p;
}

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
  std::vector<double> r0, n0;
  Case c;
  bool ok = std::fread(&p, sizeof p, 1, f) == 1 && read_n(f, r0, 3 * nray) && read_n(f, n0, 3 * nray) &&
            read_n(f, c.np, nray) && read_n(f, c.sc, nray) && read_n(f, c.end, nv * nray) && read_n(f, c.eres, nray) &&
            read_n(f, c.mres, nray);
  c.nv = nv;
  c.npt = (size_t)p.nstep_max + 1;
  c.offs.assign(nray + 1, 0);
  for (size_t i = 0; ok && i < nray; i++) {
    ok = c.np[i] >= 1 && (size_t)c.np[i] <= c.npt;
    c.offs[i + 1] = c.offs[i] + (size_t)c.np[i];
  }
  ok = ok && read_n(f, c.pv, nv * c.offs[nray]) && read_n(f, c.pr, c.offs[nray]);
  std::fclose(f);
  if (!ok || (int)nv != p.nv) { std::fprintf(stderr, "short or inconsistent case file\n"); return 2; }
  if (rays_hip_device_count() < 3) { std::fprintf(stderr, "needs 3 emulated devices\n"); return 2; }

  // ---- the host form: the first device of the list, several window lengths, all rays and a few ----
  const int lists[][2] = {{0, 1}, {2, 1}};
  int calls = 0;
  for (int l = 0; l < 2; l++) {
    CHECK(rays_hip_init_devices(2, lists[l]) >= 0);
    const int lens[] = {1, 7, 50, p.nstep_max + 5};
    for (int W : lens) {
      const size_t counts[] = {nray, 3, 1, 0};
      for (size_t n : counts) {
        if (n > nray || (W == 1 && n == nray && l == 1)) continue;
        std::vector<double> o_rv(c.npt * nv * n + 1, kPoison), o_res(c.npt * n + 1, kPoison);
        std::vector<int32_t> o_np(n + 1, -7), o_sc(n + 1, -7);
        std::vector<double> o_end(nv * n + 1, kPoison), o_er(n + 1, kPoison), o_mr(n + 1, kPoison);
        double elapsed = -1.;
        const long long before = live_device_bytes();
        // the device bytes in use while the call runs: sampled from a second thread (every block of the call is
        // allocated before its first launch and held to its end, so any sample taken during the launches sees them all)
        std::atomic<bool> stop{false};
        long long peak = before;
        std::thread sampler([&] {
          while (!stop.load()) {
            const long long b = live_device_bytes();
            if (b > peak) peak = b;
            std::this_thread::sleep_for(std::chrono::microseconds(200));
          }
        });
        const int rc = rays_hip_trace_windowed(&p, (int)n, r0.data(), n0.data(), W, o_rv.data(), o_res.data(), o_np.data(),
                                               o_sc.data(), o_end.data(), o_er.data(), o_mr.data(), &elapsed);
        stop = true;
        sampler.join();
        if (rc) std::fprintf(stderr, "rays_hip_trace_windowed(list %d, W = %d, n = %zu): rc %d: %s\n", l, W, n, rc, last_error().c_str());
        CHECK(rc == 0 && elapsed >= 0.);
        CHECK(same_trajectories(c, n, o_rv.data(), o_res.data(), kPoison));
        CHECK(o_rv[c.npt * nv * n] == kPoison && o_res[c.npt * n] == kPoison);
        CHECK(same_summaries(c, n, o_np.data(), o_sc.data(), o_end.data(), o_er.data(), o_mr.data()));
        CHECK(o_np[n] == -7 && o_sc[n] == -7 && o_end[nv * n] == kPoison && o_er[n] == kPoison && o_mr[n] == kPoison);
        // state: v, s, resid[3], sg_err[2] doubles + nstep, stop_code, flags; two slabs of W points with npoints_win;
        // the inputs; point 1 and the five summaries; + the library's fixed blocks (refill counters, ray order
        // workspace: 64 KB is generous for them) and what earlier calls left in the slot's cache (`before`)
        const long long N = (long long)n, NV = (long long)nv;
        const long long bound = before + N * (8 * (NV + 1 + 3 + 2) + 3 * 4) + 2 * N * ((long long)W * 8 * (NV + 1) + 4) + N * 6 * 8 +
                                N * (8 * (2 * NV + 2) + 2 * 4) + 65536;
        if (peak > bound) std::fprintf(stderr, "W = %d, n = %zu: %lld device bytes in use, bound %lld\n", W, n, peak, bound);
        CHECK(peak <= bound);
        calls++;
      }
    }
  }

  // ---- the device entries: recording and summary windows mixed, the state's summaries, idempotence ----
  const int one[] = {0};
  CHECK(rays_hip_init_devices(1, one) >= 0);
  CHECK(hipSetDevice(0) == hipSuccess);
  {
    const size_t n = nray;
    const int W = 16;
    double *d_r0 = dev_alloc<double>(3 * n), *d_n0 = dev_alloc<double>(3 * n);
    CHECK(hipMemcpy(d_r0, r0.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(d_n0, n0.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice) == hipSuccess);
    rays_ray_state_t S;
    S.v = dev_alloc<double>(nv * n); S.s = dev_alloc<double>(n); S.nstep = dev_alloc<int32_t>(n);
    S.stop_code = dev_alloc<int32_t>(n); S.resid = dev_alloc<double>(3 * n); S.sg_err = nullptr;  // RK4: may be null
    S.flags = dev_alloc<int32_t>(n);
    double *d_start = dev_alloc<double>(nv * n), *d_rv = dev_alloc<double>(n * W * nv), *d_res = dev_alloc<double>(n * W);
    int32_t* d_npw = dev_alloc<int32_t>(n);
    CHECK(rays_hip_state_init_device(&p, (int)n, d_r0, d_n0, &S, d_start, nullptr) == 0);
    std::vector<double> o_rv(c.npt * nv * n, kPoison), o_res(c.npt * n, kPoison), w_rv(n * W * nv), w_res(n * W);
    std::vector<int32_t> npw(n), have(n, 1), sc(n);
    for (size_t i = 0; i < n; i++) {
      CHECK(hipMemcpy(&o_rv[c.npt * nv * i], d_start + nv * i, sizeof(double) * nv, hipMemcpyDeviceToHost) == hipSuccess);
      o_res[c.npt * i] = 0.;
    }
    std::vector<char> covered(c.npt * n, 0);
    for (size_t i = 0; i < n; i++) covered[c.npt * i] = 1;
    int windows = 0;
    for (;; windows++) {
      const bool rec = windows % 3 != 1;  // every third window is a summary window
      const int rc = rays_hip_trace_window_device(&p, (int)n, &S, W, rec ? d_rv : nullptr, rec ? d_res : nullptr, d_npw, nullptr);
      if (rc) std::fprintf(stderr, "rays_hip_trace_window_device: rc %d: %s\n", rc, last_error().c_str());
      CHECK(rc == 0);
      if (rc) break;
      CHECK(hipMemcpy(npw.data(), d_npw, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess);
      if (rec) {
        CHECK(hipMemcpy(w_rv.data(), d_rv, sizeof(double) * n * W * nv, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(hipMemcpy(w_res.data(), d_res, sizeof(double) * n * W, hipMemcpyDeviceToHost) == hipSuccess);
      }
      bool any = false;
      for (size_t i = 0; i < n; i++) {
        const size_t m = (size_t)npw[i], at = (size_t)have[i];
        CHECK(npw[i] >= 0 && npw[i] <= W && at + m <= c.npt);
        if (rec && m) {
          std::memcpy(&o_rv[(c.npt * i + at) * nv], &w_rv[i * W * nv], sizeof(double) * nv * m);
          std::memcpy(&o_res[c.npt * i + at], &w_res[i * W], sizeof(double) * m);
          for (size_t j = 0; j < m; j++) covered[c.npt * i + at + j] = 1;
        }
        have[i] += npw[i];
        any = any || npw[i] == W;
      }
      if (!any) break;
    }
    CHECK(windows >= 3);
    // the recorded windows equal the matching slices of the one-shot trace; nothing else was written
    bool slices = true;
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j < c.npt; j++) {
        const bool in = j < (size_t)c.np[i] && covered[c.npt * i + j];
        const double* ref_v = in ? &c.pv[(c.offs[i] + j) * nv] : nullptr;
        for (size_t k = 0; k < nv; k++) {
          const double want = in ? ref_v[k] : kPoison;
          slices = slices && std::memcmp(&o_rv[(c.npt * i + j) * nv + k], &want, sizeof want) == 0;
        }
        const double want = in ? c.pr[c.offs[i] + j] : kPoison;
        slices = slices && std::memcmp(&o_res[c.npt * i + j], &want, sizeof want) == 0;
      }
    CHECK(slices);
    // the state's summaries, and one more window: no byte of the state changes, npoints_win = 0
    int32_t *d_np = dev_alloc<int32_t>(n), *d_sc = dev_alloc<int32_t>(n);
    double *d_end = dev_alloc<double>(nv * n), *d_er = dev_alloc<double>(n), *d_mr = dev_alloc<double>(n);
    CHECK(rays_hip_state_summary_device(&p, (int)n, &S, d_np, d_sc, d_end, d_er, d_mr, nullptr) == 0);
    std::vector<int32_t> o_np(n), o_sc(n);
    std::vector<double> o_end(nv * n), o_er(n), o_mr(n);
    CHECK(hipMemcpy(o_np.data(), d_np, 4 * n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(o_sc.data(), d_sc, 4 * n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(o_end.data(), d_end, 8 * nv * n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(o_er.data(), d_er, 8 * n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(o_mr.data(), d_mr, 8 * n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(same_summaries(c, n, o_np.data(), o_sc.data(), o_end.data(), o_er.data(), o_mr.data()));
    const auto snapshot = [&] {
      std::vector<char> b;
      const auto add = [&](const void* d, size_t bytes) {
        const size_t at = b.size();
        b.resize(at + bytes);
        CHECK(hipMemcpy(b.data() + at, d, bytes, hipMemcpyDeviceToHost) == hipSuccess);
      };
      add(S.v, 8 * nv * n); add(S.s, 8 * n); add(S.nstep, 4 * n); add(S.stop_code, 4 * n); add(S.resid, 24 * n); add(S.flags, 4 * n);
      return b;
    };
    const std::vector<char> s0 = snapshot();
    CHECK(rays_hip_trace_window_device(&p, (int)n, &S, 5, d_rv, d_res, d_npw, nullptr) == 0);
    CHECK(hipMemcpy(npw.data(), d_npw, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess);
    bool zero = true;
    for (size_t i = 0; i < n; i++) zero = zero && npw[i] == 0;
    CHECK(zero && snapshot() == s0);
    calls += windows + 2;

    // ---- refusals, by name, before anything is launched ----
    long long launches0 = 0, wrong = 0, live = 0, launches1 = 0;
    rays_emul_runtime_stats(&launches0, &wrong, &live);
    const char* who = "rays_hip_trace_window_device";
    CHECK(refused(rays_hip_trace_window_device(&p, (int)n, &S, 0, d_rv, d_res, d_npw, nullptr), "rays_hip_trace_window_device: n_steps < 1"));
    CHECK(refused(rays_hip_trace_window_device(&p, -1, &S, 4, d_rv, d_res, d_npw, nullptr), "rays_hip_trace_window_device: nray < 0"));
    CHECK(refused(rays_hip_trace_window_device(&p, (int)n, &S, 4, d_rv, nullptr, d_npw, nullptr), "given together or not at all"));
    CHECK(refused(rays_hip_trace_window_device(&p, (int)n, &S, 4, nullptr, d_res, d_npw, nullptr), "given together or not at all"));
    CHECK(refused(rays_hip_trace_window_device(&p, (int)n, &S, 4, d_rv, d_res, nullptr, nullptr), "rays_hip_trace_window_device: null device pointer"));
    CHECK(refused(rays_hip_trace_window_device(&p, (int)n, nullptr, 4, d_rv, d_res, d_npw, nullptr), "null pointer in the ray state"));
    {
      rays_ray_state_t T = S;
      T.resid = nullptr;
      CHECK(refused(rays_hip_trace_window_device(&p, (int)n, &T, 4, d_rv, d_res, d_npw, nullptr), "rays_hip_trace_window_device: null pointer in the ray state"));
      CHECK(refused(rays_hip_state_init_device(&p, (int)n, d_r0, d_n0, &T, nullptr, nullptr), "rays_hip_state_init_device: null pointer in the ray state"));
      CHECK(refused(rays_hip_state_summary_device(&p, (int)n, &T, d_np, d_sc, d_end, d_er, d_mr, nullptr), "rays_hip_state_summary_device: null pointer in the ray state"));
      rays_params_t q = p;
      q.ode_solver = RAYS_ODE_SG;  // S.sg_err is null
      if (rays_hip_check_params(&q) == 0) {
        CHECK(refused(rays_hip_trace_window_device(&q, (int)n, &S, 4, d_rv, d_res, d_npw, nullptr), "SG_ODE needs the ray state's sg_err"));
        CHECK(refused(rays_hip_state_init_device(&q, (int)n, d_r0, d_n0, &S, nullptr, nullptr), "SG_ODE needs the ray state's sg_err"));
      } else {
        std::fprintf(stderr, "the SG twin of the case is refused: %s\n", last_error().c_str());
        failures++;
      }
      // a shape that is not built: refused with the message of rays_hip_check_params
      rays_params_t u = p;
      u.nv = 12;
      const int rcu = rays_hip_check_params(&u);
      const std::string msg = last_error();
      CHECK(rcu != 0 && refused(rays_hip_trace_window_device(&u, (int)n, &S, 4, d_rv, d_res, d_npw, nullptr), msg.c_str()));
      CHECK(std::strcmp(rays_hip_window_kernel_name_for(&u, (int)n, 1), "") == 0);
    }
    CHECK(refused(rays_hip_state_init_device(&p, (int)n, nullptr, d_n0, &S, nullptr, nullptr), "rays_hip_state_init_device: null device pointer"));
    CHECK(refused(rays_hip_state_summary_device(&p, (int)n, &S, d_np, nullptr, d_end, d_er, d_mr, nullptr), "rays_hip_state_summary_device: null device pointer"));
    std::vector<double> h1(c.npt * nv);
    std::vector<int32_t> i1(1);
    CHECK(refused(rays_hip_trace_windowed(&p, 1, r0.data(), n0.data(), 0, h1.data(), h1.data(), i1.data(), i1.data(), nullptr, nullptr, nullptr, nullptr),
                  "rays_hip_trace_windowed: n_steps < 1"));
    CHECK(refused(rays_hip_trace_windowed(&p, -1, r0.data(), n0.data(), 4, h1.data(), h1.data(), i1.data(), i1.data(), nullptr, nullptr, nullptr, nullptr),
                  "rays_hip_trace_windowed: nray < 0"));
    CHECK(refused(rays_hip_trace_windowed(&p, 1, r0.data(), n0.data(), 4, nullptr, h1.data(), i1.data(), i1.data(), nullptr, nullptr, nullptr, nullptr),
                  "rays_hip_trace_windowed: null array argument"));
    (void)who;
    rays_emul_runtime_stats(&launches1, &wrong, &live);
    CHECK(launches1 == launches0);  // nothing was launched by a refused call
    // the kernels' names: the recording kernel's with the continuation bit (and the summary-only bit)
    CHECK(std::strcmp(rays_hip_window_kernel_name_for(&p, (int)n, 1), "rk4_trace_kernel<133, 2, 0, 7>") == 0);
    CHECK(std::strcmp(rays_hip_window_kernel_name_for(&p, 1 << 20, 1), "rk4_trace_kernel<133, 2, 0, 7>") == 0);
    CHECK(std::strcmp(rays_hip_window_kernel_name_for(&p, (int)n, 0), "rk4_trace_kernel<165, 2, 0, 7>") == 0);
    void* mine[] = {d_r0, d_n0, S.v, S.s, S.nstep, S.stop_code, S.resid, S.flags, d_start, d_rv, d_res, d_npw, d_np, d_sc, d_end, d_er, d_mr};
    for (void* q : mine) CHECK(hipFree(q) == hipSuccess);
  }

  long long launches = 0, wrong = 0, live = -1, pinned = -1, streams = -1, events = -1;
  CHECK(rays_hip_finalize() == 0);
  rays_emul_runtime_stats(&launches, &wrong, &live);
  rays_emul_runtime_live(&pinned, &streams, &events);
  CHECK(live == 0 && pinned == 0 && streams == 0 && events == 0 && wrong == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("window capi ok: %d calls, %lld launches\n", calls, launches);
  return 0;
}
