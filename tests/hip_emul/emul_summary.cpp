// TEST INFRASTRUCTURE ONLY: the SUMMARY-ONLY variant of the product trace kernels (EQ | kEqNoTraj: no trajectory point
// is recorded; rays_amd/csrc/rays_trace.hpp: TraceArgs::start_ray_vec) on the host emulation, for
// tests/test_cpu_summary_trace.py.  TraceArgs::ray_vec and ::residual are NULL here, as they are in the product's
// launches, so a store the variant should not have is a crash of this process and nothing worse.
//   (no switch)               one emulated lane (emul_trace.cpp's run<> / run_ms<> with the flag in EQ)
//   -DRAYS_EMUL_SUMMARY_WAVE  whole emulated waves (emul_group.cpp's runners): RK4 with refills, SG, the lane-group SG
// Built with -DRAYS_RK4_NO_HANDOVER: emul_trace.cpp switches the tolerance kernels' hand-over on for the emulation, and
// the summary-only kernels exist in the exact arithmetic only (the hand-over reads residual(:)).
#ifndef RAYS_RK4_NO_HANDOVER
#error "compile with -DRAYS_RK4_NO_HANDOVER: the summary-only kernels are exact kernels"
#endif
#ifdef RAYS_EMUL_SUMMARY_WAVE
#include "emul_group.cpp"
#else
#include "emul_trace.cpp"
#endif

namespace {
constexpr int NT = rays::kEqNoTraj;
// ray_vec = residual = nullptr
rays::TraceArgs summary_args(int nray, const double* rvec0, const double* rindex_vec0, int32_t* npoints, int32_t* stop_code,
                             double* start_ray_vec, double* end_ray_vec, double* end_residuals, double* max_residuals,
                             unsigned* counter) {
  return emul_trace_args(nray, rvec0, rindex_vec0,
                         EmulOut{nullptr, nullptr, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                 max_residuals}, counter);
}
// the lane-group kernels with a summary-only build
struct SummaryGroups {
  template <class S> static constexpr bool wave = (S::EQ == 4 && S::NS == 3) || (S::EQ == 5 && S::NS == 2);
};
}  // namespace

#ifndef RAYS_EMUL_SUMMARY_WAVE
// One emulated lane: the launch of rays_hip_trace_summary_device, or with ds_run / rays_per_run of
// rays_hip_scan_summary_device.  The same kernel selection as rays_emul_trace_ex, with kEqNoTraj in EQ.
extern "C" int rays_emul_summary_trace(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                                       int32_t* npoints, int32_t* stop_code, double* start_ray_vec, double* end_ray_vec,
                                       double* end_residuals, double* max_residuals, const double* ds_run,
                                       int rays_per_run) {
  unsigned counter = 0;
  rays::TraceArgs A = summary_args(nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                   max_residuals, &counter);
  A.ds_run = ds_run; A.rays_per_run = rays_per_run;
  std::vector<double> sg_far;
  emul_one_lane_far(A, sg_far);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  return emul_lane_dispatch<AllShapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return run1<S::EQ | NT, S::DERIV, S::NS, S::NV>(p->ode_solver, D, A);
  });
}
#else
// Whole emulated waves.  kind 0: rk4_trace_kernel, 1: rk4_trace_kernel_w2's body, 2: sg_trace_kernel (`blocks` waves of
// 64 lanes each); 3: sg_group_kernel with G = `stride_or_G` lanes per ray (`blocks` resident blocks of 256 lanes).
// stride_or_G, kinds 0: the "long rays first" neighbourhood size (0 | 1: index order).
extern "C" int rays_emul_summary_waves(const rays_params_t* p, int kind, int blocks, int stride_or_G, int nray,
                                       const double* rvec0, const double* rindex_vec0, int32_t* npoints,
                                       int32_t* stop_code, double* start_ray_vec, double* end_ray_vec,
                                       double* end_residuals, double* max_residuals) {
  if (kind < 0 || kind > 3 || blocks < 1 || p->multi_spec_damping) return 1;
  if (p->ode_solver != (kind <= 1 ? RAYS_ODE_RK4 : RAYS_ODE_SG)) return 1;
  if (p->ray_deriv != (kind == 3 ? RAYS_DERIV_NUM : RAYS_DERIV_COLD)) return 1;
  unsigned counter = 0;
  rays::TraceArgs A = summary_args(nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                   max_residuals, &counter);
  std::vector<unsigned> sched;
  if (kind == 0) emul_sched(A, sched, stride_or_G);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  if (kind <= 1) {
    g_rk4_w2_body = kind;
    return emul_wave_dispatch<UnitExpWaves>(Rk4WaveShapes{}, p, [&](auto sh) {
      typedef decltype(sh) S;
      return run_rk4_waves<S::EQ | NT, S::NS, S::NV>(D, A, blocks);
    });
  }
  if (kind == 2)
    return emul_wave_dispatch<UnitExpWaves>(SgWaveShapes{}, p, [&](auto sh) {
      typedef decltype(sh) S;
      return run_sg_waves<S::EQ | NT, S::NS, S::NV>(D, A, blocks);
    });
  return emul_wave_dispatch<SummaryGroups>(GroupShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_group_g<S::EQ | NT, S::NS>(stride_or_G, D, A, blocks);
  });
}
#endif
