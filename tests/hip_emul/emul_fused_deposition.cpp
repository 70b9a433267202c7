// TEST INFRASTRUCTURE ONLY: the FUSED DEPOSITION variant of the product trace kernels (EQ | kEqNoTraj | kEqDeposit: no
// trajectory point is recorded, every accepted point is binned into the ray's row of work;
// rays_amd/csrc/rays_deposition.hpp: DepTraceArgs) on the host emulation, for tests/test_cpu_fused_deposition.py.
// TraceArgs::residual is NULL and TraceArgs::ray_vec carries the DepTraceArgs block, as in the product's launches, so a
// trajectory store the variant should not have is a crash of this process and nothing worse.
//   (no switch)                  one emulated lane (emul_trace.cpp's run<> / run_ms<> with the two flags in EQ)
//   -DRAYS_EMUL_DEPOSIT_WAVE     whole emulated waves (emul_group.cpp's runners): RK4 with refills, SG
// Built with -DRAYS_RK4_NO_HANDOVER like the summary-only emulation: these are exact kernels.
#ifndef RAYS_RK4_NO_HANDOVER
#error "compile with -DRAYS_RK4_NO_HANDOVER: the fused deposition kernels are exact kernels"
#endif
#ifdef RAYS_EMUL_DEPOSIT_WAVE
#include "emul_group.cpp"
#else
#include "emul_trace.cpp"
#endif

namespace {
constexpr int FD = rays::kEqNoTraj | rays::kEqDeposit;

// the shapes with a fused build.  One lane: two species with damping (nv = 8 | 13) in the slab and axisym_toroid, and
// the slab's multi_spec_damping kernel; whole waves: the unit-exponent kernels with nv = 8
struct FusedShapes {
  template <int EQ, int DERIV, int NS, int NV>
  static constexpr bool lane = (EQ & rays::kEqMultiSpec) ? (EQ & 7) == 4 : (EQ & 1) == 0 && NS == 2 && (NV == 8 || NV == 13);
  template <class S> static constexpr bool wave = (S::EQ & 4) != 0 && S::NV == 8;
};

// the launch's argument blocks as rays_capi.hip: trace_deposition_launch fills them; work[n_bins][nray] zeroed here
rays::DepTraceArgs fused_block(const rays_params_t* p, int nray, int which, int n_bins, const double* power,
                               const double* rho_grid, const double* rho_fspl, int n_rho, double* work) {
  rays::DepTraceArgs T;
  T.which = which; T.n_bins = n_bins;
  T.grid_min = 0.; T.grid_max = 1.;
  if (which == RAYS_DEP_PTOTAL_X) { T.grid_min = p->slab.xmin; T.grid_max = p->slab.xmax; }
  T.power = power; T.work = work; T.rho_grid = rho_grid; T.rho_fspl = rho_fspl; T.n_rho = n_rho; T.pad_ = 0;
  for (size_t i = 0; i < (size_t)n_bins * (size_t)nray; i++) work[i] = 0.;
  return T;
}
rays::TraceArgs fused_args(int nray, const double* rvec0, const double* rindex_vec0, int32_t* npoints, int32_t* stop_code,
                           double* start_ray_vec, double* end_ray_vec, double* end_residuals, double* max_residuals,
                           unsigned* counter, const rays::DepTraceArgs* T) {
  rays::TraceArgs A = emul_trace_args(nray, rvec0, rindex_vec0,   // residual = nullptr, ray_vec: the block
                                      EmulOut{nullptr, nullptr, npoints, stop_code, start_ray_vec, end_ray_vec,
                                              end_residuals, max_residuals}, counter);
  A.set_dep(T);
  return A;
}
// profile(b) = carry(b) + work(b, 1) + work(b, 2) + ... in ray order (rays_deposition.hip: profile_sum_kernel)
void fused_profile(int n_bins, int nray, const double* work, const double* carry, double* profile) {
  for (int b = 0; b < n_bins; b++) {
    double s = carry ? carry[b] : 0.;
    for (int r = 0; r < nray; r++) s = s + work[(size_t)b * nray + r];
    profile[b] = s;
  }
}
bool fused_refused(const rays_params_t* p, int which, int n_bins) {
  if (p->nv < 8 || !p->damping_model || n_bins < 1 || n_bins > RAYS_DEP_MAX_BINS) return true;
  if (p->equilib_model == RAYS_EQ_SLAB) return which != RAYS_DEP_PTOTAL_X;
  if (p->equilib_model != RAYS_EQ_AXISYM) return true;
  return which != RAYS_DEP_PTOTAL_PSI && which != RAYS_DEP_PTOTAL_RHO;
}
}  // namespace

#ifndef RAYS_EMUL_DEPOSIT_WAVE
// One emulated lane: the launch of rays_hip_trace_deposition_device.  work[n_bins][nray] bin-major, as on the device.
extern "C" int rays_emul_fused_deposition(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                                          const double* power, int which, int n_bins, const double* rho_grid,
                                          const double* rho_fspl, int n_rho, int32_t* npoints, int32_t* stop_code,
                                          double* start_ray_vec, double* end_ray_vec, double* end_residuals,
                                          double* max_residuals, double* work, const double* profile_in, double* profile) {
  if (fused_refused(p, which, n_bins)) return 5;
  unsigned counter = 0;
  const rays::DepTraceArgs T = fused_block(p, nray, which, n_bins, power, rho_grid, rho_fspl, n_rho, work);
  rays::TraceArgs A = fused_args(nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                 max_residuals, &counter, &T);
  std::vector<double> sg_far;
  emul_one_lane_far(A, sg_far);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  const int rc = emul_lane_dispatch<FusedShapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return run1<S::EQ | FD, S::DERIV, S::NS, S::NV>(p->ode_solver, D, A);
  });
  if (rc) return rc;
  fused_profile(n_bins, nray, work, profile_in, profile);
  return 0;
}
#else
// Whole emulated waves.  kind 0: rk4_trace_kernel (stride: the "long rays first" neighbourhood size, 0 | 1: index
// order), 2: sg_trace_kernel; `blocks` waves of 64 lanes each.  Cold derivatives, two species, nv = 8.
extern "C" int rays_emul_fused_deposition_waves(const rays_params_t* p, int kind, int blocks, int stride, int nray,
                                                const double* rvec0, const double* rindex_vec0, const double* power,
                                                int which, int n_bins, const double* rho_grid, const double* rho_fspl,
                                                int n_rho, int32_t* npoints, int32_t* stop_code, double* start_ray_vec,
                                                double* end_ray_vec, double* end_residuals, double* max_residuals,
                                                double* work, const double* profile_in, double* profile) {
  if ((kind != 0 && kind != 2) || blocks < 1 || p->multi_spec_damping || fused_refused(p, which, n_bins)) return 1;
  if (p->ode_solver != (kind == 0 ? RAYS_ODE_RK4 : RAYS_ODE_SG) || p->ray_deriv != RAYS_DERIV_COLD) return 1;
  unsigned counter = 0;
  const rays::DepTraceArgs T = fused_block(p, nray, which, n_bins, power, rho_grid, rho_fspl, n_rho, work);
  rays::TraceArgs A = fused_args(nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                 max_residuals, &counter, &T);
  std::vector<unsigned> sched;
  if (kind == 0) emul_sched(A, sched, stride);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  g_rk4_w2_body = 0;
  const int rc = kind == 0 ? emul_wave_dispatch<FusedShapes>(Rk4WaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_rk4_waves<S::EQ | FD, S::NS, S::NV>(D, A, blocks);
  }) : emul_wave_dispatch<FusedShapes>(SgWaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_sg_waves<S::EQ | FD, S::NS, S::NV>(D, A, blocks);
  });
  if (rc) return rc;
  fused_profile(n_bins, nray, work, profile_in, profile);
  return 0;
}
#endif
