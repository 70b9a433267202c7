// TEST INFRASTRUCTURE ONLY: the TWO-PROFILE variant of the fused deposition kernels (EQ | kEqNoTraj | kEqDeposit |
// kEqDeposit2: every accepted point is binned into two rows from one grid evaluation; rays_amd/csrc/rays_deposition.hpp:
// Dep2TraceArgs) on the host emulation, for tests/test_cpu_fused_profiles.py.  Built like emul_fused_deposition.cpp, whose
// single-profile entries this library holds too (the comparisons take both from one library, one set of tables):
//   (no switch)                  one emulated lane
//   -DRAYS_EMUL_DEPOSIT_WAVE     whole emulated waves: RK4 with refills, SG
#include "emul_fused_deposition.cpp"

namespace {
constexpr int FD2 = FD | rays::kEqDeposit2;

// the shapes with a two-profile build: the axisym_toroid ones of the fused build
struct Fused2Shapes {
  template <int EQ, int DERIV, int NS, int NV>
  static constexpr bool lane = (EQ & 3) == 2 && FusedShapes::lane<EQ, DERIV, NS, NV>;
  template <class S> static constexpr bool wave = (S::EQ & 3) == 2 && FusedShapes::wave<S>;
};

// the launch's argument block as rays_capi.hip: trace_profiles_launch fills it; both work arrays zeroed here
rays::Dep2TraceArgs fused2_block(int nray, const int* which, const int* n_bins, const double* power, const double* rho_grid,
                                 const double* rho_fspl, int n_rho, double* const* work) {
  rays::Dep2TraceArgs T;
  for (int i = 0; i < 2; i++) {
    T.prof[i].which = which[i]; T.prof[i].n_bins = n_bins[i];
    T.prof[i].grid_min = 0.; T.prof[i].grid_max = 1.;
    T.prof[i].work = work[i];
    for (size_t k = 0; k < (size_t)n_bins[i] * (size_t)nray; k++) work[i][k] = 0.;
  }
  T.power = power; T.rho_grid = rho_grid; T.rho_fspl = rho_fspl; T.n_rho = n_rho; T.pad_ = 0;
  return T;
}
bool fused2_refused(const rays_params_t* p, const int* which, const int* n_bins) {
  if (p->equilib_model != RAYS_EQ_AXISYM || which[0] == which[1]) return true;
  return fused_refused(p, which[0], n_bins[0]) || fused_refused(p, which[1], n_bins[1]);
}
}  // namespace

#ifndef RAYS_EMUL_DEPOSIT_WAVE
// One emulated lane: the launch of rays_hip_trace_profiles_device with two records.  which[2], n_bins[2]; work_a / work_b
// bin-major, as on the device; each profile continued from its own carry.
extern "C" int rays_emul_fused_profiles(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                                        const double* power, const int* which, const int* n_bins, const double* rho_grid,
                                        const double* rho_fspl, int n_rho, int32_t* npoints, int32_t* stop_code,
                                        double* start_ray_vec, double* end_ray_vec, double* end_residuals,
                                        double* max_residuals, double* work_a, double* work_b, const double* profile_in_a,
                                        const double* profile_in_b, double* profile_a, double* profile_b) {
  if (fused2_refused(p, which, n_bins)) return 5;
  unsigned counter = 0;
  double* const work[2] = {work_a, work_b};
  const rays::Dep2TraceArgs T = fused2_block(nray, which, n_bins, power, rho_grid, rho_fspl, n_rho, work);
  rays::TraceArgs A = fused_args(nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                 max_residuals, &counter, nullptr);
  A.set_dep2(&T);
  std::vector<double> sg_far;
  emul_one_lane_far(A, sg_far);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  const int rc = emul_lane_dispatch<Fused2Shapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return run1<S::EQ | FD2, S::DERIV, S::NS, S::NV>(p->ode_solver, D, A);
  });
  if (rc) return rc;
  fused_profile(n_bins[0], nray, work_a, profile_in_a, profile_a);
  fused_profile(n_bins[1], nray, work_b, profile_in_b, profile_b);
  return 0;
}
#else
// Whole emulated waves (kind, blocks, stride: as rays_emul_fused_deposition_waves).
extern "C" int rays_emul_fused_profiles_waves(const rays_params_t* p, int kind, int blocks, int stride, int nray,
                                              const double* rvec0, const double* rindex_vec0, const double* power,
                                              const int* which, const int* n_bins, const double* rho_grid,
                                              const double* rho_fspl, int n_rho, int32_t* npoints, int32_t* stop_code,
                                              double* start_ray_vec, double* end_ray_vec, double* end_residuals,
                                              double* max_residuals, double* work_a, double* work_b,
                                              const double* profile_in_a, const double* profile_in_b, double* profile_a,
                                              double* profile_b) {
  if ((kind != 0 && kind != 2) || blocks < 1 || p->multi_spec_damping || fused2_refused(p, which, n_bins)) return 1;
  if (p->ode_solver != (kind == 0 ? RAYS_ODE_RK4 : RAYS_ODE_SG) || p->ray_deriv != RAYS_DERIV_COLD) return 1;
  unsigned counter = 0;
  double* const work[2] = {work_a, work_b};
  const rays::Dep2TraceArgs T = fused2_block(nray, which, n_bins, power, rho_grid, rho_fspl, n_rho, work);
  rays::TraceArgs A = fused_args(nray, rvec0, rindex_vec0, npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals,
                                 max_residuals, &counter, nullptr);
  A.set_dep2(&T);
  std::vector<unsigned> sched;
  if (kind == 0) emul_sched(A, sched, stride);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  g_rk4_w2_body = 0;
  const int rc = kind == 0 ? emul_wave_dispatch<Fused2Shapes>(Rk4WaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_rk4_waves<S::EQ | FD2, S::NS, S::NV>(D, A, blocks);
  }) : emul_wave_dispatch<Fused2Shapes>(SgWaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_sg_waves<S::EQ | FD2, S::NS, S::NV>(D, A, blocks);
  });
  if (rc) return rc;
  fused_profile(n_bins[0], nray, work_a, profile_in_a, profile_a);
  fused_profile(n_bins[1], nray, work_b, profile_in_b, profile_b);
  return 0;
}
#endif
