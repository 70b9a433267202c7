// TEST INFRASTRUCTURE ONLY: the CONTINUATION variant of the fused deposition kernels (EQ | kEqContinue | kEqNoTraj |
// kEqDeposit [| kEqDeposit2]: a window that bins what it accepts) on the host emulation, for
// tests/test_cpu_window_deposition.py.  The argument block is filled as rays_capi.hip fills it for
// rays_hip_trace_window_profiles_device: the saved state in the slots TraceArgs::state() names, the DepTraceArgs /
// Dep2TraceArgs block in the ray_vec slot, residual null -- and NO work row is zeroed here: the rows are accumulators.
// The library also holds the one-shot entries of emul_fused_profiles.cpp and emul_fused_deposition.cpp, so a comparison
// takes both paths from one library and one set of tables.
//   (no switch)                  one emulated lane; also rays_hip_state_init_device's launch (mode 0)
//   -DRAYS_EMUL_DEPOSIT_WAVE     whole emulated waves: RK4 with refills, SG
#include "emul_fused_profiles.cpp"

namespace {
constexpr int WD = rays::kEqContinue | FD, WD2 = rays::kEqContinue | FD2;

struct WinDepBlocks {
  rays::DepTraceArgs one;
  rays::Dep2TraceArgs two;
};
// n_profiles 1 | 2: which[], n_bins[], work[] as the records of the call; nothing is zeroed
bool windep_blocks(const rays_params_t* p, int n_profiles, const int* which, const int* n_bins, const double* power,
                   const double* rho_grid, const double* rho_fspl, int n_rho, double* const* work, WinDepBlocks* B) {
  if (n_profiles == 1) {
    if (fused_refused(p, which[0], n_bins[0])) return false;
    rays::DepTraceArgs& T = B->one;
    T.which = which[0]; T.n_bins = n_bins[0];
    T.grid_min = 0.; T.grid_max = 1.;
    if (which[0] == RAYS_DEP_PTOTAL_X) { T.grid_min = p->slab.xmin; T.grid_max = p->slab.xmax; }
    T.power = power; T.work = work[0]; T.rho_grid = rho_grid; T.rho_fspl = rho_fspl; T.n_rho = n_rho; T.pad_ = 0;
    return true;
  }
  if (n_profiles != 2 || fused2_refused(p, which, n_bins)) return false;
  rays::Dep2TraceArgs& T = B->two;
  for (int i = 0; i < 2; i++) {
    T.prof[i].which = which[i]; T.prof[i].n_bins = n_bins[i];
    T.prof[i].grid_min = 0.; T.prof[i].grid_max = 1.;
    T.prof[i].work = work[i];
  }
  T.power = power; T.rho_grid = rho_grid; T.rho_fspl = rho_fspl; T.n_rho = n_rho; T.pad_ = 0;
  return true;
}
// the launch's TraceArgs: no trajectory array, no per-ray summary (the state carries them), npoints = npoints_win
rays::TraceArgs windep_args(int nray, const double* rvec0, const double* rindex_vec0, double* st_v, double* st_s,
                            int32_t* st_nstep, int32_t* st_stop_code, double* st_resid, double* st_sg_err,
                            int32_t* st_flags, int n_steps, int32_t* npoints_win, double* start_ray_vec, unsigned* counter) {
  rays::TraceArgs A = emul_trace_args(nray, rvec0, rindex_vec0,
                                      EmulOut{nullptr, nullptr, npoints_win, nullptr, start_ray_vec, nullptr, nullptr, nullptr},
                                      counter);
  A.set_state(rays::TraceArgs::State{st_v, st_s, st_nstep, st_stop_code, st_resid, st_sg_err, st_flags}, n_steps);
  return A;
}
}  // namespace

#ifndef RAYS_EMUL_DEPOSIT_WAVE
namespace {
template <int EQ, int DERIV, int NS, int NV>
int windep1(int mode, int n_profiles, int solver, const rays::DevParams& D, const rays::TraceArgs& A) {
  threadIdx.x = 0; blockIdx.x = 0; blockDim.x = 1; gridDim.x = 1;
  if (mode == 0) {
    for (int ray = 0; ray < A.nray; ray++) rays::state_init_ray<EQ | rays::kEqContinue, NS, DERIV, NV>(D, A, ray);
  } else if (n_profiles == 2) {
    if constexpr (Fused2Shapes::lane<EQ, DERIV, NS, NV>) {
      if (solver == 0) rays::rk4_trace_kernel<EQ | WD2, NS, DERIV, NV>(D, A);
      else rays::sg_trace_kernel<EQ | WD2, NS, DERIV, NV>(D, A);
    } else {
      return 4;
    }
  } else {
    if (solver == 0) rays::rk4_trace_kernel<EQ | WD, NS, DERIV, NV>(D, A);
    else rays::sg_trace_kernel<EQ | WD, NS, DERIV, NV>(D, A);
  }
  return 0;
}
}  // namespace

// One emulated lane.  mode 0: rays_hip_state_init_device (rvec0, rindex_vec0, start_ray_vec; the profile arguments are
// not looked at); mode 1: rays_hip_trace_window_profiles_device without its profile sums.  work_a / work_b bin-major.
extern "C" int rays_emul_window_deposition(const rays_params_t* p, int mode, int nray, const double* rvec0,
                                           const double* rindex_vec0, double* st_v, double* st_s, int32_t* st_nstep,
                                           int32_t* st_stop_code, double* st_resid, double* st_sg_err, int32_t* st_flags,
                                           int n_steps, const double* power, int n_profiles, const int* which,
                                           const int* n_bins, const double* rho_grid, const double* rho_fspl, int n_rho,
                                           double* work_a, double* work_b, int32_t* npoints_win, double* start_ray_vec) {
  if (mode != 0 && mode != 1) return 1;
  unsigned counter = 0;
  rays::TraceArgs A = windep_args(nray, rvec0, rindex_vec0, st_v, st_s, st_nstep, st_stop_code, st_resid, st_sg_err, st_flags,
                                  n_steps, npoints_win, start_ray_vec, &counter);
  WinDepBlocks B;
  if (mode == 1) {
    double* const work[2] = {work_a, work_b};
    if (n_steps < 1 || !power || !windep_blocks(p, n_profiles, which, n_bins, power, rho_grid, rho_fspl, n_rho, work, &B))
      return 5;
    if (n_profiles == 2) A.set_dep2(&B.two);
    else A.set_dep(&B.one);
  }
  std::vector<double> sg_far;
  emul_one_lane_far(A, sg_far);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  return emul_lane_dispatch<FusedShapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return windep1<S::EQ, S::DERIV, S::NS, S::NV>(mode, n_profiles, p->ode_solver, D, A);
  });
}
#else
// Whole emulated waves, window launches only (kind, blocks, stride: as rays_emul_fused_deposition_waves).
extern "C" int rays_emul_window_deposition_waves(const rays_params_t* p, int kind, int blocks, int stride, int nray,
                                                 double* st_v, double* st_s, int32_t* st_nstep, int32_t* st_stop_code,
                                                 double* st_resid, double* st_sg_err, int32_t* st_flags, int n_steps,
                                                 const double* power, int n_profiles, const int* which, const int* n_bins,
                                                 const double* rho_grid, const double* rho_fspl, int n_rho, double* work_a,
                                                 double* work_b, int32_t* npoints_win) {
  if ((kind != 0 && kind != 2) || blocks < 1 || p->multi_spec_damping || n_steps < 1 || !power) return 1;
  if (p->ode_solver != (kind == 0 ? RAYS_ODE_RK4 : RAYS_ODE_SG) || p->ray_deriv != RAYS_DERIV_COLD) return 1;
  unsigned counter = 0;
  rays::TraceArgs A = windep_args(nray, nullptr, nullptr, st_v, st_s, st_nstep, st_stop_code, st_resid, st_sg_err, st_flags,
                                  n_steps, npoints_win, nullptr, &counter);
  WinDepBlocks B;
  double* const work[2] = {work_a, work_b};
  if (!windep_blocks(p, n_profiles, which, n_bins, power, rho_grid, rho_fspl, n_rho, work, &B)) return 5;
  if (n_profiles == 2) A.set_dep2(&B.two);
  else A.set_dep(&B.one);
  std::vector<unsigned> sched;
  if (kind == 0) emul_sched(A, sched, stride);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  g_rk4_w2_body = 0;
  if (n_profiles == 2)
    return kind == 0 ? emul_wave_dispatch<Fused2Shapes>(Rk4WaveShapes{}, p, [&](auto sh) {
      typedef decltype(sh) S;
      return run_rk4_waves<S::EQ | WD2, S::NS, S::NV>(D, A, blocks);
    }) : emul_wave_dispatch<Fused2Shapes>(SgWaveShapes{}, p, [&](auto sh) {
      typedef decltype(sh) S;
      return run_sg_waves<S::EQ | WD2, S::NS, S::NV>(D, A, blocks);
    });
  return kind == 0 ? emul_wave_dispatch<FusedShapes>(Rk4WaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_rk4_waves<S::EQ | WD, S::NS, S::NV>(D, A, blocks);
  }) : emul_wave_dispatch<FusedShapes>(SgWaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_sg_waves<S::EQ | WD, S::NS, S::NV>(D, A, blocks);
  });
}
#endif
