// TEST INFRASTRUCTURE ONLY: the CONTINUATION variant of the product trace kernels (EQ | kEqContinue [| kEqNoTraj]:
// windowed tracing; rays_amd/csrc/rays_trace.hpp: TraceArgs::state, state_init_ray) on the host emulation, for
// tests/test_cpu_window_trace.py.  The argument block is filled as rays_capi.hip: launch_trace fills it for
// rays_hip_state_init_device and rays_hip_trace_window_device.
//   (no switch)              one emulated lane
//   -DRAYS_EMUL_WINDOW_WAVE  whole emulated waves (emul_group.cpp's runners): RK4 with refills and the SG kernel
// Built with -DRAYS_RK4_NO_HANDOVER: emul_trace.cpp switches the tolerance kernels' hand-over on for the emulation, and
// the continuation kernels exist in the exact arithmetic only.
#ifndef RAYS_RK4_NO_HANDOVER
#error "compile with -DRAYS_RK4_NO_HANDOVER: the continuation kernels are exact kernels"
#endif
#ifdef RAYS_EMUL_WINDOW_WAVE
#include "emul_group.cpp"
#else
#include "emul_trace.cpp"
#endif

namespace {
constexpr int CT = rays::kEqContinue, NT = rays::kEqNoTraj;

// the saved ray state as the caller's seven arrays (include/rays_hip.h: rays_ray_state_t)
struct StateArrays {
  double *v, *s;
  int32_t *nstep, *stop_code;
  double *resid, *sg_err;
  int32_t* flags;
};
// mode 0: rays_hip_state_init_device (start_ray_vec: point 1, may be null); 1: rays_hip_trace_window_device with the
// two window arrays; 2: without them (the summary policy)
rays::TraceArgs window_args(int mode, int nray, const double* rvec0, const double* rindex_vec0, const StateArrays& s,
                            int n_steps, double* ray_vec_win, double* residual_win, int32_t* npoints_win,
                            double* start_ray_vec, unsigned* counter) {
  // a recording window alone has the two window arrays; no per-ray summary is written (the state carries them)
  rays::TraceArgs A = emul_trace_args(nray, rvec0, rindex_vec0,
                                      EmulOut{mode == 1 ? ray_vec_win : nullptr, mode == 1 ? residual_win : nullptr,
                                              npoints_win, nullptr, start_ray_vec, nullptr, nullptr, nullptr}, counter);
  A.set_state(rays::TraceArgs::State{s.v, s.s, s.nstep, s.stop_code, s.resid, s.sg_err, s.flags}, n_steps);
  return A;
}
}  // namespace

#ifndef RAYS_EMUL_WINDOW_WAVE
namespace {
template <int EQ, int DERIV, int NS, int NV>
int window1(int mode, int solver, const rays::DevParams& D, const rays::TraceArgs& A) {
  threadIdx.x = 0; blockIdx.x = 0; blockDim.x = 1; gridDim.x = 1;
  if (mode == 0) {
    for (int ray = 0; ray < A.nray; ray++) rays::state_init_ray<EQ | CT, NS, DERIV, NV>(D, A, ray);
  } else if (solver == 0) {
    if (mode == 1) rays::rk4_trace_kernel<EQ | CT, NS, DERIV, NV>(D, A);
    else rays::rk4_trace_kernel<EQ | CT | NT, NS, DERIV, NV>(D, A);
  } else {
    if (mode == 1) rays::sg_trace_kernel<EQ | CT, NS, DERIV, NV>(D, A);
    else rays::sg_trace_kernel<EQ | CT | NT, NS, DERIV, NV>(D, A);
  }
  return 0;
}
}  // namespace

extern "C" int rays_emul_window(const rays_params_t* p, int mode, int nray, const double* rvec0,
                                const double* rindex_vec0, double* st_v, double* st_s, int32_t* st_nstep,
                                int32_t* st_stop_code, double* st_resid, double* st_sg_err, int32_t* st_flags, int n_steps,
                                double* ray_vec_win, double* residual_win, int32_t* npoints_win, double* start_ray_vec) {
  if (mode < 0 || mode > 2) return 1;
  unsigned counter = 0;
  rays::TraceArgs A = window_args(mode, nray, rvec0, rindex_vec0,
                                  StateArrays{st_v, st_s, st_nstep, st_stop_code, st_resid, st_sg_err, st_flags}, n_steps,
                                  ray_vec_win, residual_win, npoints_win, start_ray_vec, &counter);
  std::vector<double> sg_far;
  emul_one_lane_far(A, sg_far);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  return emul_lane_dispatch<AllShapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return window1<S::EQ, S::DERIV, S::NS, S::NV>(mode, p->ode_solver, D, A);
  });
}
#else
// Whole emulated waves, window launches only (modes 1 and 2).  kind 0: rk4_trace_kernel, 2: sg_trace_kernel, `blocks`
// waves of 64 lanes each; stride: the "long rays first" neighbourhood size of the RK4 kernel (0 | 1: index order).
extern "C" int rays_emul_window_waves(const rays_params_t* p, int mode, int kind, int blocks, int stride, int nray,
                                      double* st_v, double* st_s, int32_t* st_nstep, int32_t* st_stop_code,
                                      double* st_resid, double* st_sg_err, int32_t* st_flags, int n_steps,
                                      double* ray_vec_win, double* residual_win, int32_t* npoints_win) {
  if ((mode != 1 && mode != 2) || (kind != 0 && kind != 2) || blocks < 1 || p->multi_spec_damping) return 1;
  if (p->ode_solver != (kind == 0 ? RAYS_ODE_RK4 : RAYS_ODE_SG) || p->ray_deriv != RAYS_DERIV_COLD) return 1;
  unsigned counter = 0;
  rays::TraceArgs A = window_args(mode, nray, nullptr, nullptr,
                                  StateArrays{st_v, st_s, st_nstep, st_stop_code, st_resid, st_sg_err, st_flags}, n_steps,
                                  ray_vec_win, residual_win, npoints_win, nullptr, &counter);
  std::vector<unsigned> sched;
  if (kind == 0) emul_sched(A, sched, stride);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  // (run_rk4_waves leaves the two-waves-per-SIMD body and the hand-over out of a continuation build)
  if (kind == 0)
    return emul_wave_dispatch<UnitExpWaves>(Rk4WaveShapes{}, p, [&](auto sh) {
      typedef decltype(sh) S;
      return mode == 1 ? run_rk4_waves<S::EQ | CT, S::NS, S::NV>(D, A, blocks)
                       : run_rk4_waves<S::EQ | CT | NT, S::NS, S::NV>(D, A, blocks);
    });
  return emul_wave_dispatch<UnitExpWaves>(SgWaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return mode == 1 ? run_sg_waves<S::EQ | CT, S::NS, S::NV>(D, A, blocks)
                     : run_sg_waves<S::EQ | CT | NT, S::NS, S::NV>(D, A, blocks);
  });
}
#endif
