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
#include <type_traits>

namespace {
int window_tables(const rays_params_t* p, rays::DevParams& D) {
  if (p->damping_model) {
    if (g_zfun.empty()) return 2;
    D.zf_fspl = g_zfun.data(); D.zf_nx = g_zf_nx; D.zf_xmin = g_zf_xmin; D.zf_xmax = g_zf_xmax;
  }
  if (p->equilib_model != RAYS_EQ_AXISYM) return 0;
  if (p->axisym.magnetics_model == RAYS_AXI_MAG_EQDSK_SPLINE && (g_axi[2].empty() || g_axi_lin)) return 3;
  if (p->axisym.magnetics_model == RAYS_AXI_MAG_EQDSK_LIN && (g_axi[2].empty() || !g_axi_lin)) return 3;
  D.a_lin_dR = g_axi_dR; D.a_lin_dZ = g_axi_dZ;
  D.a_nr = g_axi_n[0]; D.a_nz = g_axi_n[1]; D.a_n_rb = g_axi_n[2]; D.a_n_ne = g_axi_n[3]; D.a_n_te = g_axi_n[4]; D.a_n_ti = g_axi_n[5];
  D.a_r_grid = g_axi[0].data(); D.a_z_grid = g_axi[1].data(); D.a_psi_fspl = g_axi[2].data();
  D.a_rb_grid = g_axi[3].data(); D.a_rb_fspl = g_axi[4].data(); D.a_ne_grid = g_axi[5].data(); D.a_ne_fspl = g_axi[6].data();
  D.a_te_grid = g_axi[7].data(); D.a_te_fspl = g_axi[8].data(); D.a_ti_grid = g_axi[9].data(); D.a_ti_fspl = g_axi[10].data();
  set_spline_axes(D, D.a_r_grid, D.a_z_grid, D.a_rb_grid, D.a_ne_grid, D.a_te_grid, D.a_ti_grid);
  return 0;
}
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
  rays::TraceArgs A = rays::TraceArgs();
  A.nray = nray; A.rvec0 = rvec0; A.rindex_vec0 = rindex_vec0; A.next_ray = counter;
  A.ray_vec = mode == 1 ? ray_vec_win : nullptr;
  A.residual = mode == 1 ? residual_win : nullptr;
  A.npoints = npoints_win;
  A.set_start_ray_vec(start_ray_vec);
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
// the shapes emul_trace.cpp instantiates (run<> / run_ms<> there)
template <int EQ, int DERIV>
int window_shape(int mode, int solver, int ns, int nv, const rays::DevParams& D, const rays::TraceArgs& A) {
#define RAYS_W1(N, V) if (ns == N && nv == V) return window1<EQ, DERIV, N, V>(mode, solver, D, A);
  if constexpr ((EQ & rays::kEqMultiSpec) != 0) {
    if constexpr ((EQ & 3) == 1) { RAYS_W1(2, 10) }
    if constexpr ((EQ & 3) == 0) { RAYS_W1(2, 15) }
  } else {
    RAYS_W1(2, 7) RAYS_W1(2, 8) RAYS_W1(2, 12) RAYS_W1(2, 13)
    if constexpr ((EQ & 3) == 0) { RAYS_W1(1, 7) RAYS_W1(3, 7) RAYS_W1(6, 7) }
    if constexpr ((EQ & 3) == 1) { RAYS_W1(4, 7) }
  }
#undef RAYS_W1
  return 1;
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
  std::vector<double> sg_far(512, 0.0);  // one lane: the SG kernels' upper-tier workspace
  A.sg_far = sg_far.data(); A.sg_far_lanes = 1;
  rays::DevParams D = make_dev_params(*p);
  if (int rc = window_tables(p, D)) return rc;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0), d = p->ray_deriv, s = p->ode_solver;
  const int ns = p->nspec + 1, nv = p->nv;
  if (p->multi_spec_damping) {
    if (e == 5 && d == 0) return window_shape<5 | rays::kEqMultiSpec, 0>(mode, s, ns, nv, D, A);
    if (e == 4 && d == 0) return window_shape<4 | rays::kEqMultiSpec, 0>(mode, s, ns, nv, D, A);
    return 4;
  }
#define RAYS_EMUL_CASE(E, DV) if (e == E && d == DV) return window_shape<E, DV>(mode, s, ns, nv, D, A); else
  RAYS_EMUL_CASE(0, 0) RAYS_EMUL_CASE(0, 1) RAYS_EMUL_CASE(1, 0) RAYS_EMUL_CASE(1, 1) RAYS_EMUL_CASE(2, 0) RAYS_EMUL_CASE(2, 1)
  RAYS_EMUL_CASE(4, 0) RAYS_EMUL_CASE(4, 1) RAYS_EMUL_CASE(5, 0) RAYS_EMUL_CASE(5, 1) RAYS_EMUL_CASE(6, 0) RAYS_EMUL_CASE(6, 1)
  return 4;
#undef RAYS_EMUL_CASE
}
#else
// emul_group.cpp's run_rk4_waves without its second arm: the two-waves-per-SIMD body has no continuation variant
template <int EQ, int NS, int NV>
static int run_rk4_window_waves(const rays::DevParams& D, const rays::TraceArgs& A, int nwaves) {
  gridDim.x = (unsigned)nwaves;
  blockDim.x = 64;
  for (int b = 0; b < nwaves; b++) {
    blockIdx.x = (unsigned)b;
    wave_emul::run_wave(0u, [&] { rays::rk4_trace_kernel<EQ, NS, 0, NV>(D, A); }, threadIdx);
  }
  return 0;
}
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
  if (kind == 0 && stride > 1) {
    sched.assign(4 + (size_t)rays::sched_pilots((unsigned)nray, stride), 0u);
    A.sched = sched.data();
    A.sched_stride = stride;
  }
  rays::DevParams D = make_dev_params(*p);
  if (int rc = window_tables(p, D)) return rc;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0), ns = p->nspec + 1, nv = p->nv;
#define RAYS_WW_CASE(RUN, E, N, V)                                              \
  if (e == E && ns == N && nv == V)                                             \
    return mode == 1 ? RUN<E | CT, N, V>(D, A, blocks) : RUN<E | CT | NT, N, V>(D, A, blocks);
  if (kind == 0) {
    RAYS_WW_CASE(run_rk4_window_waves, 4, 2, 7) RAYS_WW_CASE(run_rk4_window_waves, 5, 2, 7)
    RAYS_WW_CASE(run_rk4_window_waves, 6, 2, 8)
  } else {
    RAYS_WW_CASE(run_sg_waves, 5, 2, 7) RAYS_WW_CASE(run_sg_waves, 6, 2, 8)
  }
#undef RAYS_WW_CASE
  return 4;
}
#endif
