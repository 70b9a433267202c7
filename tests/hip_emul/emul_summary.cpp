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
struct SummaryOut {
  int32_t *npoints, *stop_code;
  double *start_ray_vec, *end_ray_vec, *end_residuals, *max_residuals;
};
rays::TraceArgs summary_args(int nray, const double* rvec0, const double* rindex_vec0, const SummaryOut& o,
                             unsigned* counter) {
  rays::TraceArgs A = rays::TraceArgs();  // ray_vec = residual = nullptr
  A.nray = nray; A.rvec0 = rvec0; A.rindex_vec0 = rindex_vec0;
  A.npoints = o.npoints; A.stop_code = o.stop_code; A.set_start_ray_vec(o.start_ray_vec); A.end_ray_vec = o.end_ray_vec;
  A.end_residuals = o.end_residuals; A.max_residuals = o.max_residuals; A.next_ray = counter;
  return A;
}
int summary_tables(const rays_params_t* p, rays::DevParams& D) {
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
constexpr int NT = rays::kEqNoTraj;
}  // namespace

#ifndef RAYS_EMUL_SUMMARY_WAVE
// One emulated lane: the launch of rays_hip_trace_summary_device, or with ds_run / rays_per_run of
// rays_hip_scan_summary_device.  The same kernel selection as rays_emul_trace_ex, with kEqNoTraj in EQ.
extern "C" int rays_emul_summary_trace(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                                       int32_t* npoints, int32_t* stop_code, double* start_ray_vec, double* end_ray_vec,
                                       double* end_residuals, double* max_residuals, const double* ds_run,
                                       int rays_per_run) {
  unsigned counter = 0;
  rays::TraceArgs A = summary_args(nray, rvec0, rindex_vec0,
                                   SummaryOut{npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals},
                                   &counter);
  A.ds_run = ds_run; A.rays_per_run = rays_per_run;
  std::vector<double> sg_far(512, 0.0);  // one lane: the SG kernels' upper-tier workspace
  A.sg_far = sg_far.data(); A.sg_far_lanes = 1;
  rays::DevParams D = make_dev_params(*p);
  if (int rc = summary_tables(p, D)) return rc;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0), d = p->ray_deriv, s = p->ode_solver;
  const rays::DevParams& D_ = D;
  if (p->multi_spec_damping) {
    if (e == 5 && d == 0) return run_ms<5 | rays::kEqMultiSpec | NT, 0>(s, p->nspec + 1, p->nv, D_, A);
    if (e == 4 && d == 0) return run_ms<4 | rays::kEqMultiSpec | NT, 0>(s, p->nspec + 1, p->nv, D_, A);
    return 4;
  }
#define RAYS_EMUL_CASE(E, D) if (e == E && d == D) return run<E | NT, D>(s, p->nspec + 1, p->nv, D_, A); else
  RAYS_EMUL_CASE(0, 0) RAYS_EMUL_CASE(0, 1) RAYS_EMUL_CASE(1, 0) RAYS_EMUL_CASE(1, 1) RAYS_EMUL_CASE(2, 0) RAYS_EMUL_CASE(2, 1)
  RAYS_EMUL_CASE(4, 0) RAYS_EMUL_CASE(4, 1) RAYS_EMUL_CASE(5, 0) RAYS_EMUL_CASE(5, 1) RAYS_EMUL_CASE(6, 0) RAYS_EMUL_CASE(6, 1)
  return 4;
#undef RAYS_EMUL_CASE
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
  rays::TraceArgs A = summary_args(nray, rvec0, rindex_vec0,
                                   SummaryOut{npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals},
                                   &counter);
  std::vector<unsigned> sched;
  if (kind == 0 && stride_or_G > 1) {
    sched.assign(4 + (size_t)rays::sched_pilots((unsigned)nray, stride_or_G), 0u);
    A.sched = sched.data();
    A.sched_stride = stride_or_G;
  }
  rays::DevParams D = make_dev_params(*p);
  if (int rc = summary_tables(p, D)) return rc;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0), ns = p->nspec + 1, nv = p->nv;
  if (kind <= 1) {
    g_rk4_w2_body = kind;
#define RAYS_RK4W_CASE(E, N, V) if (e == E && ns == N && nv == V) return run_rk4_waves<E | NT, N, V>(D, A, blocks);
    RAYS_RK4W_CASE(4, 2, 7) RAYS_RK4W_CASE(5, 2, 7) RAYS_RK4W_CASE(6, 2, 8)
#undef RAYS_RK4W_CASE
  } else if (kind == 2) {
#define RAYS_SGW_CASE(E, N, V) if (e == E && ns == N && nv == V) return run_sg_waves<E | NT, N, V>(D, A, blocks);
    RAYS_SGW_CASE(5, 2, 7) RAYS_SGW_CASE(6, 2, 8)
#undef RAYS_SGW_CASE
  } else if (nv == 7) {
#define RAYS_GRP_CASE(E, N) if (e == E && ns == N) return run_group_g<E | NT, N>(stride_or_G, D, A, blocks);
    RAYS_GRP_CASE(4, 3) RAYS_GRP_CASE(5, 2)
#undef RAYS_GRP_CASE
  }
  return 4;
}
#endif
