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

int fused_tables(const rays_params_t* p, rays::DevParams& D) {
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
  rays::TraceArgs A = rays::TraceArgs();  // residual = nullptr
  A.nray = nray; A.rvec0 = rvec0; A.rindex_vec0 = rindex_vec0;
  A.npoints = npoints; A.stop_code = stop_code; A.set_start_ray_vec(start_ray_vec); A.end_ray_vec = end_ray_vec;
  A.end_residuals = end_residuals; A.max_residuals = max_residuals; A.next_ray = counter;
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
  std::vector<double> sg_far(512, 0.0);  // one lane: the SG kernels' upper-tier workspace
  A.sg_far = sg_far.data(); A.sg_far_lanes = 1;
  rays::DevParams D = make_dev_params(*p);
  if (int rc = fused_tables(p, D)) return rc;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0), d = p->ray_deriv, s = p->ode_solver;
  const rays::DevParams& D_ = D;
  int rc = 4;
  if (p->multi_spec_damping) {
    if (e == 4 && d == 0) rc = run_ms<4 | rays::kEqMultiSpec | FD, 0>(s, p->nspec + 1, p->nv, D_, A);
  } else if (p->nspec + 1 == 2 && (p->nv == 8 || p->nv == 13)) {
    const int nv = p->nv;
#define RAYS_EMUL_CASE(E, DV)                                                      \
  if (e == E && d == DV)                                                           \
    rc = nv == 8 ? run1<E | FD, DV, 2, 8>(s, D_, A) : run1<E | FD, DV, 2, 13>(s, D_, A);
    RAYS_EMUL_CASE(0, 0) RAYS_EMUL_CASE(0, 1) RAYS_EMUL_CASE(2, 0) RAYS_EMUL_CASE(2, 1)
    RAYS_EMUL_CASE(4, 0) RAYS_EMUL_CASE(4, 1) RAYS_EMUL_CASE(6, 0) RAYS_EMUL_CASE(6, 1)
#undef RAYS_EMUL_CASE
  }
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
  if (kind == 0 && stride > 1) {
    sched.assign(4 + (size_t)rays::sched_pilots((unsigned)nray, stride), 0u);
    A.sched = sched.data();
    A.sched_stride = stride;
  }
  rays::DevParams D = make_dev_params(*p);
  if (int rc = fused_tables(p, D)) return rc;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0), ns = p->nspec + 1, nv = p->nv;
  int rc = 4;
  if (kind == 0) {
    g_rk4_w2_body = 0;
    if (e == 6 && ns == 2 && nv == 8) rc = run_rk4_waves<6 | FD, 2, 8>(D, A, blocks);
    else if (e == 4 && ns == 2 && nv == 8) rc = run_rk4_waves<4 | FD, 2, 8>(D, A, blocks);
  } else {
    if (e == 6 && ns == 2 && nv == 8) rc = run_sg_waves<6 | FD, 2, 8>(D, A, blocks);
  }
  if (rc) return rc;
  fused_profile(n_bins, nray, work, profile_in, profile);
  return 0;
}
#endif
