// rays_deposition.hpp -- deposition profiles on the device: the step right
// after the hot path, applied to the trajectories while they are still resident in HBM.
//
// Reference path restated here:
//   calculate_deposition_profiles / bin_a_ray   post_process_lib/deposition_profiles_m.f90:228-292
//   Ptotal_axisym_psi_evaluator / _rho_         deposition_profiles_m.f90:458-503
//   binner_real (bin_to_uniform_grid)           math_functions_lib/bin_to_uniform_grid_m.f90
//   eqdsk_magnetics_spline_interp_psi / _rho    eqdsk_magnetics_spline_interp_m.f90:286-352
//
// One thread bins one ray (the binner walks the ray's points in order) into a row held in LDS and
// writes it to work[bin][ray] (bin-major, so both this write and the reduction read coalesce).
// The profile is then the sum over rays IN RAY ORDER -- the order of the reference's sum(work, 2);
// floating-point addition is not associative -- one wave per bin: the lanes load 64 consecutive
// rays at a time and the running sum walks through them with v_readlane.  It can be continued from
// another rank's partial sums, so the multi-GPU result is bit-identical to the single-process one.
#pragma once

#include "rays_device.hpp"

namespace rays {

struct DepArgs {
  int which;  // RAYS_DEP_PTOTAL_PSI | RAYS_DEP_PTOTAL_RHO | RAYS_DEP_PTOTAL_X
  int n_bins, nray, nv, npt;
  double grid_min, grid_max;
  const double* ray_vec;   // [nray][npt][nv]
  const int* npoints;      // [nray]
  const double* power;     // initial_ray_power[nray]
  const double* rho_grid;  // rho(psiN) spline (Ptotal_rho)
  const double* rho_fspl;
  int n_rho;
  double* work;            // [n_bins][nray]
};

// grid value of a ray point: psiN or rho(psiN) at (x, y, z); x itself for the slab's Ptotal_x
RAYS_DEV double dep_grid_value(const DevParams& P, const DepArgs& D, const double* v) {
  const double x = v[0], y = v[1], z = v[2];
  if (D.which == 2) return x;  // Ptotal_x_slab_evaluator (deposition_profiles_m.f90:449)
  const double r = sqrt(x * x + y * y);
  double f6[6];
  double psiN;
  if (P.a_mag_model == RAYS_AXI_MAG_SOLOVEV) {  // axisym_toroid_psi -> solovev_magnetics_psi (solovev_magnetics_m.f90:199-207)
    const double psi = P.half_bp0 * (sq(r * z / P.rk) + sq(r * r - P.rmaj2) / P.rmaj2 / 4.);
    psiN = psi / P.psiB;
  } else if (P.a_mag_model == RAYS_AXI_MAG_EQDSK_LIN) {  // eqdsk_magnetics_lin_interp_psi: GetPsi / PSIBOUND
    psiN = eqlin_getpsi(P, r, z) / P.a_psiB;
  } else {
    spl2_fpp(P, r, z, f6);
    psiN = f6[0] / P.a_psiB;  // psiN = Psi/PSIBOUND (:314)
  }
  if (D.which == 0) return psiN;
  double rho, drho;
  spl1_fp(D.rho_grid, D.rho_fspl, D.n_rho, psiN, rho, drho);
  return rho;
}

// (int)floor(x) of a bin coordinate, as the DEVICE converts it: v_cvt_i32_f64 saturates and turns NaN into 0.  A NaN grid
// value -- 'Ptotal_rho' with a rho(psiN) spline the host could not build (tests/golden: the 129 x 129 eqdsk) -- thereby
// puts the segment into bin 1, which is what the reference's binner does with it.  The C++ conversion is undefined
// there, so the host emulation restates the device's.
RAYS_DEV int dep_floor_index(double x) {
#ifdef RAYS_HOST_EMUL
  const double f = floor(x);
  if (f != f) return 0;
  if (f >= 2147483647.0) return 2147483647;
  if (f <= -2147483648.0) return -2147483647 - 1;
  return (int)f;
#else
  return (int)floor(x);
#endif
}

// One segment of binner_real: the absorbed power gained between two consecutive recorded points, (x_prev, q_prev) ->
// (xq, q), spread over the bins of row[b * stride], b = 0..n_bins-1, that the segment covers.  The body of deposit_ray's
// point loop, and what the fused trace kernels (kEqDeposit: rays_rk4_body.inc, rays_sg.hpp) call when a point is accepted
// -- the same statements in the same order, so a row comes out the same bits whichever of the two walks the ray.
template <class RowPtr, class Stride>
RAYS_DEV void deposit_segment(RowPtr row_base, Stride stride, int n_bins, double xmin, double xmax, double x_prev,
                              double q_prev, double xq, double q) {
  struct Row {
    RowPtr p;
    Stride st;
    RAYS_DEV auto& operator[](int b) const { return p[b * st]; }
  } row{row_base, stride};
  const double x_bin_width = (xmax - xmin) / (double)n_bins;
  double x_low = fmin(x_prev, xq), x_high = fmax(x_prev, xq);
  double ix_low = (x_low - xmin) / x_bin_width, ix_high = (x_high - xmin) / x_bin_width;
  const double delta_ix = ix_high - ix_low;
  int index_low = dep_floor_index(ix_low) + 1, index_high = dep_floor_index(ix_high) + 1;
  if (x_high >= xmax) index_high = n_bins;
  int delta_i = index_high - index_low;
  double delta_Q = q - q_prev;
  const double Q_density = delta_Q / delta_ix;
  bool skip = fabs(delta_Q) < 4.0 * 2.2250738585072014e-308;  // 4.0_skind*tiny(delta_Q)
  if (x_high < xmin || x_low > xmax) skip = true;
  if (!skip) {
    if (x_low < xmin) {
      delta_Q = delta_Q * (ix_high / delta_ix);
      ix_low = 0.0;
      index_low = 1;
      delta_i = index_high - index_low;
    }
    if (x_high > xmax) {
      delta_Q = delta_Q * (((double)n_bins - ix_low) / delta_ix);
      ix_high = (double)n_bins;
      index_high = n_bins;
      delta_i = index_high - index_low;
    }
    if (delta_i == 0) {
      if (index_low >= 1 && index_low <= n_bins) row[index_low - 1] = row[index_low - 1] + delta_Q;
    } else if (delta_i > 0) {
      const double Q_incrL = delta_Q * (((double)index_low - ix_low) / delta_ix);
      row[index_low - 1] = row[index_low - 1] + Q_incrL;
      const double Q_incrH = delta_Q * ((ix_high - (double)(index_high - 1)) / delta_ix);
      // x_high just below xmax whose quotient rounds up to n_bins: index_high = n_bins + 1, one element past
      // the row (the reference updates binned_Q(n_bins + 1) there: undefined)
      if (index_high <= n_bins) row[index_high - 1] = row[index_high - 1] + Q_incrH;
      for (int i = index_low + 1; i <= index_high - 1; i++) row[i - 1] = row[i - 1] + Q_density;
    }
  }
}

// bin_a_ray + binner_real for ray `iray` into row[b * stride], b = 0..n_bins-1 (zeroed here, as the
// binner does)
template <class RowPtr>
RAYS_DEV void deposit_ray(const DevParams& P, const DepArgs& D, int iray, RowPtr row_base, int stride) {
  const int n_bins = D.n_bins;
  for (int b = 0; b < n_bins; b++) row_base[b * stride] = 0.;
  const int np = D.npoints[iray];
  const double* rv = D.ray_vec + (long long)iray * D.npt * D.nv;
  const double pw = D.power[iray];
  const double xmin = D.grid_min, xmax = D.grid_max;
  double x_prev = 0., q_prev = 0.;
  for (int is = 0; is < np; is++) {
    const double* v = rv + (long long)is * D.nv;
    const double xq = dep_grid_value(P, D, v);
    const double q = v[7] * pw;  // ray_vec(8)*initial_ray_power
    if (is > 0) deposit_segment(row_base, stride, n_bins, xmin, xmax, x_prev, q_prev, xq, q);
    x_prev = xq;
    q_prev = q;
  }
}

// ---- binning inside the trace kernels (kEqDeposit) -----------------------------------------------------
// What a fused trace kernel reads besides TraceArgs: a block in device memory, filled on the launch's stream right before
// the kernel (rays_deposition.hip: launch_dep_trace_args) and found through TraceArgs::dep().  Wave-uniform: scalar loads
// at the point of use.
struct DepTraceArgs {
  int which, n_bins;       // RAYS_DEP_PTOTAL_*; 1..RAYS_DEP_MAX_BINS
  double grid_min, grid_max;
  const double* power;     // initial_ray_power[nray]
  double* work;            // [n_bins][nray], zeroed before the launch; ray i owns work[b * nray + i]
  const double* rho_grid;  // rho(psiN) spline (Ptotal_rho)
  const double* rho_fspl;
  int n_rho, pad_;
};
static_assert(sizeof(DepTraceArgs) == 64, "DepTraceArgs: one 64-byte block");

// the post-processor's grid value and absorbed power of the ODE vector v of ray `ray`: dep_grid_value's own bits
RAYS_DEV void dep_trace_point(const DevParams& P, const DepTraceArgs& T, int ray, const double* v, double& xq, double& q) {
  DepArgs D;
  D.which = T.which;
  D.rho_grid = T.rho_grid;
  D.rho_fspl = T.rho_fspl;
  D.n_rho = T.n_rho;
  xq = dep_grid_value(P, D, v);
  q = v[7] * T.power[ray];  // ray_vec(8)*initial_ray_power
}
// an accepted point of ray `ray` (of nray): the segment from the ray's previous point into the ray's row of work
RAYS_DEV void dep_trace_segment(const DevParams& P, const DepTraceArgs& T, int ray, int nray, const double* v,
                                double& x_prev, double& q_prev) {
  double xq, q;
  dep_trace_point(P, T, ray, v, xq, q);
  deposit_segment(T.work + ray, (long long)nray, T.n_bins, T.grid_min, T.grid_max, x_prev, q_prev, xq, q);
  x_prev = xq;
  q_prev = q;
}

// ---- two profiles in one pass (kEqDeposit2) -----------------------------------------------------------
// The axisym_toroid post-processor bins every ray twice, on psiN and on rho(psiN) (deposition_profiles_m.f90:228-260).
// The two-profile variant of a fused trace kernel does both from ONE grid evaluation per accepted point: one q, two
// x_prev, one q_prev per lane.  Its argument block, written and found like DepTraceArgs:
struct Dep2Profile {
  int which, n_bins;       // RAYS_DEP_PTOTAL_PSI | RAYS_DEP_PTOTAL_RHO; 1..RAYS_DEP_MAX_BINS
  double grid_min, grid_max;
  double* work;            // [n_bins][nray], zeroed before the launch; ray i owns work[b * nray + i]
};
struct Dep2TraceArgs {
  Dep2Profile prof[2];     // in the caller's order; the two bin counts are independent
  const double* power;     // initial_ray_power[nray]
  const double* rho_grid;  // rho(psiN) spline
  const double* rho_fspl;
  int n_rho, pad_;
};
static_assert(sizeof(Dep2Profile) == 32 && sizeof(Dep2TraceArgs) == 96, "Dep2TraceArgs: two records + the shared part");

// psiN and rho(psiN) of a ray point from one evaluation: dep_grid_value's statements, so each has dep_grid_value's bits
RAYS_DEV void dep2_grid_values(const DevParams& P, const Dep2TraceArgs& T, const double* v, double& psiN, double& rho) {
  const double x = v[0], y = v[1], z = v[2];
  const double r = sqrt(x * x + y * y);
  double f6[6];
  if (P.a_mag_model == RAYS_AXI_MAG_SOLOVEV) {
    const double psi = P.half_bp0 * (sq(r * z / P.rk) + sq(r * r - P.rmaj2) / P.rmaj2 / 4.);
    psiN = psi / P.psiB;
  } else if (P.a_mag_model == RAYS_AXI_MAG_EQDSK_LIN) {
    psiN = eqlin_getpsi(P, r, z) / P.a_psiB;
  } else {
    spl2_fpp(P, r, z, f6);
    psiN = f6[0] / P.a_psiB;
  }
  double drho;
  spl1_fp(T.rho_grid, T.rho_fspl, T.n_rho, psiN, rho, drho);
}
// the two grid values, in the records' order, and the absorbed power of the ODE vector v of ray `ray`
RAYS_DEV void dep2_trace_point(const DevParams& P, const Dep2TraceArgs& T, int ray, const double* v, double& xa,
                               double& xb, double& q) {
  double psiN, rho;
  dep2_grid_values(P, T, v, psiN, rho);
  xa = T.prof[0].which == 0 ? psiN : rho;
  xb = T.prof[1].which == 0 ? psiN : rho;
  q = v[7] * T.power[ray];  // ray_vec(8)*initial_ray_power
}
// point 1 of ray `ray`: where its first segment starts on either grid
RAYS_DEV void dep2_trace_first(const DevParams& P, const Dep2TraceArgs& T, int ray, const double* v, double& xa_prev,
                               double& xb_prev, double& q_prev) {
  double xa, xb, q;
  dep2_trace_point(P, T, ray, v, xa, xb, q);
  xa_prev = xa;
  xb_prev = xb;  // (its own grid value: the two grids differ from the first point on)
  q_prev = q;
}
// an accepted point of ray `ray` (of nray): the segment from the ray's previous point into the ray's row of each work
RAYS_DEV void dep2_trace_segment(const DevParams& P, const Dep2TraceArgs& T, int ray, int nray, const double* v,
                                 double& xa_prev, double& xb_prev, double& q_prev) {
  double xa, xb, q;
  dep2_trace_point(P, T, ray, v, xa, xb, q);
  deposit_segment(T.prof[0].work + ray, (long long)nray, T.prof[0].n_bins, T.prof[0].grid_min, T.prof[0].grid_max, xa_prev,
                  q_prev, xa, q);
  deposit_segment(T.prof[1].work + ray, (long long)nray, T.prof[1].n_bins, T.prof[1].grid_min, T.prof[1].grid_max, xb_prev,
                  q_prev, xb, q);
  xa_prev = xa;
  xb_prev = xb;
  q_prev = q;
}

}  // namespace rays
