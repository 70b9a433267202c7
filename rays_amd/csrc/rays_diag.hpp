// rays_diag.hpp -- per-point ray diagnostics on the device: the post-processors' ray_detailed_diagnostics
// applied to the trajectories where the trace left them.
//
// Reference path restated here (one serial loop over every recorded point of every ray):
//   ray_detailed_diagnostics        post_process_lib/axisym_toroid_processor_m.f90:252-482 (the loop: :351-419)
//   ray_detailed_diagnostics_slab   post_process_lib/slab_processor_m.f90 (X, Y in place of Psi, R; same loop body)
// with equilibrium (equilibrium_m.f90:135-272), deriv_cold (deriv_cold.f90), damping -> damp_fund_ECH
// (damping_m.f90:74-117) and axisym_toroid_psi; all of them are the device functions of rays_device_arith.inc, in the
// exact arithmetic (this header is never compiled with RAYS_TOL_FLAVOUR: rays_hip_set_numerics does not reach it).
//
// Extensions and the one behavioural difference:
//   - nineteen fields: the union of the axisym set and the slab set;
//   - equilib_model = 'solovev' has no processor in the reference; PSI is then psiN of solovev_psi
//     (solovev_eq_m.f90:308-318), everything else is the same loop body;
//   - where the reference `stop`s the program (abs(dddw) <= tiny(dddw), :395-400) the point gets N_IMAG = 0 and
//     diag_point returns true: the caller records the ray's first such point (rays_hip.h: first_bad_point).
//
// One lane per POINT (diag_point), not per ray: the loop body has no dependence between points.
#pragma once

#include "rays_device.hpp"

namespace rays {

// fields whose value needs the equilibrium at the point; the rest are copies of the trajectory arrays (and R)
constexpr unsigned kDiagNeedsEq =
    (1u << RAYS_DIAG_NE) | (1u << RAYS_DIAG_TE_KEV) | (1u << RAYS_DIAG_MODB) | (1u << RAYS_DIAG_ALPHA_E) |
    (1u << RAYS_DIAG_GAMMA_E) | (1u << RAYS_DIAG_N_PAR) | (1u << RAYS_DIAG_N_PERP) | (1u << RAYS_DIAG_N_IMAG) |
    (1u << RAYS_DIAG_XI_0) | (1u << RAYS_DIAG_XI_1) | (1u << RAYS_DIAG_XI_2);
constexpr unsigned kDiagXi = (1u << RAYS_DIAG_XI_0) | (1u << RAYS_DIAG_XI_1) | (1u << RAYS_DIAG_XI_2);
constexpr unsigned kDiagAllFields = (1u << RAYS_DIAG_NFIELDS) - 1u;

// psiN at (x, y, z) with r = sqrt(x**2 + y**2): axisym_toroid_psi for the three magnetics models (the expression of
// rays_deposition.hpp: dep_grid_value), solovev_psi for equilib_model = 'solovev', 0 for the slab
template <int EQ>
RAYS_DEV double diag_psiN(const DevParams& P, double r, double z) {
  constexpr int MODEL = EQ & 3;
  if (MODEL == RAYS_EQ_SLAB) return 0.;
  if (MODEL == RAYS_EQ_SOLOVEV || P.a_mag_model == RAYS_AXI_MAG_SOLOVEV) {
    // solovev_eq_m.f90:308-318 / solovev_magnetics_m.f90:199-207
    const double psi = P.half_bp0 * (sq(r * z / P.rk) + sq(r * r - P.rmaj2) / P.rmaj2 / 4.);
    return psi / P.psiB;
  }
  if (P.a_mag_model == RAYS_AXI_MAG_EQDSK_LIN) return eqlin_getpsi(P, r, z) / P.a_psiB;  // GetPsi / PSIBOUND
  double f6[6];
  spl2_fpp(P, r, z, f6);
  return f6[0] / P.a_psiB;  // eqdsk_magnetics_spline_interp_m.f90:314
}

// The body of step_loop (axisym_toroid_processor_m.f90:353-417) at one recorded point.
//   v      : the point's row of ray_vec (v(1:7), and v(8) when the run has damping)
//   resid  : residual(istep, iray)
//   fields : bit f set = field RAYS_DIAG_<f> is wanted; out[f] of the other fields is left untouched, and what only
//            they need is not evaluated (wave-uniform branches)
// Returns true where the reference would stop the program ('infinite group velocity', :395-400).
template <int EQ, int NS>
RAYS_DEV bool diag_point(const DevParams& P, const double* v, double resid, unsigned fields,
                         double out[RAYS_DIAG_NFIELDS]) {
  const double rvec[3] = {v[0], v[1], v[2]}, kvec[3] = {v[3], v[4], v[5]};  // :355-357
  const bool damp = P.damping_model != RAYS_DAMP_NONE;
  const double r = fsqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1]);  // :360
  out[RAYS_DIAG_S] = v[6];                                        // :358
  out[RAYS_DIAG_R] = r;
  out[RAYS_DIAG_X] = rvec[0];
  out[RAYS_DIAG_Y] = rvec[1];
  out[RAYS_DIAG_Z] = rvec[2];                                     // :361
  out[RAYS_DIAG_RESIDUAL] = resid;                                // :378
  out[RAYS_DIAG_P_ABSORBED] = damp ? v[7] : 0.;                   // :404 (inside `damp`; allocated with source = 0)
  if (fields & (1u << RAYS_DIAG_PSI)) out[RAYS_DIAG_PSI] = diag_psiN<EQ>(P, r, rvec[2]);  // :370-371
  bool bad = false;
  if (fields & kDiagNeedsEq) {
    EqPoint<NS> eq;
    equilibrium<EQ, NS>(P, const_recip(P.omgrf, P.inv_omgrf), const_recip(P.omgrf2, P.inv_omgrf2), rvec, eq, false);  // :363
    const double e = (double)1.6022e-19f;  // constants_m.f90:48 (a default-real literal)
    out[RAYS_DIAG_TE_KEV] = fdiv(fdiv(eq.ts0, e), 1000.0);  // :364
    out[RAYS_DIAG_MODB] = eq.bmag;                          // :365
    out[RAYS_DIAG_ALPHA_E] = eq.alpha[0];                   // :366
    out[RAYS_DIAG_GAMMA_E] = fabs(eq.gamma[0]);             // :367
    out[RAYS_DIAG_NE] = eq.ns[0];                           // :368
    const Recip Rk0 = const_recip(P.k0, P.inv_k0);
    const double k3 = kvec[0] * eq.bunit[0] + kvec[1] * eq.bunit[1] + kvec[2] * eq.bunit[2];  // :373
    const double k1 = fsqrt(sq(kvec[0] - k3 * eq.bunit[0]) + sq(kvec[1] - k3 * eq.bunit[1]) +
                            sq(kvec[2] - k3 * eq.bunit[2]));                                   // :374
    out[RAYS_DIAG_N_PAR] = div(k3, Rk0);   // :375-376
    out[RAYS_DIAG_N_PERP] = div(k1, Rk0);  // :375, :377
    if (fields & (1u << RAYS_DIAG_N_IMAG)) {
      double n_imag = 0.;
      if (damp) {  // :381-405.  Always the cold derivatives: the reference tests ray_dispersion_model, not ray_deriv_name
        const double nvec[3] = {div(kvec[0], Rk0), div(kvec[1], Rk0), div(kvec[2], Rk0)};
        double dddx[3], dddk[3], dddw;
        deriv_cold<NS>(P, eq, nvec, dddx, dddk, dddw);  // :388
        if (fabs(dddw) > 2.2250738585072014e-308) {     // :395 tiny(dddw)
          const Recip Rw = make_recip(dddw);
          const double vg[3] = {div(-dddk[0], Rw), div(-dddk[1], Rw), div(-dddk[2], Rw)};  // :396
          const double ki = damp_fund_ech<NS>(P, eq, kvec, vg);                             // :402
          n_imag = div(ki, Rk0);                                                            // :403
        } else {
          bad = true;  // the reference stops here (:398-399)
        }
      }
      out[RAYS_DIAG_N_IMAG] = n_imag;
    }
    if (fields & kDiagXi) {  // :408-415
      double xi0 = 0., xi1 = 0., xi2 = 0.;
      if (eq.ts0 > 0. && fabs(k3) > 0.) {
        const double vth = fsqrt(fdiv(2. * eq.ts0, P.ms[0]));
        const Recip Rd = make_recip(k3 * vth);
        xi0 = div(P.omgrf, Rd);
        xi1 = div(P.omgrf + eq.omgc0, Rd);
        xi2 = div(P.omgrf + 2. * eq.omgc0, Rd);
      }
      out[RAYS_DIAG_XI_0] = xi0;
      out[RAYS_DIAG_XI_1] = xi1;
      out[RAYS_DIAG_XI_2] = xi2;
    }
  }
  return bad;
}

// Arguments of the kernel (rays_diag.hip).  Two layouts of the trajectory and output arrays:
//   padded (offsets == nullptr): ray_vec[nray][npt][nv], residual[nray][npt], out[k][nray][npt] -- what
//     rays_hip_trace_device leaves; slots past npoints(iray) of out are written as +0.0 by the kernel;
//   packed (offsets[iray] = points of the rays before iray): ray_vec[total][nv], residual[total], out[k][total] -- the
//     host-pointer form, so that only recorded points cross PCIe; npt is then the largest npoints of the block.
struct DiagArgs {
  int nray, npt, nv;
  unsigned fields;
  const double* ray_vec;
  const double* residual;
  const int* npoints;
  const long long* offsets;
  long long out_stride;  // doubles between two selected fields of out: nray * npt | total
  double* out;
  int* first_bad;        // [nray], zeroed by the launcher; may be null
};

// ---- the packed form (rays_hip_ray_diagnostics_packed_device): work follows the recorded points ----------------------
// offsets[0 .. nray] is the exclusive prefix sum of the rays' point counts (rays_hip_point_offsets_device), so that
// flat index j of the packed arrays is point j - offsets[r] of the ray r with offsets[r] <= j < offsets[r + 1]; rays
// without points share their offset with the next ray and are never the answer.

// The ray of flat index j, 0 <= j < offsets[nray], by bisection: the largest r in [0, nray) with offsets[r] <= j.
// (numpy: searchsorted(offsets, j, side = "right") - 1.)  An index outside that range gives 0 or nray - 1.
RAYS_DEV int diag_locate(const long long* offsets, int nray, long long j) {
  int lo = 0, hi = nray;  // offsets[lo] <= j (or lo == 0), offsets[hi] > j (or hi == nray)
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// The same answer for j >= offsets[r0], found from r0 outwards: doubling strides until a ray starts beyond j, then
// bisection between the last two probes -- 1 probe where j lies in ray r0, O(log(r - r0)) otherwise, so that a wave
// whose first point lies in r0 settles its 64 lanes in a few probes however many rays of 0 or 1 points it spans.
RAYS_DEV int diag_locate_from(const long long* offsets, int nray, int r0, long long j) {
  int lo = r0, hi = r0 + 1;
  for (int step = 1; hi < nray && offsets[hi] <= j; step += step) {
    lo = hi;
    hi = nray - hi > step ? hi + step : nray;
  }
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// Arguments of the packed kernel.  out[k][out_stride]; flat index j of field k lands at out[k * out_stride + j]; no
// store at or beyond min(offsets[nray], capacity) of any field, capacity = min(out_stride, nray * npt).
struct DiagPackedArgs {
  int nray, npt, nv;     // npt = nstep_max + 1: the row count per ray of the padded input
  int in_packed;         // ray_vec[total][nv], residual[total] (else the padded arrays of the trace)
  unsigned fields;
  const double* ray_vec;
  const double* residual;
  const int* npoints;
  const long long* offsets;  // [nray + 1]
  long long out_stride, capacity;
  double* out;
  int* first_bad;        // [nray], zeroed by the launcher; may be null
};

}  // namespace rays
