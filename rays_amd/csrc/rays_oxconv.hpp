// rays_oxconv.hpp -- O-X mode conversion analysis on the device: the post-processors' analyze_OX_conv applied to the
// trajectories where the trace left them, one record per ray (rays_hip.h: rays_ox_result_t).
//
// Reference path restated here (citations are RAYS_project/post_process_lib/OX_conv_analysis_m.f90:<line>):
//   analyze_OX_conv     :91-198    the ray loop and what a ray's record holds
//   find_x_max_ray      :202-252   the first point whose alpha(0) is smaller than its predecessor's
//   find_x_cutoff_ray   :256-311   steepest ascent from there to |alpha - 1| <= 1e-4, at most 10 iterations
//   OX_conv_coeff       :315-407   Mjolhus' coefficient at the cutoff point
// with equilibrium (equilibrium_m.f90:135-272) = the device function of rays_device_arith.inc, in the exact arithmetic
// (this header is never compiled with RAYS_TOL_FLAVOUR).
//
// What the compiler of the reference build (flang, -O2 -ffp-contract=off) makes of the intrinsics, read off its output
// and held by tests/test_cpu_ox_conv.py against a program of ours:
//   norm2        a call of the runtime's Norm2 (no inline sum of squares): a running maximum m and the sum s of the
//                squares of the OTHER elements over m, rescaled when the maximum changes, result m * sqrt(1 + s)
//                (ox_norm2_add).  The runtime's compensated summation adds nothing for three elements or fewer.
//   minval       of a two-element constructor (/a, b/): inline, a unless b < a or (a is NaN and b is not)
//   dot_product  inline, ((0 + a1*b1) + a2*b2) + a3*b3
//   x/norm2(x)   one IEEE division per element
//
// Bit-identical to the reference: everything up to and including cos_theta = dot(xc, bunit), gamma, L, n_vertical, ny_c,
// nz_c, the three nvec*_c, x_cut and the iteration count -- products, sums, quotients and square roots.  conv_coeff
// passes through acos, sin and cos, which this project has not restated for the device: ox_conv_value is a template
// over the five library functions, the kernel instantiates it with the device library's acos / sin / cos and
// rays_libm.hpp's exp / pow (a tolerance), the host form of the C ABI with the host's libm (bit-identical).
//
// Defined where the reference is not: the module never looks at equib_err.  A ray one of whose NEEDED points the
// equilibrium refuses -- a scanned point up to and including the one that shows the first decrease (every point of a
// ray without a decrease), an ascent iterate, the cutoff point -- gets status RAYS_OX_EQ_REFUSED and zeros.  Points
// behind the first decrease are not the reference's business: what the scan evaluates there (the rest of the chunk of
// 64) reaches no output.
#pragma once

#include "rays_device.hpp"

namespace rays {

constexpr double kOxPi = (double)3.1415926535897932385f;  // constants_m.f90:39: a default-real literal
constexpr double kOxThreshold = (double)0.0001f;          // :32 conversion_threshold, a default-real literal
constexpr double kOxAlphaTol = 1.0 / 10000.0;             // :274 one/10.0_rkind**4
constexpr int kOxMaxIterations = 10;                      // :275

// ---- the intrinsics as the reference build evaluates them ------------------------------------------------------------
RAYS_DEV void ox_norm2_add(double x, double& mx, double& s) {
  const double a = fabs(x);
  if (mx == 0.) {  // (no maximum yet, or only zeros so far; false for a NaN maximum)
    mx = a;
  } else if (a > mx) {
    const double t = fdiv(mx, a), t2 = t * t;
    s = s * t2;  // the sum so far, over the new maximum
    s = s + t2;  // the old maximum's own term
    mx = a;
  } else {
    const double t = fdiv(a, mx);
    s = s + t * t;
  }
}
RAYS_DEV double ox_norm2_3(const double v[3]) {
  double mx = 0., s = 0.;
  ox_norm2_add(v[0], mx, s);
  ox_norm2_add(v[1], mx, s);
  ox_norm2_add(v[2], mx, s);
  return mx * fsqrt(1. + s);
}
RAYS_DEV double ox_norm2_2(double a, double b) {
  double mx = 0., s = 0.;
  ox_norm2_add(a, mx, s);
  ox_norm2_add(b, mx, s);
  return mx * fsqrt(1. + s);
}
RAYS_DEV double ox_minval2(double a, double b) {
  double m = a;
  if (b < a || (a != a && b == b)) m = b;
  return m;
}
RAYS_DEV double ox_dot(const double a[3], const double b[3]) { return ((0. + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]; }
// vectors3_m.f90:64-71 cross_product_D
RAYS_DEV void ox_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- one ray's record (rays_hip.h: rays_ox_result_t, one element of every array) -----------------------------------
struct OxRecord {
  int status, step_number, iterations;
  double alpha_max, x_max[3], k_max[3], x_cut[3], conv_coeff, nvecx_c[3], nvecy_c[3], nvecz_c[3], aux[RAYS_OX_NAUX];
};
RAYS_DEV void ox_clear(OxRecord& R, int status) {
  R.status = status;
  R.step_number = R.iterations = 0;
  R.alpha_max = R.conv_coeff = 0.;
#pragma unroll
  for (int i = 0; i < 3; i++) R.x_max[i] = R.k_max[i] = R.x_cut[i] = R.nvecx_c[i] = R.nvecy_c[i] = R.nvecz_c[i] = 0.;
#pragma unroll
  for (int i = 0; i < RAYS_OX_NAUX; i++) R.aux[i] = 0.;
}

// alpha(0) at a point (:232-234, :237-239); refused: equilibrium left an error flag there
template <int EQ, int NS>
RAYS_DEV double ox_alpha(const DevParams& P, const double x[3], bool& refused) {
  EqPoint<NS> eq;
  equilibrium<EQ, NS>(P, const_recip(P.omgrf, P.inv_omgrf), const_recip(P.omgrf2, P.inv_omgrf2), x, eq, true);
  refused = eq.err != 0;
  return eq.alpha[0];
}

// conv_coeff from its five ingredients (:387-394).  M supplies acos_, sin_, cos_, exp_, pow_.
template <class M>
__host__ __device__ inline double ox_conv_value(double cos_theta, double gamma, double L, double ny_c, double nz_c,
                                                double k0) {
  const double theta = M::acos_(cos_theta);  // :363
  const double st = M::sin_(theta), ct = M::cos_(theta);
  const double n_crit = st * sqrt(gamma / (1. + gamma));                     // :387
  const double den = (1. + gamma) * (ct * ct) + (st * st) / 2.;              // :389-390, :392
  const double F = 0.5 * (1. + gamma) * sqrt(gamma) / M::pow_(den, 1.5);     // :389-390
  const double G = 0.5 * sqrt(gamma) / sqrt(den);                            // :392
  const double dz = fabs(nz_c) - n_crit, ay = fabs(ny_c);
  return M::exp_(-(kOxPi * k0 * L * (F * (dz * dz) + G * (ay * ay))));      // :394
}
struct OxDeviceMath {  // the device library's trigonometry, this project's exp and pow
  static RAYS_DEV double acos_(double x) { return ::acos(x); }
  static RAYS_DEV double sin_(double x) { return ::sin(x); }
  static RAYS_DEV double cos_(double x) { return ::cos(x); }
  static RAYS_DEV double exp_(double x) { return libm::exp(x); }
  static RAYS_DEV double pow_(double x, double y) { return libm::pow(x, y); }
};

// OX_conv_coeff (:357-394) on the equilibrium record of the cutoff point: the unit vectors, the five ingredients (aux),
// the three index vectors and the coefficient
template <int NS>
RAYS_DEV void ox_coeff(const DevParams& P, const EqPoint<NS>& eq, OxRecord& R) {
  const double g[3] = {eq.gradns[0][0], eq.gradns[0][1], eq.gradns[0][2]};
  const double gn = ox_norm2_3(g);
  double xc[3], yc[3], zc[3], v[3];
#pragma unroll
  for (int i = 0; i < 3; i++) xc[i] = fdiv(g[i], gn);  // :359
  ox_cross(eq.bunit, xc, v);                           // :360
  const double vn = ox_norm2_3(v);
#pragma unroll
  for (int i = 0; i < 3; i++) yc[i] = fdiv(v[i], vn);  // :361
  ox_cross(xc, yc, zc);                                // :362
  const double cos_theta = ox_dot(xc, eq.bunit);       // :363 (the argument of acos)
  const double gamma = fabs(eq.gamma[0]);              // :364
  const double L = fdiv(eq.ns[0], gn);                 // :365
  const double n_vertical = fdiv(ox_dot(R.k_max, xc), P.k0);  // :379
  const double nz_c = fdiv(ox_dot(R.k_max, zc), P.k0);        // :380
  const double ny_c = fdiv(ox_dot(R.k_max, yc), P.k0);        // :381
#pragma unroll
  for (int i = 0; i < 3; i++) {  // :383-385
    R.nvecx_c[i] = n_vertical * xc[i];
    R.nvecy_c[i] = ny_c * yc[i];
    R.nvecz_c[i] = nz_c * zc[i];
  }
  R.aux[RAYS_OX_AUX_COS_THETA] = cos_theta;
  R.aux[RAYS_OX_AUX_GAMMA] = gamma;
  R.aux[RAYS_OX_AUX_L] = L;
  R.aux[RAYS_OX_AUX_NY_C] = ny_c;
  R.aux[RAYS_OX_AUX_NZ_C] = nz_c;
  R.conv_coeff = ox_conv_value<OxDeviceMath>(cos_theta, gamma, L, ny_c, nz_c, P.k0);
  if (R.conv_coeff > kOxThreshold) R.status |= RAYS_OX_CONVERTED;  // :154
}

// find_x_cutoff_ray (:279-308) from R.x_max, then OX_conv_coeff at the point it ends on; R.status holds FOUND_MAX on
// entry.  One call site of the equilibrium: the evaluation before the reference's loop and the one of its first
// iteration are at the same point, and the evaluation of OX_conv_coeff is the loop's next one.
//   iteration k evaluates at x(k-1), steps to x(k), and iteration k + 1 first tests the alpha of x(k-1): the reference
//   leaves with x_cut = x(k), one step past the point that met the tolerance (iteration 2 repeats iteration 1's test).
template <int EQ, int NS>
RAYS_DEV void ox_cutoff(const DevParams& P, OxRecord& R) {
  double x[3] = {R.x_max[0], R.x_max[1], R.x_max[2]};
  double alpha_temp = 0.;
  bool found = false, at_cutoff = false;
  int iteration = 1;
  for (;;) {
    EqPoint<NS> eq;
    equilibrium<EQ, NS>(P, const_recip(P.omgrf, P.inv_omgrf), const_recip(P.omgrf2, P.inv_omgrf2), x, eq, true);
    if (eq.err != 0) {
      ox_clear(R, RAYS_OX_EQ_REFUSED);
      return;
    }
    if (iteration == 1) {
      R.alpha_max = eq.alpha[0];  // :242: the alpha the scan saw at this point
      found = fabs(eq.alpha[0] - 1.) <= kOxAlphaTol;  // :289, first iteration
      at_cutoff = found;
    }
    if (at_cutoff) {  // x is x_cutoff_ray
      R.status |= RAYS_OX_FOUND_CUTOFF;
      R.iterations = iteration;
#pragma unroll
      for (int i = 0; i < 3; i++) R.x_cut[i] = x[i];
      ox_coeff<NS>(P, eq, R);
      return;
    }
    alpha_temp = eq.alpha[0];                                                      // :295
    const double g[3] = {eq.gradns[0][0], eq.gradns[0][1], eq.gradns[0][2]};
    const double gn = ox_norm2_3(g);
    const double mod_grad_alpha = gn * fdiv(alpha_temp, eq.ns[0]);                 // :296
    const double r = ox_norm2_2(x[0], x[1]);                                       // :298
    const double delta = fdiv(1. - eq.alpha[0], mod_grad_alpha);                   // :299
    const double step = ox_minval2(delta, 0.25 * r);                               // :301
#pragma unroll
    for (int i = 0; i < 3; i++) x[i] = x[i] + fdiv(g[i], gn) * step;               // :297, :301-302
    iteration++;
    if (iteration > kOxMaxIterations) break;                                       // :287: iteration = 11 after the loop
    if (fabs(alpha_temp - 1.) <= kOxAlphaTol) at_cutoff = true;                    // :289
  }
  R.iterations = iteration;  // not found: x_cut and everything behind it stay zero (:143)
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
// Input layouts (rays_hip.h): padded ray_vec[nray][npt][nv] as the trace leaves it, or packed ray_vec[total][nv] with
// offsets[0 .. nray].  npoints is clamped to the array (and, packed, to the ray's own run) whatever it holds.
struct OxArgs {
  int nray, npt, nv, packed;
  const double* ray_vec;
  const int* npoints;
  const long long* offsets;  // packed only
  int* scan;                 // [nray][2]: RAYS_OX_FOUND_MAX | RAYS_OX_EQ_REFUSED | 0, step_number
  rays_ox_result_t out;      // device pointers, each may be null
};

constexpr int kOxWave = 64;
constexpr int kOxScanBlock = 256;   // four independent waves, one ray each
constexpr int kOxAscentBlock = 64;  // one wave of 64 rays: small fans still spread over the CUs

RAYS_DEV const double* ox_ray_rows(const OxArgs& A, int iray, int& np) {
  np = A.npoints[iray];
  np = np < A.npt ? np : A.npt;
  long long first = (long long)iray * A.npt;
  if (A.packed) {
    first = A.offsets[iray];
    const long long run = A.offsets[iray + 1] - first;
    if (np > run) np = (int)run;
  }
  return A.ray_vec + first * A.nv;
}

// find_x_max_ray: one wave per ray, one lane per point, chunks of 64 consecutive points.  Each lane evaluates alpha(0)
// at its point, takes its predecessor's by lane shuffle (lane 0: the previous chunk's lane 63, carried wave-uniform),
// and the first set bit of the ballot of `alpha < predecessor's` is the reference's first decrease.  The wave leaves at
// the chunk that holds it: launched arithmetic follows step_number, not nstep_max.
// A lane reads the three doubles of its own row straight from global memory.  The rows of a chunk are one contiguous
// span of 64 * nv doubles; with rows of 56 .. 128 bytes (nv = 7 .. 16) the 64 strided 24-byte reads touch every
// 128-byte line of that span once, which is what staging the span through LDS would fetch too -- but staging moves all
// nv columns to use three of them, nothing is reused between lanes, it needs a block-wide barrier in a kernel whose
// waves leave at different chunks, and the three loads are issued once in front of a few hundred dependent FP64
// operations (the equilibrium), so their latency is the only cost and it is paid once per chunk either way.
template <int EQ, int NS>
__global__ void __launch_bounds__(kOxScanBlock) ox_scan_kernel(const DevParams P, const OxArgs A) {
  const int lane = threadIdx.x & (kOxWave - 1), wave = threadIdx.x / kOxWave;
  const long long w = (long long)blockIdx.x * (kOxScanBlock / kOxWave) + wave;
  if (w >= A.nray) return;  // (the whole wave)
  const int iray = (int)w;
  int np;
  const double* rv = ox_ray_rows(A, iray, np);
  double carry = 0.;        // alpha of the previous chunk's last point
  bool carry_refused = false, decided = false;
  int flags = 0, step = 0;
  for (int p0 = 0; p0 < np; p0 += kOxWave) {
    const int ip = p0 + lane;
    const bool live = ip < np;
    double alpha = 0.;
    bool refused = false;
    if (live) {
      const double* row = rv + (long long)ip * A.nv;
      const double x[3] = {row[0], row[1], row[2]};
      alpha = ox_alpha<EQ, NS>(P, x, refused);
    }
    double before = __shfl(alpha, lane - 1);
    if (lane == 0) before = carry;
    const bool lower = live && ip > 0 && alpha < before;  // :240
    const unsigned long long m = __ballot(lower), mr = __ballot(refused);
    if (m) {
      const int f = __builtin_ctzll(m);  // the first such point: ip = p0 + f, 1-based index p0 + f + 1
      const unsigned long long upto = f == kOxWave - 1 ? ~0ull : (2ull << f) - 1ull;
      if (carry_refused || (mr & upto)) {
        flags = RAYS_OX_EQ_REFUSED;
      } else {
        flags = RAYS_OX_FOUND_MAX;
        step = p0 + f;  // :243 step_number = i - 1
      }
      decided = true;
      break;
    }
    carry = __shfl(alpha, 63);
    carry_refused = carry_refused || mr != 0;
  }
  if (!decided && carry_refused) flags = RAYS_OX_EQ_REFUSED;  // no decrease: every point was needed
  if (lane == 0) {
    A.scan[2 * (long long)iray] = flags;
    A.scan[2 * (long long)iray + 1] = step;
  }
}

RAYS_DEV void ox_store3(double* dst, long long iray, const double v[3]) {
  if (dst) {
    dst[3 * iray] = v[0];
    dst[3 * iray + 1] = v[1];
    dst[3 * iray + 2] = v[2];
  }
}

// find_x_cutoff_ray + OX_conv_coeff: one lane per ray (up to twelve evaluations of the equilibrium in a row; a wave
// per ray would idle 63 lanes through them).  A ray without a maximum writes its zeros (:126-129) and leaves.
template <int EQ, int NS>
__global__ void __launch_bounds__(kOxAscentBlock) ox_ascent_kernel(const DevParams P, const OxArgs A) {
  const long long iray = (long long)blockIdx.x * kOxAscentBlock + threadIdx.x;
  if (iray >= A.nray) return;
  OxRecord R;
  ox_clear(R, A.scan[2 * iray]);
  if (R.status & RAYS_OX_FOUND_MAX) {
    int np;
    const double* rv = ox_ray_rows(A, (int)iray, np);
    R.step_number = A.scan[2 * iray + 1];
    const double* row = rv + (long long)(R.step_number - 1) * A.nv;  // 1 <= step_number < np
#pragma unroll
    for (int i = 0; i < 3; i++) {  // :244-245
      R.x_max[i] = row[i];
      R.k_max[i] = row[3 + i];
    }
    ox_cutoff<EQ, NS>(P, R);
  }
  const rays_ox_result_t& O = A.out;
  if (O.status) O.status[iray] = R.status;
  if (O.step_number) O.step_number[iray] = R.step_number;
  if (O.iterations) O.iterations[iray] = R.iterations;
  if (O.alpha_max) O.alpha_max[iray] = R.alpha_max;
  if (O.conv_coeff) O.conv_coeff[iray] = R.conv_coeff;
  ox_store3(O.x_max, iray, R.x_max);
  ox_store3(O.k_max, iray, R.k_max);
  ox_store3(O.x_cut, iray, R.x_cut);
  ox_store3(O.nvecx_c, iray, R.nvecx_c);
  ox_store3(O.nvecy_c, iray, R.nvecy_c);
  ox_store3(O.nvecz_c, iray, R.nvecz_c);
  if (O.aux) {
#pragma unroll
    for (int i = 0; i < RAYS_OX_NAUX; i++) O.aux[RAYS_OX_NAUX * iray + i] = R.aux[i];
  }
}

}  // namespace rays
