// rays_cold_adjoint.inc -- dD/dalpha_s and dD/dgamma_s of the cold dispersion polynomial in adjoint form, for the
// tolerance flavour of deriv_cold (rays_device_arith.inc).  Sums and products only: no quotient, root or builtin, so
// tests/hip_emul/emul_cold_adjoint.cpp compiles this file for the host as it stands.
//
// deriv_cold.f90:104-112 and :152-154 write out, per species, the partial derivatives of ONE polynomial
//   D = t p n3^4 + (-2 p u + (t p + u) n1^2) n3^2 + p q - (q + p u) n1^2 + u n1^4
// in its intermediates p, t, u, q (:78-101).  With the partials of D in those four taken once per evaluation,
//   D_t = p m,   D_p = t m + q - u h,   D_u = n1^2 n3^2 + n1^4 - p h,   D_q = p - n1^2        (m = n3^4 + n1^2 n3^2,
//                                                                                               h = 2 n3^2 + n1^2)
// each species costs the chain rule alone (dp/dalpha_s = -1, dt/dalpha_s = 0, dp/dgamma_s = 0):
//   dD/dalpha_s = D_u du/dalpha_s + D_q dq/dalpha_s - D_p
//   dD/dgamma_s = D_t dt/dgamma_s + D_u du/dgamma_s + D_q dq/dgamma_s
// The same monomials as the expanded expressions, summed in another order: equal to rounding.
template <int NS>
RAYS_DEV void cold_adjoint(double p, double t, double u, double q, double n1_2, double n3_2, const double duda[NS],
                           const double dqda[NS], const double dtdg[NS], const double dudg[NS], const double dqdg[NS],
                           double ddda[NS], double dddg[NS]) {
  const double n3_4 = n3_2 * n3_2, n1_4 = n1_2 * n1_2;
  const double a1 = n1_2 * n3_2;
  const double m = n3_4 + a1;
  const double h = 2. * n3_2 + n1_2;
  const double D_t = p * m;
  const double D_p = t * m + q - u * h;
  const double D_u = a1 + n1_4 - p * h;
  const double D_q = p - n1_2;
#pragma unroll
  for (int is = 0; is < NS; is++) {
    ddda[is] = D_u * duda[is] + D_q * dqda[is] - D_p;
    dddg[is] = D_t * dtdg[is] + D_u * dudg[is] + D_q * dqdg[is];
  }
}
