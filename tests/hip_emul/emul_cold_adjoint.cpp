// The tolerance flavour's adjoint form of dD/dalpha_s, dD/dgamma_s (rays_amd/csrc/rays_cold_adjoint.inc: sums and
// products only) compiled for the host as it stands, for tests/test_cpu_cold_adjoint.py.
#define RAYS_DEV static inline
namespace rays {
#include "../../rays_amd/csrc/rays_cold_adjoint.inc"
}

// in: p, t, u, q, n1**2, n3**2 and the five per-species tables [ns]; out: ddda[ns], dddg[ns]
extern "C" int rays_emul_cold_adjoint(int ns, double p, double t, double u, double q, double n1_2, double n3_2,
                                      const double* duda, const double* dqda, const double* dtdg, const double* dudg,
                                      const double* dqdg, double* ddda, double* dddg) {
  switch (ns) {
#define RAYS_CASE(NS) \
  case NS: rays::cold_adjoint<NS>(p, t, u, q, n1_2, n3_2, duda, dqda, dtdg, dudg, dqdg, ddda, dddg); return 0;
    RAYS_CASE(1) RAYS_CASE(2) RAYS_CASE(3) RAYS_CASE(4) RAYS_CASE(5) RAYS_CASE(6)
#undef RAYS_CASE
  }
  return 1;
}
