// TEST INFRASTRUCTURE ONLY: the device right-hand side (rays_amd/csrc/rays_device_arith.inc: equilibrium, deriv_cold,
// deriv_num, rhs_eval = eqn_ray + check_save, rk4_step_as_reference) compiled for the host and evaluated at given
// states, in the configuration's own shape (its derivative model, its nv: damping and gradient rows included).  Used by
// tests/test_cpu_rhs_states.py against the reference's records of the same states.
#include <hip/hip_runtime.h>
#include <vector>
RAYS_EMUL_DEFINE_GLOBALS
#include "../../rays_amd/csrc/rays_trace.hpp"   // (rays_device.hpp + TraceArgs, which emul_common.hpp's helpers name)

// make_dev_params is host code in rays_capi.hip; reuse its text through a small include shim
#include "emul_dev_params.inc"
#include "emul_common.hpp"

// the shapes the state fixture's cases have: two species, nv = 7 | 8 | 12
struct ProbeShapes {
  template <int EQ, int DERIV, int NS, int NV>
  static constexpr bool lane = NS == 2 && (NV == 7 || NV == 8 || NV == 12) && (EQ & rays::kEqMultiSpec) == 0;
  template <class S> static constexpr bool wave = false;
};

// The eq_point record in the layout of oracle/rays_oracle.c: rays_oracle_probe.  EqPoint keeps the electron
// temperature only: the ts / gradts entries of the other species are written as 0 and not compared.
template <int NS>
static void put_eq(const rays::EqPoint<NS>& eq, double* o) {
  for (int i = 0; i < 3; i++) *o++ = eq.bvec[i];
  *o++ = eq.bmag;
  for (int i = 0; i < 3; i++) *o++ = eq.gradbmag[i];
  for (int i = 0; i < 3; i++) *o++ = eq.bunit[i];
  for (int j = 0; j < 3; j++)
    for (int i = 0; i < 3; i++) *o++ = eq.gradbunit[i][j];
  for (int j = 0; j < 3; j++)
    for (int i = 0; i < 3; i++) *o++ = eq.gbt[i][j];
  for (int is = 0; is < NS; is++) {
    *o++ = eq.ns[is];
    for (int i = 0; i < 3; i++) *o++ = eq.gradns[is][i];
    *o++ = is == 0 ? eq.ts0 : 0.;
    for (int i = 0; i < 3; i++) *o++ = is == 0 ? eq.gradts0[i] : 0.;
    *o++ = eq.omgc[is];
    *o++ = eq.omgp2[is];
    *o++ = eq.alpha[is];
    *o++ = eq.gamma[is];
  }
}

template <int EQ, int DERIV, int NS, int NV>
static int probe_states(const rays::DevParams& P, int n, const double* vin, double* eq_out, double* cold7, double* num7,
                        double* dvds, double* resid, int32_t* codes) {
  using namespace rays;
  const int neq = 28 + 12 * NS;
  for (int s = 0; s < n; s++) {
    double v[NV];
    for (int i = 0; i < NV; i++) v[i] = vin[(size_t)s * NV + i];
    const double rvec[3] = {v[0], v[1], v[2]}, kvec[3] = {v[3], v[4], v[5]};
    EqPoint<NS> eq;
    equilibrium<EQ, NS>(P, const_recip(P.omgrf, P.inv_omgrf), const_recip(P.omgrf2, P.inv_omgrf2), rvec, eq, true);
    codes[4 * s] = eq.err;
    put_eq<NS>(eq, eq_out + (size_t)s * neq);
    const double nvec[3] = {kvec[0] / P.k0, kvec[1] / P.k0, kvec[2] / P.k0};
    double* c = cold7 + 7 * (size_t)s;
    double* m = num7 + 7 * (size_t)s;
    deriv_cold<NS>(P, eq, nvec, c, c + 3, c[6]);
    deriv_num<EQ, NS>(P, eq, rvec, kvec, m, m + 3, m[6]);
    double f[NV], r;
    int cs_flag, code;
    bool cs_stop;
    rhs_eval<EQ, NS, DERIV, NV>(P, v, true, r, cs_flag, cs_stop, code, f);
    for (int i = 0; i < NV; i++) dvds[(size_t)s * NV + i] = f[i];
    resid[s] = r;
    codes[4 * s + 1] = code;
    codes[4 * s + 2] = cs_flag;
    codes[4 * s + 3] = cs_stop ? 1 : 0;
  }
  return 0;
}

// One step as trace_rays has it: RK4_ode, and check_save at the new state if no stage refused.
// v1 = the new state, or v untouched after a refused stage; codes[s] = {stage stop code, check_save flag, stop_ode}
template <int EQ, int DERIV, int NS, int NV>
static int step_states(const rays::DevParams& P, int n, const double* vin, const double* s0, double* v1, double* resid,
                       int32_t* codes) {
  using namespace rays;
  for (int s = 0; s < n; s++) {
    double v[NV], w[NV], f[NV], r = 0.;
    for (int i = 0; i < NV; i++) v[i] = vin[(size_t)s * NV + i];
    const double sa = s0 ? s0[s] : 0., sout = sa + P.ds;
    int cs_flag = 0, code = 0;
    bool cs_stop = false;
    const int stop = rk4_step_as_reference<EQ, NS, DERIV, NV>(P, v, sout - sa, w);
    if (!stop) rhs_eval<EQ, NS, DERIV, NV>(P, w, true, r, cs_flag, cs_stop, code, f);
    for (int i = 0; i < NV; i++) v1[(size_t)s * NV + i] = stop ? v[i] : w[i];
    resid[s] = r;
    codes[3 * s] = stop;
    codes[3 * s + 1] = cs_flag;
    codes[3 * s + 2] = cs_stop ? 1 : 0;
  }
  return 0;
}

// v[n][nv]; eq_out[n][28 + 12 ns], cold7[n][7], num7[n][7], dvds[n][nv], resid[n], codes[n][4] (equilibrium err, eqn_ray
// stop code, check_save flag, check_save stop_ode).  1 | 4: a shape outside the fixture's; 2 | 3: a table is missing
extern "C" int rays_emul_probe(const rays_params_t* p, int n, const double* v, double* eq_out, double* cold7,
                               double* num7, double* dvds, double* resid, int32_t* codes) {
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  const rays::DevParams& D_ = D;
  return emul_lane_dispatch<ProbeShapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return probe_states<S::EQ, S::DERIV, S::NS, S::NV>(D_, n, v, eq_out, cold7, num7, dvds, resid, codes);
  });
}

extern "C" int rays_emul_rk4_step(const rays_params_t* p, int n, const double* v, const double* s0, double* v1,
                                  double* resid, int32_t* codes) {
  if (p->ode_solver != RAYS_ODE_RK4) return 100;
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  const rays::DevParams& D_ = D;
  return emul_lane_dispatch<ProbeShapes>(p, [&](auto sh) {
    typedef decltype(sh) S;
    return step_states<S::EQ, S::DERIV, S::NS, S::NV>(D_, n, v, s0, v1, resid, codes);
  });
}
