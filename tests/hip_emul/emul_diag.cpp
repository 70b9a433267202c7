// TEST INFRASTRUCTURE ONLY: the per-point ray diagnostics (rays_amd/csrc/rays_diag.hpp: diag_point) compiled for the
// host, applied point by point in the layout of rays_hip_ray_diagnostics.  Used by tests/test_cpu_ray_diagnostics.py.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
RAYS_EMUL_DEFINE_GLOBALS
#include "../../rays_amd/csrc/rays_diag.hpp"

// make_dev_params is host code in rays_capi.hip; reuse its text through a small include shim
#include "emul_dev_params.inc"

static std::vector<double> g_zfun;
static int g_zf_nx = 0;
static double g_zf_xmin = 0., g_zf_xmax = 0.;
extern "C" int rays_emul_diag_set_zfun_table(const double* f, int nx, double x_min, double x_max) {
  g_zfun.assign(f, f + 4 * (size_t)nx);
  g_zf_nx = nx; g_zf_xmin = x_min; g_zf_xmax = x_max;
  return 0;
}

static std::vector<double> g_axi[11];
static int g_axi_n[6];
static int g_axi_lin = 0;
static double g_axi_dR = 0., g_axi_dZ = 0.;
extern "C" int rays_emul_diag_set_axisym_tables(const rays_axisym_tables_t* t, int lin, double dR, double dZ) {
  g_axi_lin = lin; g_axi_dR = dR; g_axi_dZ = dZ;
  const double* src[11] = {t->r_grid, t->z_grid, t->psi_fspl, t->rb_grid, t->rb_fspl, t->ne_grid, t->ne_fspl,
                           t->te_grid, t->te_fspl, t->ti_grid, t->ti_fspl};
  const size_t len[11] = {(size_t)t->nr, (size_t)t->nz, (size_t)(lin ? 1 : 16) * t->nr * t->nz, lin ? (size_t)0 : (size_t)t->n_rb,
                          (size_t)(lin ? 1 : 4) * t->n_rb,
                          (size_t)t->n_ne, (size_t)4 * t->n_ne, (size_t)t->n_te, (size_t)4 * t->n_te,
                          (size_t)t->n_ti, (size_t)4 * t->n_ti};
  for (int k = 0; k < 11; k++) g_axi[k].assign(src[k] ? src[k] : nullptr, src[k] ? src[k] + len[k] : nullptr);
  g_axi_n[0] = t->nr; g_axi_n[1] = t->nz; g_axi_n[2] = t->n_rb; g_axi_n[3] = t->n_ne; g_axi_n[4] = t->n_te; g_axi_n[5] = t->n_ti;
  return 0;
}

template <int EQ, int NS>
static void run_points(const rays::DevParams& D, const rays_params_t* p, int nray, const double* ray_vec,
                       const double* residual, const int32_t* npoints, unsigned fields, double* out, int32_t* first_bad) {
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  for (int r = 0; r < nray; r++) {
    if (first_bad) first_bad[r] = 0;
    for (int is = 0; is < npoints[r]; is++) {
      double v[8] = {0.}, f[RAYS_DIAG_NFIELDS] = {0.};
      std::memcpy(v, ray_vec + ((size_t)r * npt + is) * nv, sizeof(double) * (nv < 8 ? nv : 8));
      const bool bad = rays::diag_point<EQ, NS>(D, v, residual[(size_t)r * npt + is], fields, f);
      if (bad && first_bad && first_bad[r] == 0) first_bad[r] = is + 1;
      int k = 0;
      for (int i = 0; i < RAYS_DIAG_NFIELDS; i++)
        if (fields & (1u << i)) out[((size_t)k++ * nray + r) * npt + is] = f[i];
    }
  }
}

template <int EQ>
static int run_ns(const rays::DevParams& D, const rays_params_t* p, int nray, const double* ray_vec, const double* residual,
                  const int32_t* npoints, unsigned fields, double* out, int32_t* first_bad) {
#define RAYS_EMUL_NS(NS) \
  case NS: run_points<EQ, NS>(D, p, nray, ray_vec, residual, npoints, fields, out, first_bad); return 0;
  switch (p->nspec + 1) {
    RAYS_EMUL_NS(1) RAYS_EMUL_NS(2) RAYS_EMUL_NS(3) RAYS_EMUL_NS(4) RAYS_EMUL_NS(5) RAYS_EMUL_NS(6)
  }
#undef RAYS_EMUL_NS
  return 4;
}

// The arguments and layouts of rays_hip_ray_diagnostics (include/rays_hip.h): out[k][nray][nstep_max+1], zero where no
// point was recorded.
extern "C" int rays_emul_ray_diagnostics(const rays_params_t* p, int nray, const double* ray_vec, const double* residual,
                                         const int32_t* npoints, unsigned fields, double* out, int32_t* first_bad) {
  if (fields == 0 || (fields & ~rays::kDiagAllFields)) return 1;
  int nsel = 0;
  for (unsigned x = fields; x; x &= x - 1) nsel++;
  std::memset(out, 0, sizeof(double) * (size_t)nsel * nray * ((size_t)p->nstep_max + 1));
  rays::DevParams D = make_dev_params(*p);
  if (p->damping_model) {
    if (g_zfun.empty()) return 2;
    D.zf_fspl = g_zfun.data(); D.zf_nx = g_zf_nx; D.zf_xmin = g_zf_xmin; D.zf_xmax = g_zf_xmax;
  }
  if (p->equilib_model == RAYS_EQ_AXISYM) {
    if (p->axisym.magnetics_model == RAYS_AXI_MAG_EQDSK_SPLINE && (g_axi[2].empty() || g_axi_lin)) return 3;
    if (p->axisym.magnetics_model == RAYS_AXI_MAG_EQDSK_LIN && (g_axi[2].empty() || !g_axi_lin)) return 3;
    D.a_lin_dR = g_axi_dR; D.a_lin_dZ = g_axi_dZ;
    D.a_nr = g_axi_n[0]; D.a_nz = g_axi_n[1]; D.a_n_rb = g_axi_n[2]; D.a_n_ne = g_axi_n[3]; D.a_n_te = g_axi_n[4]; D.a_n_ti = g_axi_n[5];
    D.a_r_grid = g_axi[0].data(); D.a_z_grid = g_axi[1].data(); D.a_psi_fspl = g_axi[2].data();
    D.a_rb_grid = g_axi[3].data(); D.a_rb_fspl = g_axi[4].data(); D.a_ne_grid = g_axi[5].data(); D.a_ne_fspl = g_axi[6].data();
    D.a_te_grid = g_axi[7].data(); D.a_te_fspl = g_axi[8].data(); D.a_ti_grid = g_axi[9].data(); D.a_ti_fspl = g_axi[10].data();
    set_spline_axes(D, D.a_r_grid, D.a_z_grid, D.a_rb_grid, D.a_ne_grid, D.a_te_grid, D.a_ti_grid);
  }
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0);
#define RAYS_EMUL_EQ(E) \
  case E: return run_ns<E>(D, p, nray, ray_vec, residual, npoints, fields, out, first_bad);
  switch (e) { RAYS_EMUL_EQ(0) RAYS_EMUL_EQ(1) RAYS_EMUL_EQ(2) RAYS_EMUL_EQ(4) RAYS_EMUL_EQ(5) RAYS_EMUL_EQ(6) }
#undef RAYS_EMUL_EQ
  return 4;
}
