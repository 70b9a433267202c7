// TEST INFRASTRUCTURE ONLY: the O-X conversion analysis (rays_amd/csrc/rays_oxconv.hpp) compiled for the host: the scan
// kernel on the host wave emulator (hip/hip_wave_emul.h: 64 lanes as fibers, __ballot / __shfl are rendezvous, the
// carried lane 63), the ascent kernel lane by lane, and the host finish of rays_hip_ox_conv (conv_coeff and CONVERTED
// once more with the host's libm, the compacted list).  Used by tests/test_cpu_ox_conv.py.
#define RAYS_EMUL_WAVE 1
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
RAYS_EMUL_DEFINE_GLOBALS
#include "../../rays_amd/csrc/rays_oxconv.hpp"

// make_dev_params is host code in rays_capi.hip; reuse its text through a small include shim
#include "emul_dev_params.inc"

static std::vector<double> g_axi[11];
static int g_axi_n[6];
static int g_axi_lin = 0;
static double g_axi_dR = 0., g_axi_dZ = 0.;
extern "C" int rays_emul_ox_set_axisym_tables(const rays_axisym_tables_t* t, int lin, double dR, double dZ) {
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
static void run_kernels(const rays::DevParams& D, const rays::OxArgs& A) {
  const int per_block = rays::kOxScanBlock / rays::kOxWave;
  blockDim.x = rays::kOxScanBlock;
  gridDim.x = (unsigned)((A.nray + per_block - 1) / per_block);
  for (unsigned b = 0; b < gridDim.x; b++) {
    blockIdx.x = b;
    for (int w = 0; w < per_block; w++)
      wave_emul::run_wave(64u * (unsigned)w, [&] { rays::ox_scan_kernel<EQ, NS>(D, A); }, threadIdx);
  }
  blockDim.x = rays::kOxAscentBlock;
  gridDim.x = (unsigned)((A.nray + rays::kOxAscentBlock - 1) / rays::kOxAscentBlock);
  for (unsigned b = 0; b < gridDim.x; b++) {
    blockIdx.x = b;
    for (unsigned t = 0; t < (unsigned)rays::kOxAscentBlock; t++) {
      threadIdx.x = t;
      rays::ox_ascent_kernel<EQ, NS>(D, A);
    }
  }
}

template <int EQ>
static int run_ns(const rays::DevParams& D, int ns, const rays::OxArgs& A) {
#define RAYS_EMUL_NS(NS) \
  case NS: run_kernels<EQ, NS>(D, A); return 0;
  switch (ns) { RAYS_EMUL_NS(1) RAYS_EMUL_NS(2) RAYS_EMUL_NS(3) RAYS_EMUL_NS(4) RAYS_EMUL_NS(5) RAYS_EMUL_NS(6) }
#undef RAYS_EMUL_NS
  return 4;
}

struct HostMath {  // as rays_oxconv.hip: OxHostMath
  static double acos_(double x) { return std::acos(x); }
  static double sin_(double x) { return std::sin(x); }
  static double cos_(double x) { return std::cos(x); }
  static double exp_(double x) { return std::exp(x); }
  static double pow_(double x, double y) { return std::pow(x, y); }
};

// The arguments of rays_hip_ox_conv_device with host pointers (in_layout, offsets as there).  host_finish != 0: what
// rays_hip_ox_conv does behind the kernels -- it needs out->status, out->conv_coeff and out->aux -- and the list.
extern "C" int rays_emul_ox_conv(const rays_params_t* p, int nray, int in_layout, const double* ray_vec,
                                 const int32_t* npoints, const long long* offsets, const rays_ox_result_t* out,
                                 int host_finish, int32_t* n_converted, int32_t* converted) {
  rays::DevParams D = make_dev_params(*p);
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
  std::vector<int> scan(2 * (size_t)(nray > 0 ? nray : 1), -7);
  rays::OxArgs A;
  A.nray = nray; A.npt = p->nstep_max + 1; A.nv = p->nv; A.packed = in_layout == RAYS_DIAG_IN_PACKED;
  A.ray_vec = ray_vec; A.npoints = npoints; A.offsets = offsets;
  A.scan = scan.data();
  A.out = *out;
  const int e = p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0);
  int rc = 4;
#define RAYS_EMUL_EQ(E) \
  case E: rc = run_ns<E>(D, p->nspec + 1, A); break;
  switch (e) { RAYS_EMUL_EQ(0) RAYS_EMUL_EQ(1) RAYS_EMUL_EQ(2) RAYS_EMUL_EQ(4) RAYS_EMUL_EQ(5) RAYS_EMUL_EQ(6) }
#undef RAYS_EMUL_EQ
  if (rc || !host_finish) return rc;
  if (!out->status || !out->conv_coeff || !out->aux) return 5;
  int32_t n = 0;
  for (int i = 0; i < nray; i++) {
    if (out->status[i] & RAYS_OX_FOUND_CUTOFF) {
      const double* a = out->aux + RAYS_OX_NAUX * (size_t)i;
      out->conv_coeff[i] = rays::ox_conv_value<HostMath>(a[RAYS_OX_AUX_COS_THETA], a[RAYS_OX_AUX_GAMMA], a[RAYS_OX_AUX_L],
                                                         a[RAYS_OX_AUX_NY_C], a[RAYS_OX_AUX_NZ_C], p->k0);
      out->status[i] &= ~RAYS_OX_CONVERTED;
      if (out->conv_coeff[i] > rays::kOxThreshold) out->status[i] |= RAYS_OX_CONVERTED;
    }
    if (out->status[i] & RAYS_OX_CONVERTED) {
      if (converted) converted[n] = i + 1;
      n++;
    }
  }
  if (n_converted) *n_converted = n;
  return 0;
}
