// TEST INFRASTRUCTURE ONLY: what every emulated build of the trace kernels shares (included by emul_trace.cpp, and
// through it by emul_group.cpp and the variant builds emul_summary.cpp, emul_window.cpp, emul_fused_deposition.cpp):
// the table store and its attach, the TraceArgs maker with the two small workspaces, and the shape lists with their
// dispatchers.  A variant build gives its flags in EQ, what to run for a shape, and a predicate where it takes fewer
// shapes than the list has; it copies none of this.
#pragma once
#include <vector>

// ---- the table store: the Z-function spline and the axisym_toroid tables, set once per library by the Python side ----
static std::vector<double> g_zfun;
static int g_zf_nx = 0;
static double g_zf_xmin = 0., g_zf_xmax = 0.;
extern "C" int rays_emul_set_zfun_table(const double* f, int nx, double x_min, double x_max) {
  g_zfun.assign(f, f + 4 * (size_t)nx);
  g_zf_nx = nx; g_zf_xmin = x_min; g_zf_xmax = x_max;
  return 0;
}

static std::vector<double> g_axi[11];
static int g_axi_n[6];
static int g_axi_lin = 0;
static double g_axi_dR = 0., g_axi_dZ = 0.;
extern "C" int rays_emul_set_axisym_tables(const rays_axisym_tables_t* t, int lin, double dR, double dZ) {
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

// what an entry attaches: the Z-function table (if the run damps), the axisym_toroid magnetics (psi, R Bphi), and with
// them the three profile tables.  Ray initialisation and the lane-group entry take no Z-function, the deposition
// post-processor the magnetics alone (its profile axes stay null).
enum { kTabZfun = 1, kTabMagnetics = 2, kTabProfiles = 4, kTabAxisym = kTabMagnetics | kTabProfiles, kTabAll = 7 };
// 0, or 2: no Z-function table, 3: axisym tables missing or of the other kind
static int emul_attach_tables(const rays_params_t* p, rays::DevParams& D, int what) {
  if ((what & kTabZfun) && p->damping_model) {
    if (g_zfun.empty()) return 2;
    D.zf_fspl = g_zfun.data(); D.zf_nx = g_zf_nx; D.zf_xmin = g_zf_xmin; D.zf_xmax = g_zf_xmax;
  }
  if (!(what & kTabMagnetics) || p->equilib_model != RAYS_EQ_AXISYM) return 0;
  if (p->axisym.magnetics_model == RAYS_AXI_MAG_EQDSK_SPLINE && (g_axi[2].empty() || g_axi_lin)) return 3;
  if (p->axisym.magnetics_model == RAYS_AXI_MAG_EQDSK_LIN && (g_axi[2].empty() || !g_axi_lin)) return 3;
  D.a_lin_dR = g_axi_dR; D.a_lin_dZ = g_axi_dZ;
  D.a_nr = g_axi_n[0]; D.a_nz = g_axi_n[1]; D.a_n_rb = g_axi_n[2];
  D.a_r_grid = g_axi[0].data(); D.a_z_grid = g_axi[1].data(); D.a_psi_fspl = g_axi[2].data();
  D.a_rb_grid = g_axi[3].data(); D.a_rb_fspl = g_axi[4].data();
  if (!(what & kTabProfiles)) {
    set_spline_axes(D, D.a_r_grid, D.a_z_grid, D.a_rb_grid, nullptr, nullptr, nullptr);
    return 0;
  }
  D.a_n_ne = g_axi_n[3]; D.a_n_te = g_axi_n[4]; D.a_n_ti = g_axi_n[5];
  D.a_ne_grid = g_axi[5].data(); D.a_ne_fspl = g_axi[6].data();
  D.a_te_grid = g_axi[7].data(); D.a_te_fspl = g_axi[8].data(); D.a_ti_grid = g_axi[9].data(); D.a_ti_fspl = g_axi[10].data();
  set_spline_axes(D, D.a_r_grid, D.a_z_grid, D.a_rb_grid, D.a_ne_grid, D.a_te_grid, D.a_ti_grid);
  return 0;
}

// ---- the launch's argument block ----
// the output arrays of a launch; null where the variant has none (summary-only: no ray_vec / residual)
struct EmulOut {
  double *ray_vec, *residual;
  int32_t *npoints, *stop_code;
  double *start_ray_vec, *end_ray_vec, *end_residuals, *max_residuals;
};
static rays::TraceArgs emul_trace_args(int nray, const double* rvec0, const double* rindex_vec0, const EmulOut& o,
                                       unsigned* counter) {
  rays::TraceArgs A = rays::TraceArgs();
  A.nray = nray; A.rvec0 = rvec0; A.rindex_vec0 = rindex_vec0; A.ray_vec = o.ray_vec;
  A.residual = o.residual; A.npoints = o.npoints; A.stop_code = o.stop_code; A.set_start_ray_vec(o.start_ray_vec);
  A.end_ray_vec = o.end_ray_vec; A.end_residuals = o.end_residuals; A.max_residuals = o.max_residuals; A.next_ray = counter;
  return A;
}
// one lane: the SG kernels' upper-tier workspace
static void emul_one_lane_far(rays::TraceArgs& A, std::vector<double>& far) {
  far.assign(512, 0.0);
  A.sg_far = far.data(); A.sg_far_lanes = 1;
}
// stride > 1: the "long rays first" hand-out order (rays_trace.hpp: take_rays) with that neighbourhood size
static void emul_sched(rays::TraceArgs& A, std::vector<unsigned>& sched, int stride) {
  if (stride <= 1) return;
  sched.assign(4 + (size_t)rays::sched_pilots((unsigned)A.nray, stride), 0u);
  A.sched = sched.data();
  A.sched_stride = stride;
}
// the kernel selection of rays_capi.hip: find_kernel (EQ = model | kEqUnitExp)
static int emul_eq(const rays_params_t* p) { return p->equilib_model | (unit_exponents(*p) ? rays::kEqUnitExp : 0); }

// ---- the one-lane shape ladder ----
// (EQ & 7, DERIV) in {0, 1, 2, 4, 5, 6} x {0, 1}, each with two species and nv = 7 | 8, and nv = 12 | 13
// (integrate_eq_gradients); the slab also with one, three and six species, Solovev with four (nv = 7); the
// multi_spec_damping kernels (EQ | kEqMultiSpec, DERIV 0, unit exponents): Solovev nv = 10, slab nv = 15.
template <int EQ_, int DERIV_, int NS_, int NV_>
struct Shape { static constexpr int EQ = EQ_, DERIV = DERIV_, NS = NS_, NV = NV_; };
// the predicate of a build that takes the whole ladder
struct AllShapes {
  template <int EQ, int DERIV, int NS, int NV> static constexpr bool lane = true;
  template <class S> static constexpr bool wave = true;
};
template <class Pred, int EQ, int DERIV, class F>
static int emul_lane_shape(int ns, int nv, F& f) {
#define RAYS_EMUL_SHAPE(N, V)                                                                  \
  if (ns == N && nv == V) {                                                                    \
    if constexpr (Pred::template lane<EQ, DERIV, N, V>) return f(Shape<EQ, DERIV, N, V>{});    \
    else return 4;                                                                             \
  }
  if constexpr ((EQ & rays::kEqMultiSpec) != 0) {
    if constexpr ((EQ & 3) == 1) { RAYS_EMUL_SHAPE(2, 10) }
    if constexpr ((EQ & 3) == 0) { RAYS_EMUL_SHAPE(2, 15) }
  } else {
    RAYS_EMUL_SHAPE(2, 7) RAYS_EMUL_SHAPE(2, 8) RAYS_EMUL_SHAPE(2, 12) RAYS_EMUL_SHAPE(2, 13)
    if constexpr ((EQ & 3) == 0) { RAYS_EMUL_SHAPE(1, 7) RAYS_EMUL_SHAPE(3, 7) RAYS_EMUL_SHAPE(6, 7) }
    if constexpr ((EQ & 3) == 1) { RAYS_EMUL_SHAPE(4, 7) }
  }
#undef RAYS_EMUL_SHAPE
  return 1;
}
// Hands p's shape to f as a type, f(Shape<EQ, DERIV, NS, NV>{}), if the ladder has it and Pred::lane<...> takes it.
// 4: not built (no such (EQ, DERIV), or the predicate leaves the shape out), 1: (ns, nv) is not on the ladder.
template <class Pred, class F>
static int emul_lane_dispatch(const rays_params_t* p, F f) {
  const int e = emul_eq(p), d = p->ray_deriv, ns = p->nspec + 1, nv = p->nv;
  if (p->multi_spec_damping) {
    if (e == 5 && d == 0) return emul_lane_shape<Pred, 5 | rays::kEqMultiSpec, 0>(ns, nv, f);
    if (e == 4 && d == 0) return emul_lane_shape<Pred, 4 | rays::kEqMultiSpec, 0>(ns, nv, f);
    return 4;
  }
#define RAYS_EMUL_CASE(E, DV) if (e == E && d == DV) return emul_lane_shape<Pred, E, DV>(ns, nv, f);
  RAYS_EMUL_CASE(0, 0) RAYS_EMUL_CASE(0, 1) RAYS_EMUL_CASE(1, 0) RAYS_EMUL_CASE(1, 1) RAYS_EMUL_CASE(2, 0) RAYS_EMUL_CASE(2, 1)
  RAYS_EMUL_CASE(4, 0) RAYS_EMUL_CASE(4, 1) RAYS_EMUL_CASE(5, 0) RAYS_EMUL_CASE(5, 1) RAYS_EMUL_CASE(6, 0) RAYS_EMUL_CASE(6, 1)
#undef RAYS_EMUL_CASE
  return 4;
}

// ---- the whole-wave shape lists (emul_group.cpp has one per runner) ----
template <int EQ_, int NS_, int NV_>
struct WaveShape { static constexpr int EQ = EQ_, NS = NS_, NV = NV_; };
template <class... S> struct WaveShapes {};
template <class Pred, class S, class F>
static int emul_wave_shape(F& f) {
  if constexpr (Pred::template wave<S>) return f(S{});
  else return 4;
}
// Hands the listed shape that matches p to f as a type, if Pred::wave<S> takes it; 4: not built.
template <class Pred, class F, class... S>
static int emul_wave_dispatch(WaveShapes<S...>, const rays_params_t* p, F f) {
  const int e = emul_eq(p), ns = p->nspec + 1, nv = p->nv;
  int rc = 4;
  (void)((e == S::EQ && ns == S::NS && nv == S::NV && ((rc = emul_wave_shape<Pred, S>(f)), true)) || ...);
  return rc;
}
