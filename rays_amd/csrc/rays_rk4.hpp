// rays_rk4.hpp -- RK4 ray-trace kernel (ode_solver_name = 'RK4_ODE').
//
// Reference path restated here:
//   trace_rays   ray_tracing.f90:67-264   (per-ray bookkeeping, stop logic, recording)
//   RK4_ode      RK4_ode_m.f90:59-94      (4 stages, early return leaves v untouched)
//   eqn_ray / check_save                  (rays_device.hpp)
//
// One iteration of the wave loop is one RK4 STEP: a counted loop over the four RHS evaluations, in the order
//   stage 3     : w = v + ds*(f1 + 2 f2 + 2 f3 + f4)/6 ; check_save(w) fused with the next step's
//                 f1 = eqn_ray(w) (same equilibrium + dispersion derivatives, evaluated once)
//   stage 0,1,2 : evaluate f at w (= v + ds*f1/2, v + ds*f2/2, v + ds*f3)  -> f2, f3, f4
// A new ray starts in stage 3 with w = v0 (`first`), which is exactly the reference's initial
// check_save call (ray_tracing.f90:100) and also yields the first step's f1.
// A lane under way runs one stage per evaluation and a wave starts rays only between two iterations, so every
// lane under way is at the stage of the copy of the loop body it is in: the stage is no variable.  The
// one-wave-per-SIMD kernel unrolls the stage loop -- the stage and do_check are compile-time constants of each
// copy, check_save's share, the record path and the next step's preparation exist once, in the stage-3 copy,
// and the other three copies hold the light arm alone.  Whether a pass is due is asked once per step; when no
// lane is under way after a stage, a scalar branch leaves the step (rays_rk4_body.inc).  The two-waves-per-SIMD
// kernel runs ONE evaluation per iteration with the stage in a wave-uniform scalar (as a rolled stage loop it
// needed 12 more registers and the 1 M-ray slab fan ran 2 % slower).
//
// Recorded points: the one-wave-per-SIMD kernel with nv = 7 passes them through a per-lane LDS window
// and writes whole 64-byte sectors (PointWindow, rays_trace.hpp: HBM write traffic 1.06x the
// algorithmic bytes for 1.3 % of the pass; with nv = 8 only residual(:) needs it, a ray_vec record being
// one sector); the other builds store each point directly from its lane
// (record_point: 2.1x the bytes through partly written sectors, no LDS).  The kernel is bound by
// instruction issue, not by HBM, so what matters is the issue slots the recording
// costs: ~50 per step for the window, 14 for direct stores, ~500 for an earlier cooperative flush of
// 512-byte runs (12 % of the pass).  -DRAYS_RK4_DIRECT_STORES builds the kernel without the window.
#pragma once

#include "rays_trace.hpp"
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
#include <cstdio>
#endif

namespace rays {

// ---- rk4_resume_ray: a ray the tolerance kernels handed over, continued to its end as trace_rays has it ----------
// (ray_tracing.f90:118-260, RK4_ode_m.f90:59-94), one ray per lane, plainly: step, check_save, record, next.  The
// tolerance kernel left the ray with stop code kStopResumeExact, npoints so far, v at the start of the step it did not
// commit (end_ray_vec), the running maximum of the residuals (max_residuals); the recorded residuals are in the array.
// Only instantiated in EXACT translation units (rays_inst.hip), so its arithmetic is the reference's and the points it
// records are the exact kernels', bit for bit -- tests/test_gpu_tolerance_flavour.py hands WHOLE rays over to check that.
// A handful of steps per ray at most (the last one or two of a ray that runs into dD/dw -> 0): divergence and the five
// evaluations per step (four stages + check_save, not fused here) do not matter; points are stored directly.
template <int EQ, int NS, int DERIV, int NV>
RAYS_DEV void rk4_resume_ray(const DevParams& P, const TraceArgs& A, int ray) {
  const long long npt = (long long)P.nstep_max + 1;
  double v[NV], w[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) v[i] = A.end_ray_vec[(long long)ray * NV + i];
  int nstep = A.npoints[ray] - 1;
  double maxr = A.max_residuals[ray];
  double last_resid = A.residual[(long long)ray * npt + nstep];
  double prev_resid = nstep >= 1 ? A.residual[(long long)ray * npt + nstep - 1] : 0.;
  double ds_ray = P.ds;
  if (A.rays_per_run > 0) ds_ray = A.ds_run[ray / A.rays_per_run];
  // the ray parameter as trace_rays accumulates it: sout = sout + ds, once per step taken (start_ray, rays_rk4_body.inc)
  double sout = A.s0 ? A.s0[ray] : 0., s = sout;
  for (int k = 0; k <= nstep; k++) {
    s = sout;
    sout = sout + ds_ray;
  }
  int stop;
  for (;;) {
    const double dsl = sout - s;  // RK4_ode_m.f90:81
    stop = rk4_step_as_reference<EQ, NS, DERIV, NV>(P, v, dsl, w);
    if (stop) break;  // :83-89 a stage refused: v untouched, the ray ends
    double f[NV], resid;
    int code, cs_flag;
    bool cs_stop;
    rhs_eval<EQ, NS, DERIV, NV>(P, w, true, resid, cs_flag, cs_stop, code, f);  // check_save + the next step's first stage
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = w[i];
    s = sout;
    if (cs_stop) {  // ray_tracing.f90:214-234: step not recorded, v is the new state
      stop = cs_flag;
      break;
    }
    nstep = nstep + 1;  // :237-243
    record_point<NV>(A, (long long)ray * npt + nstep, v, resid);
    if (fabs(last_resid) > maxr) maxr = fabs(last_resid);
    prev_resid = last_resid;
    last_resid = resid;
    sout = sout + ds_ray;  // :118-172
    if (sout > P.s_max) {
      stop = RAYS_STOP_SOUT_GT_SMAX;
      break;
    }
    if (nstep + 1 > P.nstep_max) {
      stop = RAYS_STOP_NSTEP_MAX;
      break;
    }
    if (code) {  // first RK4 stage of the next step stops (RK4_ode_m.f90:82-83)
      stop = code;
      break;
    }
  }
  A.npoints[ray] = nstep + 1;  // ray_tracing.f90:252-260
  A.stop_code[ray] = stop;
#pragma unroll
  for (int i = 0; i < NV; i++) A.end_ray_vec[(long long)ray * NV + i] = v[i];
  if (A.end_residuals) A.end_residuals[ray] = nstep >= 1 ? prev_resid : 0.;
  A.max_residuals[ray] = maxr;
}

// one lane per ray of the launch; lanes whose ray was not handed over leave at once
template <int EQ, int NS, int DERIV, int NV>
__global__ void __launch_bounds__(256)
rk4_resume_kernel(const DevParams P, const TraceArgs A) {
  const int ray = blockIdx.x * blockDim.x + threadIdx.x;
  if (ray >= A.nray || A.stop_code[ray] != kStopResumeExact) return;
  rk4_resume_ray<EQ, NS, DERIV, NV>(P, A, ray);
}

#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
// Host emulation only: the trace bodies report a lane under way whose own stage differs from the stage of the copy of the
// loop body it is in (two-waves body: from its wave's stage, and a lane whose copy of that scalar differs from lane 0's)
// here -- on stderr, and counted for the test that built this.
extern "C" __attribute__((visibility("default"), used)) inline int* rays_emul_uniform_stage_violations() {
  static int n = 0;
  return &n;
}
// ... and what the batching threshold sees each time a step asks it (lane 0 of the wave records): the step's alive_sum,
// `occupied` and idle_acc after the step is settled.  [0] = number of entries asked for, then three ints per entry.
extern "C" __attribute__((visibility("default"), used)) inline int* rays_emul_threshold_log(int reset) {
  static int log[1 + 3 * 4096];
  if (reset) log[0] = 0;
  return log;
}
inline void threshold_asked(int alive_sum, int occupied, int idle_acc) {
  int* log = rays_emul_threshold_log(0);
  if (log[0] < 4096) {
    int* e = log + 1 + 3 * log[0];
    e[0] = alive_sum, e[1] = occupied, e[2] = idle_acc;
  }
  log[0]++;
}
// ... and the steps a wave left before their last stage because no lane was under way any more
extern "C" __attribute__((visibility("default"), used)) inline int* rays_emul_early_step_exits() {
  static int n = 0;
  return &n;
}
// ... and the lanes that entered the lean copy of rk4_trace_kernel's step loop (rays_trace.hpp: rk4_lean_loop)
extern "C" __attribute__((visibility("default"), used)) inline int* rays_emul_lean_loop_lanes() {
  static int n = 0;
  return &n;
}
inline void uniform_stage_violation(int ray, int lane_stage, int wave_stage) {
  int& n = *rays_emul_uniform_stage_violations();
  if (n++ < 8)
    std::fprintf(stderr, "[rays_rk4] UNIFORM STAGE VIOLATED: ray %d is at stage %d, its wave at stage %d\n", ray, lane_stage,
                 wave_stage);
}
#endif

// ---- the lean step loop of the one-wave-per-SIMD kernel ---------------------------------------------------------------
// Three switches of the Solovev RHS are constants of a RUN -- the density model, the species' temperature models
// (solovev_fields) and ray_param (ray_equations) -- yet wave-uniform branches on the parameter block inside the unrolled
// step: they cut every evaluation into a dozen basic blocks with zero-fills, selects and exec-mask regions round the
// joins, and keep the dead arms in the loop's text.  rk4_trace_kernel therefore holds its body TWICE, and a launch takes
// one copy: the lean one, compiled with the three tests false (LEAN of rhs_eval, rays_device_arith.inc), when the density
// model is not 'constant', no species has a parabolic temperature profile (ts = 0 then, as the general code computes it)
// and ray_param is not 'arcl'; the general one -- the body as it is compiled everywhere else -- otherwise.  Same
// operations in the same order: the exact kernels' results are bit-identical in both.  One copy runs per launch, so the
// instruction-cache footprint of a pass is one loop's.  Built where the stage loop is unrolled and the equilibrium is
// Solovev (rk4_lean_built); every other kernel holds the general body alone.  Same kernel, same name: what a parameter
// set takes is asked through rays_hip_rk4_loop_for (rays_capi.hip).
// (rk4_lean_built, rk4_lean_loop: rays_trace.hpp, next to the argument block the switch travels in)

#ifndef RAYS_HOST_EMUL
// One wave per SIMD (all 256 VGPRs): fastest while the fan has at most one wave per SIMD (<= 64k rays).
template <int EQ, int NS, int DERIV, int NV>
__global__ void __launch_bounds__(256)
rk4_trace_kernel(const DevParams P_kernarg, const TraceArgs A_hot) {
#ifdef RAYS_RK4_DIRECT_STORES
#define RAYS_RK4_USE_WINDOW 0
#else
#define RAYS_RK4_USE_WINDOW 1
#endif
#define RAYS_RK4_LONG_FIRST 1  // pass loop around the trip loop, rays handed out long-first (rays_rk4_body.inc)
  // the body twice, one copy per launch (rays_trace.hpp: rk4_lean_loop); the selection is made here, once, from kernel
  // arguments that are dead before the pass loop starts
  if constexpr (rk4_lean_built(EQ, NS, DERIV)) {
    if (rk4_lean_loop(P_kernarg, NS, A_hot)) {
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
      ++*rays_emul_lean_loop_lanes();
#endif
#define RAYS_RK4_LEAN 1
#include "rays_rk4_body.inc"
#undef RAYS_RK4_LEAN
      return;
    }
  }
  {
#define RAYS_RK4_LEAN 0
#include "rays_rk4_body.inc"
#undef RAYS_RK4_LEAN
  }
#undef RAYS_RK4_LONG_FIRST
#undef RAYS_RK4_USE_WINDOW
}

// Two waves per SIMD (<= 256 combined registers): from two waves' worth of rays on this build wins,
// because two waves share a SIMD's issue slots better than one (tools/ubench: 4.6 vs 5.5 clocks per
// FP64 op).  Measured on the Solovev fan: -2 % at 64k rays, +6 % at 128k, +18 % at 1M.
// rays_capi.hip: find_kernel picks by fan size.  (The launch bound must be a literal: hipcc ignores
// a template-dependent second argument.)
template <int EQ, int NS, int DERIV, int NV>
__global__ void __launch_bounds__(256, 2)
rk4_trace_kernel_w2(const DevParams P_kernarg, const TraceArgs A_hot) {
#ifdef RAYS_RK4_W2_DIRECT_STORES
#define RAYS_RK4_USE_WINDOW 0
#else
#define RAYS_RK4_USE_WINDOW 2  // residual(:) through a 30 KB window, ray_vec stored directly (rays_trace.hpp)
#endif
#define RAYS_RK4_LONG_FIRST 0  // one loop, rays in index order: what fits this build's 256 registers (rays_rk4_body.inc)
#define RAYS_RK4_LEAN 0
#include "rays_rk4_body.inc"
#undef RAYS_RK4_LEAN
#undef RAYS_RK4_LONG_FIRST
#undef RAYS_RK4_USE_WINDOW
}
#else
// (host emulation: the same two bodies, for the CPU test tier)
template <int EQ, int NS, int DERIV, int NV>
void rk4_trace_kernel_w2(const DevParams P_kernarg, const TraceArgs A_hot) {
#define RAYS_RK4_USE_WINDOW 2
#define RAYS_RK4_LONG_FIRST 0
#define RAYS_RK4_LEAN 0
#include "rays_rk4_body.inc"
#undef RAYS_RK4_LEAN
#undef RAYS_RK4_LONG_FIRST
#undef RAYS_RK4_USE_WINDOW
}
template <int EQ, int NS, int DERIV, int NV>
void rk4_trace_kernel(const DevParams P_kernarg, const TraceArgs A_hot) {
#ifdef RAYS_RK4_DIRECT_STORES
#define RAYS_RK4_USE_WINDOW 0
#else
#define RAYS_RK4_USE_WINDOW 1
#endif
#define RAYS_RK4_LONG_FIRST 1  // pass loop around the trip loop, rays handed out long-first (rays_rk4_body.inc)
  // the body twice, one copy per launch (rays_trace.hpp: rk4_lean_loop); the selection is made here, once, from kernel
  // arguments that are dead before the pass loop starts
  if constexpr (rk4_lean_built(EQ, NS, DERIV)) {
    if (rk4_lean_loop(P_kernarg, NS, A_hot)) {
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
      ++*rays_emul_lean_loop_lanes();
#endif
#define RAYS_RK4_LEAN 1
#include "rays_rk4_body.inc"
#undef RAYS_RK4_LEAN
      return;
    }
  }
  {
#define RAYS_RK4_LEAN 0
#include "rays_rk4_body.inc"
#undef RAYS_RK4_LEAN
  }
#undef RAYS_RK4_LONG_FIRST
#undef RAYS_RK4_USE_WINDOW
}
#endif

}  // namespace rays
