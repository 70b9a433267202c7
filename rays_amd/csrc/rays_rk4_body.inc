// rays_rk4_body.inc -- body of the RK4 trace kernels, included textually by the two __global__
// functions of rays_rk4.hpp (they differ in their launch bounds and in RAYS_RK4_USE_WINDOW: whether
// recorded points pass through the LDS sector window of rays_trace.hpp).  It is not a function of its
// own on purpose: as a device function taking the kernel's by-value arguments by reference it
// compiled 5 % slower (the by-value kernel arguments were no longer read as plain scalar kernarg
// loads).  Uses: template parameters EQ, NS, DERIV, NV and the kernel arguments
// `const DevParams P_kernarg, const TraceArgs A_hot`; RAYS_RK4_LEAN: 1 in the copy of rk4_trace_kernel's two that a launch
// takes when the run's model switches allow it (rays_trace.hpp: rk4_lean_loop) -- its evaluations are compiled with those
// switches folded -- 0 in every other inclusion.
  constexpr bool kLean = RAYS_RK4_LEAN != 0;
  DevParams P;  // working copy: scalarised by the compiler, hot constants in vector registers
  hot_params<EQ, NS>(P_kernarg, P);
#ifndef RAYS_HOST_EMUL
  if constexpr ((EQ & 3) == RAYS_EQ_AXISYM) {
    // the spline grids' ends and spans (a_axis): read by every cell search of every evaluation, and otherwise five scalar
    // re-loads from the kernarg segment per evaluation, ~30 ns each for a lone wave (tools/ubench/mem_latency.hip)
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int j = 0; j < 3; j++) P.a_axis[a][j] = in_vgpr(P_kernarg.a_axis[a][j]);
  }
  if constexpr (RayVec<(EQ & kEqMultiSpec) != 0, NS, NV>::DAMP) {  // the Z-function spline's range: five uses per evaluation
    P.zf_xmin = in_vgpr(P_kernarg.zf_xmin);
    P.zf_xmax = in_vgpr(P_kernarg.zf_xmax);
  }
#if RAYS_RK4_LONG_FIRST
  // check_save's residual limit and the factor of dD/dw (deriv_cold): otherwise scalar re-loads from the kernarg segment
  // inside the evaluation (~30 ns each for a lone wave) or two more scalar registers held across the unrolled step.  No
  // gain on the Solovev headline (2.019 against 2.033 ms), but without them the axisym kernel of cfg 5b, which spills
  // scalar registers, is 3.5 % SLOWER than before the step loop (2.113 -> 2.188 ms) and with them 1.6 % faster (2.083):
  // profiles/r05/measurements/rk4_step_loop_ab.txt.  The one-wave-per-SIMD kernel has the vector registers.
  P.resid_limit = in_vgpr(P_kernarg.resid_limit);
  P.m1_over_omgrf = in_vgpr(P_kernarg.m1_over_omgrf);
#endif
#endif

  const unsigned total_lanes = gridDim.x * blockDim.x;
  const long long npt = (long long)P.nstep_max + 1;

  // ---- per-lane ray state -------------------------------------------------------------------
  int ray = blockIdx.x * blockDim.x + threadIdx.x;
  bool alive = false;                 // holds a ray that is under way
  bool need_init = ray < A_hot.nray;  // holds a ray that has not started yet
  bool hungry = false;                // holds nothing and wants a ray (take_rays, rays_trace.hpp)
#if RAYS_RK4_LONG_FIRST
  if (A_hot.sched_stride > 1 && (unsigned)A_hot.nray > total_lanes) {
    // "long rays first": the lanes start with the pilots (rays_trace.hpp: take_rays)
    const unsigned m = (unsigned)ray, r = sched_pilot_ray(m, A_hot.sched_stride);
    need_init = m < sched_pilots((unsigned)A_hot.nray, A_hot.sched_stride) && r < (unsigned)A_hot.nray;
    hungry = !need_init;
    ray = (int)r;
  }
#endif
  // One-wave-per-SIMD kernel (RAYS_RK4_LONG_FIRST): one iteration of the inner loop is one RK4 STEP of the wave, a counted
  // loop over the four evaluations in the order stage 3, 0, 1, 2.  A ray starts at stage 3 -- the first evaluation of an
  // iteration -- a lane under way runs one stage per evaluation and never sits one out, and a pass starts rays only
  // between two iterations: so every lane under way is at the stage of the loop's copy it is in, and the stage is no
  // variable of the kernel at all.  The stage loop is unrolled: the stage and do_check are compile-time constants of each
  // copy (check_save's share, the record path and the next step's preparation exist in the stage-3 copy only; `acc = f`
  // and `v = w` are renames), and the test "is a pass due" runs once per step.  Headline 2.35 -> 2.02 ms.
  // The two-waves-per-SIMD kernel keeps one evaluation per iteration and the stage as a wave-uniform scalar `jw` (see its
  // loop head below): the same invariant, checked trip by trip.
  // (-DRAYS_EMUL_CHECK_UNIFORM_STAGE, host emulation only: every lane also keeps the stage it would have on its own,
  // and a lane under way that disagrees with the copy it is in is reported -- rays_rk4.hpp: uniform_stage_violation.)
  // Unrolled where the four copies of the evaluation stay a few thousand instructions (the analytic derivatives, up to
  // two species).  The larger evaluations (finite differences, multi-species damping, more species) run the same loop
  // rolled: four copies of them pass the compiler's limit for a requested unroll (it then leaves the loop rolled and
  // warns) and the 64 KB instruction cache.  That form is not measured on a GPU (no BASELINE config runs it; DESIGN.md 4.1).
  constexpr bool kUnrollStages =
      RAYS_RK4_LONG_FIRST && DERIV == RAYS_DERIV_COLD && (EQ & kEqMultiSpec) == 0 && NS <= 2;
  [[maybe_unused]] constexpr int kStageUnroll = kUnrollStages ? 4 : 1;
#if !RAYS_RK4_LONG_FIRST
  int jw = 3;  // the two-waves kernel's stage: wave-uniform, never assigned under lane-divergent control (see its loop)
#endif
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
  int j_lane = 3;
#endif
  // stage-3 evaluation is the initial check_save (int, not bool: see rays_sg.hpp); of a parked lane: its stop code
  int first = 1;
  int nstep = 0;
  double s = 0., sout = 0., dsl = 0.;
  double ds_ray = P.ds;  // output step of this lane's run (a fused scan gives every run its own)
  double v[NV], w[NV], acc[NV];
  double last_resid = 0., prev_resid = 0., maxr = -1.7976931348623157e308;
#pragma unroll
  for (int i = 0; i < NV; i++) v[i] = w[i] = acc[i] = 0.;

  const Recip R6 = const_recip(6.0, 1.0 / 6.0);  // RN(1/6); div() = the correctly rounded quotient
  typedef PointWindow<NV, RAYS_RK4_USE_WINDOW == 2> Window;  // rays_trace.hpp (2: residual(:) only)
  constexpr bool kNoTraj = (EQ & kEqNoTraj) != 0;  // summary-only variant: no point is recorded, no window exists
  // continuation variant (kEqContinue; DESIGN.md 4.10): rays start from the saved state and are paused into it after the
  // launch's n_steps recorded steps; points are stored directly into the window slab [nray][n_steps].  (kIsContinue<EQ>,
  // rays_trace.hpp: a constant of namespace scope -- one more local constant here moves instructions in the kernels
  // that do not have the bit, and those are to come out of the compiler exactly as they were.)
  static_assert(!kIsContinue<EQ> || (RAYS_RK4_LONG_FIRST && !(EQ & kEqTol) && (!(EQ & kEqDeposit) || (EQ & kEqNoTraj))),
                "the continuation variant: an exact one-wave-per-SIMD kernel, recording, summary-only or fused deposition");
  constexpr bool kWindow = RAYS_RK4_USE_WINDOW && Window::kAny && !kNoTraj && !kIsContinue<EQ>;
  // fused deposition variant (kEqDeposit; rays_deposition.hpp): an accepted point is binned into the ray's row of work.
  // The grid value and the absorbed power of the ray's last recorded point belong to the ray: set at its point 1.
  constexpr bool kDeposit = (EQ & kEqDeposit) != 0;
  static_assert(!kDeposit || (kNoTraj && RayVec<(EQ & kEqMultiSpec) != 0, NS, NV>::DAMP),
                "the fused deposition variant: a summary-only kernel with the absorbed-power row");
  [[maybe_unused]] double dep_x_prev = 0., dep_q_prev = 0.;
  // two-profile variant (kEqDeposit2): the second profile's grid value of that point; q is shared
  static_assert(!kIsDeposit2<EQ> || (kDeposit && (EQ & 3) == 2), "the two-profile variant: a fused axisym_toroid kernel");
  [[maybe_unused]] double dep_x2_prev = 0.;
  extern __shared__ double lds[];
  Window win;
  if constexpr (kWindow) win.attach(lds, threadIdx.x);
#ifndef RAYS_HOST_EMUL
  if constexpr (RAYS_RK4_USE_WINDOW == 1 && zf_tab_lds_bytes<EQ, NS, NV>() > 0) {
    // damping: the Z-function spline table into LDS (behind the window and the eqdsk tables)
    const int n = 4 * P.zf_nx;
    if (P.damping_model && n > 0 && (size_t)n * sizeof(double) + 64 <= kZfTabBytes) {
      double* tab = lds + (window_lds_bytes<EQ, NV>() + eq_tab_lds_bytes<EQ, NV>() + 64) / sizeof(double);
      for (int i = threadIdx.x; i < n; i += blockDim.x) tab[i] = P.zf_fspl[i];
      __syncthreads();
      P.zf_lds = (unsigned)(unsigned long long)(trace_lds_ptr)tab;
    }
  }
  if constexpr (RAYS_RK4_USE_WINDOW == 1 && eq_tab_lds_bytes<EQ, NV>() > 0) {
    // eqdsk equilibrium: the 1-D spline tables (RBphi(R), n(psi), Te(psi), Ti(psi): a few KB) into LDS
    const int n = P.a_tab1d_doubles, nrz = P.a_nr + P.a_nz;
    if (n > 0 && (size_t)(n + nrz) * sizeof(double) <= kEqTabBytes) {
      double* tab = lds + (window_lds_bytes<EQ, NV>() + kEqTabPad) / sizeof(double);
      for (int i = threadIdx.x; i < n; i += blockDim.x) tab[i] = P.a_rb_grid[i];
      for (int i = threadIdx.x; i < P.a_nr; i += blockDim.x) tab[n + i] = P.a_r_grid[i];
      for (int i = threadIdx.x; i < P.a_nz; i += blockDim.x) tab[n + P.a_nr + i] = P.a_z_grid[i];
      __syncthreads();
      P.a_lds_tab = (unsigned)(unsigned long long)(trace_lds_ptr)tab;
      P.a_lds_rz = (unsigned)(unsigned long long)(trace_lds_ptr)(tab + n);
    }
  }
#endif

  // ---- lanes without a ray under way: batched ray ends and starts ---------------------------------
  // What a ray's end and the next ray's start cost the WAVE (the tail of the LDS window, the per-ray summary
  // behind four dependent kernarg reads, the refill atomic behind every store in flight, initialize_ode_vector:
  // together four to five trips' worth of clocks, run with one or two lanes active) is paid per EVENT, not per
  // lane.  A lane whose ray has ended therefore only parks it (`pending`: v, nstep, the stop code -- in j --
  // and the window rows stay where they are) and the wave handles all parked lanes in one pass: their tails and
  // summaries, one atomic each, the new rays' starts.  The pass runs when the idle lane-trips accumulated since
  // the last one have reached its own cost (the square-root rule of batching: both losses equal), at once when
  // no lane is under way, and -- if no ray is left to hand out -- only then.  Scheduling only: no lane's
  // arithmetic changes.  (Headline and cfg 5b -4 %: neighbouring rays mostly end on the same trips -- a wave of cfg 5b
  // sees a dozen passes -- so the threshold hardly matters; what the pass saves is the lane-by-lane end code.)
#ifndef RAYS_REFILL_EVENT_COST
#define RAYS_REFILL_EVENT_COST 256  // lane-trips
#endif
  bool pending = false;                         // holds an ended ray that is not written out yet
  // ---- ill-conditioned steps are handed over to the reference's arithmetic (tolerance flavour) --------------------
  // A ray of the Solovev fans ends by running into the coalescence of two modes: dD/dw -> 0, and a stage of its last
  // recorded step lands where one unit of the last place of the stage's INPUT moves the step's result by 1e-10 and
  // more, so no arithmetic but the reference's own lands within north_star's bar of the reference's point (measured on
  // the headline fan without this: 13 of 12 873 661 steps above 1e-10, max 4.5e-10, each a ray's last recorded step;
  // with it: none above 1e-12, max 5e-15 -- tests/test_gpu_numerics_full_fans.py).  Detection: dD/dw of a stage
  // evaluation has fallen below RAYS_RK4_HANDOVER_RATIO of its value at the step's first evaluation (or changed sign, or
  // is NaN) -- tested on the step's LAST stage, which sits a whole step ahead (in every such step of the BASELINE fans
  // it is the one that collapses: ratios 0.6, 0.5, 0.0003 over the three stages) -- the lane is then `suspect`.  It finishes the step all the same; if check_save ends the ray there, that is
  // that (the step is not recorded; every second suspect step is a ray's last attempt).  Otherwise the step is NOT
  // committed: the ray ends here for this kernel with the internal stop code kStopResumeExact and the summary the pass
  // writes anyway -- npoints so far, v at the step's start (end_ray_vec), the residual statistics -- and
  // rk4_resume_kernel (rays_rk4.hpp; an EXACT translation unit, launched behind this kernel by rays_capi.hip) takes
  // the step again from there and runs the ray to its end, a step or two later, bit-identically to the exact kernels.
  // (Taking the step again INSIDE this kernel, with a second copy of the arithmetic compiled without re-association
  // and contraction, gave the same numbers and cost the hot loop 16 % by its mere presence -- 66 spilled SGPRs, 84
  // AGPRs of parked values -- inlined or behind a call: profiles/r04/measurements/retake_in_kernel_ab.txt.)
#undef RAYS_RK4_HANDOVER
// (RAYS_EMUL_HANDOVER: the CPU tier's build of these sources, tests/hip_emul/emul_trace.cpp, runs the same hand-over
// and resume with the one arithmetic the host has: bit-identical to the fixtures by construction, control flow covered.)
// Built into the one-wave-per-SIMD kernel only.  In the two-waves build (one loop, 230 registers) the same few lines cost
// the 1 M-ray slab fan of cfg 4 24 % (28.2 -> 35.0 ms, A/B on one box: profiles/r04/measurements/w2_handover_ab.txt),
// and that fan has no such step: max per-step deviation 4.6e-13 over 32.8 M restarts without it.  Under the tolerance
// setting the dispatcher therefore takes the two-waves build for the slab only (rays_capi.hip: find_kernel): a Solovev
// or axisym fan of any size runs the one-wave kernel with the hand-over, so that its last steps keep the bar too.
#if (defined(RAYS_TOL_FLAVOUR) || defined(RAYS_EMUL_HANDOVER)) && RAYS_RK4_LONG_FIRST && !defined(RAYS_RK4_NO_HANDOVER)
#define RAYS_RK4_HANDOVER 1
#else
#define RAYS_RK4_HANDOVER 0
#endif
#ifndef RAYS_RK4_HANDOVER_RATIO
#define RAYS_RK4_HANDOVER_RATIO 0.5
#endif
  // dD/dw at the step's first evaluation; NaN = a stage of the step under way ran into dD/dw -> 0 ("suspect": the flag
  // travels in the value -- a lane mask of its own across the wave loop cost 23 spilled SGPRs)
  double dddw_f1 = 0.;
  bool can_refill = (unsigned)A_hot.nray > total_lanes;  // wave-uniform: the counter may still hand out a ray
  // Idle lane-trips since the last pass (wave-uniform).  A pass can only fall between two steps, so the sum is settled
  // once per step (by the two-waves kernel: on the trip that stage 3 follows).  Between two passes the lanes that hold a
  // ray or want one (`occupied`, counted by the pass) stay the same and lanes only go from under way to parked, so the
  // idle lanes of a trip are occupied minus the lanes under way: every stage adds its count of lanes under way to
  // alive_sum -- the count that also tells whether any lane is left -- and the step settles:
  // idle_acc += 4 * occupied - alive_sum.  Step for step the sum the threshold sees is what a ballot of the parked lanes
  // on every trip gave.
  int idle_acc = 0, alive_sum = 0, occupied = 0;
  [[maybe_unused]] int win0 = 0;  // continuation variant: steps the ray had recorded when this window began
  // RAYS_RK4_LONG_FIRST (the one-wave-per-SIMD kernel): two loops -- the outer one is the pass (cold: a handful of
  // times per wave), the inner one the trips between two passes (hot) -- and the rays are handed out "long rays first"
  // (rays_trace.hpp: take_rays).  As ONE loop with that pass inside an `if`, the pass's registers (cursors, window
  // tails, the new rays' start) were allocated against the hot trip's: 25 % more vector instructions per trip, moves
  // all of them (headline 2.50 -> 2.85 ms).  The two-waves-per-SIMD kernel keeps one loop, the smaller pass that
  // hands rays out in index order, and its 228 registers: with two loops it needed 256 + 75 spilled to scratch.
#if RAYS_RK4_LONG_FIRST
  for (;;) {
    {
#include "rays_rk4_pass.inc"
    }
    if (!__any(alive)) {
      if (!__any(hungry)) break;
      continue;  // lanes that found their probe budget spent ask again
    }
    bool fire;
    do {  // ---- the steps until the next pass is due ----
      int n_alive = 0;
#else
  // The two-waves-per-SIMD kernel keeps ONE evaluation per iteration and the stage as a wave-uniform scalar, advanced
  // once per trip and set to 3 by the pass: as a rolled stage loop it needed 238 registers for 226 and the 1 M-ray slab fan
  // of cfg 4 ran 2.2 % slower (29.21 -> 29.85 ms, profiles/r05/measurements/rk4_step_loop_ab.txt).
  for (;;) {
    const int n_alive = (int)__popcll(__ballot(alive));
    bool fire = false;
    if (n_alive == 0) {  // wave-uniform
      fire = __any(pending || need_init);
    } else {
      alive_sum += n_alive;
      if (jw == 3) {  // the lanes under way are about to run stage 3: fresh rays can join them in step
        if (can_refill && occupied > n_alive) {
          idle_acc += 4 * occupied - alive_sum;
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
          if ((threadIdx.x & 63u) == 0) threshold_asked(alive_sum, occupied, idle_acc);
#endif
          fire = idle_acc >= RAYS_REFILL_EVENT_COST;
        }
        alive_sum = 0;
      }
    }
    if (fire) {
#include "rays_rk4_pass.inc"
    }
    if (!__any(alive)) break;
    {
#endif

    // ---- one RK4 step: the evaluations of stage 3 (check_save + the step's first stage), 0, 1, 2 -----------------------
#if RAYS_RK4_LONG_FIRST
#pragma unroll kStageUnroll
    for (int k = 0; k < 4; k++) {
    const int jw = (k + 3) & 3;
#else
    {
#endif
    // ---- the RHS evaluation of this stage ----------------------------------------------------
    double f[NV], resid = 0.;
    int code = 0, cs_flag = 0;
    bool cs_stop = false;
    // ---- the lanes under way: ONE region -- the evaluation, then the arm of the stage.  Unrolled, the stage is a constant
    // of this copy and only its own arm is left; rolled (and in the two-waves kernel) the arms are scalar branches on the
    // wave's stage.  (A lane whose ray ends is parked until the wave's next pass over its idle lanes: its stop code goes
    // into `first`.)
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
#if !RAYS_RK4_LONG_FIRST
    // (the stage is a variable here: every lane of the emulated wave keeps its own copy, which must be lane 0's)
    if (__shfl(jw, 0) != jw) uniform_stage_violation(ray, alive ? j_lane : -1, jw);
#endif
    if (alive && j_lane != jw) uniform_stage_violation(ray, j_lane, jw);
    j_lane = (j_lane + 1) & 3;
#endif
    if (alive) {
#if RAYS_RK4_HANDOVER
      // (the detection itself sits in the state machine's own branches below -- stage 2 tests, stage 3 re-arms: as a
      // block of its own behind the evaluation it cost the trip four more exec-mask regions and 7 % of the pass)
      double dddw_now = 0.;
      if constexpr (DERIV == RAYS_DERIV_COLD)
        rhs_eval<EQ, NS, DERIV, NV, kLean>(P, w, jw == 3, resid, cs_flag, cs_stop, code, f, &dddw_now);
      else
#endif
        rhs_eval<EQ, NS, DERIV, NV, kLean>(P, w, jw == 3, resid, cs_flag, cs_stop, code, f);
      // The two arms are two if-then regions in sequence, not an if / else: as an if / else the compiler's structured
      // control flow runs the second arm behind a guard AFTER the first, keeps the first arm's inputs alive for it and
      // joins the arms' results by copies (33 64-bit moves per stage-3 trip, 8 per other trip); in sequence each arm
      // updates acc, w and v in place.  Hence, where the stage loop is rolled, the second, opaque copy of the stage for the
      // second test (unrolled, each copy holds the arm of its stage alone and the tests fold away).
      int jw_again = jw;
#ifndef RAYS_HOST_EMUL
      if constexpr (!kUnrollStages) asm volatile("" : "+s"(jw_again));
#endif
      if (jw != 3) {
        // Stages 0, 1, 2: acc += c f (c = 2, 2, 1) and w = v + (ds f)/2, v + ds f, v + (ds acc)/6.  The products by the
        // wave-uniform 1.0 and 2.0 are exact, so every stage rounds as it does written out on its own.  Updated whether
        // or not the stage stopped (RK4_ode_m.f90:83-89 leaves v untouched): acc and w of a parked lane are dead.
        if (jw == 2) {
#pragma unroll
          for (int i = 0; i < NV; i++) {
            acc[i] = acc[i] + f[i];
            w[i] = v[i] + div(dsl * acc[i], R6);  // RK4_ode_m.f90:91  (ds*(...))/6.0
          }
#if RAYS_RK4_HANDOVER
          // the last stage sits a whole step ahead: has dD/dw collapsed (or changed sign, or is it NaN) since the step's start?
          if constexpr (DERIV == RAYS_DERIV_COLD)
            if (!(dddw_now * dddw_f1 >= RAYS_RK4_HANDOVER_RATIO * (dddw_f1 * dddw_f1))) dddw_f1 = __builtin_nan("");
#endif
        } else {
          const double h = jw == 0 ? 0.5 : 1.0;
#pragma unroll
          for (int i = 0; i < NV; i++) {
            acc[i] = acc[i] + 2.0 * f[i];
            w[i] = v[i] + dsl * f[i] * h;  // (ds*f2)/2.0, exact scaling; ds*f3
          }
        }
        if (code) {  // the stage stopped
          alive = false;
          pending = true;
          first = code;
        }
      }
      if (jw_again == 3) {
        int stop = 0;        // 0 = keep going
        int done = 0;        // ray finished this trip
        // stage 3: w is the new state; check_save decides whether the step is recorded
        if (first) {
          // ray_tracing.f90:92-112: point 1 = initial state, residual(1) = 0
          if constexpr (kIsContinue<EQ>) {
            // a continued ray's first evaluation, at its saved point: the next step's first stage and nothing else -- the
            // point was recorded (and passed check_save) by the launch that paused the ray there; cs_stop is not looked at.
            // It was also the last point binned (DESIGN.md 4.10.1): its grid value and absorbed power are what the one-shot
            // kernel carries in registers here (dep_trace_segment ends by calling dep_trace_point on the same v).
            if constexpr (kIsDeposit2<EQ>) {
              const TraceArgs& A = cold_args(A_hot);
              dep2_trace_first(P, *A.dep2(), ray, v, dep_x_prev, dep_x2_prev, dep_q_prev);
            } else if constexpr (kDeposit) {
              const TraceArgs& A = cold_args(A_hot);
              dep_trace_point(P, *A.dep(), ray, v, dep_x_prev, dep_q_prev);
            }
          } else if constexpr (kNoTraj) {  // ... of which the summaries keep the state: start_ray_vec (ray_tracing.f90:259)
            const TraceArgs& A = cold_args(A_hot);
            double* const start = A.start_ray_vec();
            if (start)
#pragma unroll
              for (int i = 0; i < NV; i++) start[(long long)ray * NV + i] = v[i];
            if constexpr (kIsDeposit2<EQ>) dep2_trace_first(P, *A.dep2(), ray, v, dep_x_prev, dep_x2_prev, dep_q_prev);
            else if constexpr (kDeposit) dep_trace_point(P, *A.dep(), ray, v, dep_x_prev, dep_q_prev);
          } else if constexpr (kWindow) {
            int pv, pr;
            Window::phases(A_hot, ray, npt, pv, pr);
            win.put(A_hot, (long long)ray * npt, 0, pv, pr, v, 0.);
          } else {
            record_point<NV>(A_hot, (long long)ray * npt, v, 0.);
          }
          if (!kIsContinue<EQ> && cs_stop) {  // ray did not start: npoints = 1, summary fields stay zero
            const TraceArgs& A = cold_args(A_hot);
            A.npoints[ray] = 1;
            A.stop_code[ray] = cs_flag;
            if (A.end_ray_vec)
#pragma unroll
              for (int i = 0; i < NV; i++) A.end_ray_vec[(long long)ray * NV + i] = 0.;
            if (A.end_residuals) A.end_residuals[ray] = 0.;
            if (A.max_residuals) A.max_residuals[ray] = 0.;
            done = 1;
            stop = -1;  // summary already written
          }
          first = 0;
        } else if (RAYS_RK4_HANDOVER && DERIV == RAYS_DERIV_COLD && RAYS_RARE(dddw_f1 != dddw_f1 && !cs_stop)) {
          // an ill-conditioned step that would be recorded: not committed (v, s as at its start); rk4_resume_kernel takes over
          stop = kStopResumeExact;
          done = 1;
        } else {
#pragma unroll
          for (int i = 0; i < NV; i++) v[i] = w[i];  // RK4_ode_m.f90:91-92
          s = sout;
          if (cs_stop) {  // ray_tracing.f90:214-234: step not recorded, v is the new state
            stop = cs_flag;
            done = 1;
          } else {  // :237-243
            nstep = nstep + 1;
            if constexpr (kNoTraj) {
              // the point is counted, not stored -- and binned by the fused deposition variant
              if constexpr (kIsDeposit2<EQ>) {
                const TraceArgs& A = cold_args(A_hot);
                dep2_trace_segment(P, *A.dep2(), ray, A.nray, v, dep_x_prev, dep_x2_prev, dep_q_prev);
              } else if constexpr (kDeposit) {
                const TraceArgs& A = cold_args(A_hot);
                dep_trace_segment(P, *A.dep(), ray, A.nray, v, dep_x_prev, dep_q_prev);
              }
            } else if constexpr (kIsContinue<EQ>) {  // the point's place in the window slab
              record_point<NV>(A_hot, (long long)ray * A_hot.win_steps() + (nstep - win0 - 1), v, resid);
            } else if constexpr (kWindow) {
              int pv, pr;
              Window::phases(A_hot, ray, npt, pv, pr);
              win.put(A_hot, (long long)ray * npt, nstep, pv, pr, v, resid);
              if ((nstep & 7) == 7) win.flush(A_hot, (long long)ray * npt, (nstep + 1) >> 3, pv, pr);
            } else {
              record_point<NV>(A_hot, (long long)ray * npt + nstep, v, resid);
            }
            if (fabs(last_resid) > maxr) maxr = fabs(last_resid);
            prev_resid = last_resid;
            last_resid = resid;
            if constexpr (kIsContinue<EQ>) {
              // the window's end: the ray is paused where trace_rays stands at ray_tracing.f90:116, before sout is
              // advanced and before any of the next trip's three tests (the launch that continues it applies them)
              if (nstep - win0 >= A_hot.win_steps()) {
                stop = kStopPaused;
                done = 1;
              }
            }
          }
        }
#if RAYS_RK4_HANDOVER
        dddw_f1 = dddw_now;  // this evaluation is also the next step's first
#endif
        // Top of the next trajectory trip, ray_tracing.f90:118-172, and the first stage of the next step -- without a
        // branch: s, sout, dsl, acc and w of a lane that parks here are dead, so a ray that has just ended computes them too
        // (the reference's order of the three tests is kept by the order of the selects).
        s = sout;
        sout = sout + ds_ray;
        if (!done) {
          stop = code;  // first RK4 stage of the next step stops (RK4_ode_m.f90:82-83)
          if (nstep + 1 > P.nstep_max) stop = RAYS_STOP_NSTEP_MAX;
          if (sout > P.s_max) stop = RAYS_STOP_SOUT_GT_SMAX;
          done = stop != 0;
        }
        {
          RAYS_FP_AS_WRITTEN  // (s + ds) - s as the reference rounds it -- re-association folds it to ds
          dsl = sout - s;     // RK4_ode_m.f90:81
        }
#pragma unroll
        for (int i = 0; i < NV; i++) {
          acc[i] = f[i];
          w[i] = v[i] + dsl * f[i] * 0.5;
        }
        if (done) {
          alive = false;
          pending = true;
          first = stop;
        }
      }
    }
#if RAYS_RK4_LONG_FIRST
    // the lanes still under way: what the step's idle lane-trips are settled with, and nobody left ends the step early
    n_alive = (int)__popcll(__ballot(alive));
    alive_sum += n_alive;
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
    if (n_alive == 0 && k < 3 && (threadIdx.x & 63u) == 0) ++*rays_emul_early_step_exits();
#endif
    if (n_alive == 0) break;  // wave-uniform
    }
#else
    jw = (jw + 1) & 3;
    }
#endif
#if RAYS_RK4_LONG_FIRST
    // ---- is a pass due? ------------------------------------------------------------------------------------------------
    // A fresh ray joins the lanes under way at stage 3 (its first evaluation is the initial check_save), the first
    // evaluation of a step: the threshold is asked once per step.
    fire = n_alive == 0;
    if (!fire) {  // wave-uniform
      if (can_refill && occupied > n_alive) {
        idle_acc += 4 * occupied - alive_sum;
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
        if ((threadIdx.x & 63u) == 0) threshold_asked(alive_sum, occupied, idle_acc);
#endif
        fire = idle_acc >= RAYS_REFILL_EVENT_COST;
      }
      alive_sum = 0;
    }
    } while (!fire);
  }
#else
    }
  }
#endif
