// rays_rk4_pass.inc -- the pass of a wave over its lanes without a ray under way (rays_rk4_body.inc includes it at
// the one place its loop structure runs it): ended rays are written out (what the LDS window still holds, the per-ray
// summary), free lanes get their next ray and start it.  Uses the body's variables.
    idle_acc = 0;
    alive_sum = 0;
    const TraceArgs& Ac = cold_args(A_hot);
#if RAYS_RK4_LONG_FIRST
    const int S = (Ac.sched_stride > 1 && (unsigned)Ac.nray > total_lanes) ? Ac.sched_stride : 0;
#else
    constexpr int S = 0;
#endif
    if (pending) {  // the ended ray: what the window still holds, the per-ray summary
      const TraceArgs& A = Ac;
      if constexpr (kWindow) {  // points still in the LDS window (nstep + 1 recorded)
        int pv, pr;
        Window::phases(A, ray, npt, pv, pr);
        win.finish(A, (long long)ray * npt, nstep + 1, pv, pr);
      }
      const int stop = first;  // parked there by the trip that ended the ray
      if constexpr (kIsContinue<EQ>) {
        // ended or paused: the lane's values go back into the state, which holds the summaries too.  s is sout as the
        // trip found it (the body assigns s = sout before it advances sout).
        state_store<NV>(A, ray, v, s, nstep, stop, last_resid, prev_resid, maxr, win0);
      } else if (stop >= 0) {  // ray_tracing.f90:252-260
        A.npoints[ray] = nstep + 1;
        A.stop_code[ray] = stop;
        if (A.end_ray_vec)
#pragma unroll
          for (int i = 0; i < NV; i++) A.end_ray_vec[(long long)ray * NV + i] = v[i];
        if (A.end_residuals) A.end_residuals[ray] = nstep >= 1 ? prev_resid : 0.;
        if (A.max_residuals) A.max_residuals[ray] = maxr;
      }
      if (S && sched_is_pilot((unsigned)ray, S))  // a pilot has ended: its neighbourhood is one of the short ones
        atomicOr(A.sched + 4 + sched_neighbourhood((unsigned)ray, S), kSchedDone);
      pending = false;
      hungry = can_refill;
    }
    if constexpr (kIsContinue<EQ>) {
      // (a ray that ended in an earlier window is not started -- it records nothing and costs no evaluation -- and its
      // lane asks again at once)
      bool skipped;
      do {
#include "rays_rk4_take.inc"
        skipped = false;
        if (need_init && Ac.stop_code[ray] != RAYS_STOP_NONE) {
          Ac.npoints[ray] = 0;
          if (S && sched_is_pilot((unsigned)ray, S)) atomicOr(Ac.sched + 4 + sched_neighbourhood((unsigned)ray, S), kSchedDone);
          need_init = false;
          hungry = can_refill;
          skipped = hungry;
        }
      } while (__any(skipped));
    } else {
#include "rays_rk4_take.inc"
    }
    if constexpr (kIsContinue<EQ>) if (need_init) {  // the saved state (rays_trace.hpp: TraceArgs::state)
      const TraceArgs::State st = Ac.state();
#pragma unroll
      for (int i = 0; i < NV; i++) w[i] = v[i] = st.v[(long long)ray * NV + i];
      sout = st.s[ray];
      ds_ray = P.ds;
      nstep = win0 = st.nstep[ray];
      s = sout;
      last_resid = st.resid[3ll * ray];
      prev_resid = st.resid[3ll * ray + 1];
      maxr = st.resid[3ll * ray + 2];
      first = 1;
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
      j_lane = 3;
#endif
      need_init = false;
      alive = true;
    }
    if (need_init) {  // initialize_ode_vector + per-ray resets (ray_tracing.f90:77-93)
      const TraceArgs& A = cold_args(A_hot);
      start_ray<EQ, NS, NV>(P, A, ray, v, sout, ds_ray);
#pragma unroll
      for (int i = 0; i < NV; i++) w[i] = v[i];
      first = 1;
#if defined(RAYS_HOST_EMUL) && defined(RAYS_EMUL_CHECK_UNIFORM_STAGE)
      j_lane = 3;
#endif
      nstep = 0;
      s = sout;
      last_resid = 0.;
      prev_resid = 0.;
      maxr = -1.7976931348623157e308;
      need_init = false;
      alive = true;
    }
    // A pass runs between two steps of the wave -- when no lane is under way or when the lanes under way are about to run
    // stage 3 -- and the rays it has just started begin there, with the step's first evaluation.
#if !RAYS_RK4_LONG_FIRST
    jw = 3;  // (the two-waves kernel's stage: wave-uniform, assigned outside every lane-divergent region)
#endif
    occupied = (int)__popcll(__ballot(alive || pending || hungry));  // constant until the next pass
