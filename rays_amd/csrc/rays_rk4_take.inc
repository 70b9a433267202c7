// rays_rk4_take.inc -- the part of the pass (rays_rk4_pass.inc) that hands the free lanes their next rays.  A file of
// its own because the continuation variant runs it in a loop (a ray that had ended before the launch is handed out and
// dropped at once) and every other kernel exactly once, as before.  Uses the pass's variables.
#if RAYS_RK4_LONG_FIRST
    if (can_refill) {  // wave-uniform; the lanes that want a ray are served together (rays_trace.hpp: take_rays)
      bool dry = false;
      const int nxt = take_rays(Ac, total_lanes, S, hungry, (int)(threadIdx.x & 63u), dry);
      if (hungry && nxt >= 0) {
        ray = nxt;
        need_init = true;
        hungry = false;
      }
      if (dry) {  // no ray is left for anybody
        can_refill = false;
        hungry = false;
      }
    }
#else
    {  // index order, one atomic per lane
      bool dry = false;
      if (hungry) {
        const unsigned nxt = atomicAdd(Ac.next_ray, 1u) + total_lanes;
        if (nxt < (unsigned)Ac.nray) {
          ray = (int)nxt;
          need_init = true;
        } else {
          dry = true;
        }
        hungry = false;
      }
      if (__any(dry)) can_refill = false;  // the counter only grows
    }
#endif
