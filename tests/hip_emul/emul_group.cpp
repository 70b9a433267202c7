// TEST INFRASTRUCTURE ONLY: the lane-group Shampine-Gordon kernel (rays_amd/csrc/rays_sg_group.hpp) on the host wave
// emulator (hip/hip_wave_emul.h: 64 lanes per wave as fibers, __shfl / __any / __ballot are rendezvous), compared with
// the reference fixtures and the oracle by tests/test_cpu_group_emul.py.  Built as its own library: with
// RAYS_EMUL_WAVE the cross-lane operations are collective, so only kernels that issue them from wave-uniform control
// flow can run here (the one-lane entries of emul_trace.cpp are compiled along for their table plumbing, not called).
#define RAYS_EMUL_WAVE 1
#include "emul_trace.cpp"
#include "../../rays_amd/csrc/rays_sg_group.hpp"

// ---- the three whole-wave runners and the shapes (EQ, NS, NV) each is built for (cold derivatives, except the lane
// group: numerical).  A variant build (emul_summary.cpp, ...) hands its flags in EQ and narrows a list with a predicate.
typedef WaveShapes<WaveShape<0, 2, 7>, WaveShape<4, 2, 7>, WaveShape<1, 2, 7>, WaveShape<5, 2, 7>, WaveShape<2, 2, 8>,
                   WaveShape<6, 2, 8>, WaveShape<4, 2, 8>> Rk4WaveShapes;
typedef WaveShapes<WaveShape<1, 2, 7>, WaveShape<5, 2, 7>, WaveShape<2, 2, 8>, WaveShape<6, 2, 8>> SgWaveShapes;
typedef WaveShapes<WaveShape<0, 2, 7>, WaveShape<4, 2, 7>, WaveShape<0, 3, 7>, WaveShape<4, 3, 7>, WaveShape<1, 2, 7>,
                   WaveShape<5, 2, 7>, WaveShape<2, 2, 7>, WaveShape<6, 2, 7>> GroupShapes;
// the slab with damping (4, 2, 8) is traced on whole waves by the fused deposition build alone
struct RecordingWaves { template <class S> static constexpr bool wave = !(S::EQ == 4 && S::NV == 8); };
// the variant builds: the unit-exponent kernels of a list
struct UnitExpWaves { template <class S> static constexpr bool wave = (S::EQ & 4) != 0 && RecordingWaves::wave<S>; };

template <int EQ, int NS, int G>
static int run_group(const rays::DevParams& D, const rays::TraceArgs& A, int resident_blocks) {
  typedef rays::GrpGeom<G> GEO;
  const int need = (A.nray + GEO::kRaysPerBlock - 1) / GEO::kRaysPerBlock;
  const int blocks = need < resident_blocks ? (need < 1 ? 1 : need) : resident_blocks;
  gridDim.x = (unsigned)blocks;
  blockDim.x = 256;
  std::vector<double> far((size_t)rays::sg_group_far_doubles_per_lane<G>() * 256 * (size_t)blocks, 0.0);
  rays::TraceArgs A2 = A;
  A2.sg_far = far.data();
  A2.sg_far_lanes = 256ll * blocks;
  for (int b = 0; b < blocks; b++) {
    blockIdx.x = (unsigned)b;
    for (int w = 0; w < 4; w++)
      wave_emul::run_wave(64u * (unsigned)w, [&] { rays::sg_group_kernel<EQ, NS, G>(D, A2); }, threadIdx);
  }
  return 0;
}
template <int EQ, int NS>
static int run_group_g(int G, const rays::DevParams& D, const rays::TraceArgs& A, int resident_blocks) {
  if (G == 4) return run_group<EQ, NS, 4>(D, A, resident_blocks);
  if (G == 8) return run_group<EQ, NS, 8>(D, A, resident_blocks);
  if (G == 16) return run_group<EQ, NS, 16>(D, A, resident_blocks);
  return 1;
}

// SG + ray_deriv_name = 'numerical', nv = 7 only.  resident_blocks: blocks launched (fewer than the fan needs:
// finished groups pull the remaining rays).
extern "C" int rays_emul_trace_group(const rays_params_t* p, int G, int resident_blocks, int nray, const double* rvec0,
                                     const double* rindex_vec0, double* ray_vec, double* residual, int32_t* npoints,
                                     int32_t* stop_code, double* end_ray_vec, double* end_residuals, double* max_residuals) {
  if (p->ode_solver != RAYS_ODE_SG || p->ray_deriv != RAYS_DERIV_NUM || p->nv != 7 || p->multi_spec_damping) return 1;
  unsigned counter = 0;
  const rays::TraceArgs A = emul_trace_args(nray, rvec0, rindex_vec0,
                                            EmulOut{ray_vec, residual, npoints, stop_code, nullptr, end_ray_vec,
                                                    end_residuals, max_residuals}, &counter);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAxisym)) return rc;
  return emul_wave_dispatch<AllShapes>(GroupShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_group_g<S::EQ, S::NS>(G, D, A, resident_blocks);
  });
}

// The one-ray-per-lane kernels on whole waves: `nwaves` blocks of one 64-lane wave each.  Fewer lanes than rays: lanes
// whose ray has ended are parked, written out and refilled by the wave's batched pass (rays_rk4_body.inc) -- the
// control flow a single emulated lane cannot exercise (its ballots have one bit).
static int g_rk4_w2_body = 0;  // run the body of the two-waves-per-SIMD build (one loop, index order, residual window)
template <int EQ, int NS, int NV>
static int run_rk4_waves(const rays::DevParams& D, const rays::TraceArgs& A, int nwaves) {
  // the continuation kernels (windowed tracing) have no two-waves-per-SIMD body and no hand-over
  constexpr bool kContinue = (EQ & rays::kEqContinue) != 0;
  gridDim.x = (unsigned)nwaves;
  blockDim.x = 64;
  for (int b = 0; b < nwaves; b++) {
    blockIdx.x = (unsigned)b;
    if constexpr (!kContinue) {
      if (g_rk4_w2_body) {
        wave_emul::run_wave(0u, [&] { rays::rk4_trace_kernel_w2<EQ, NS, 0, NV>(D, A); }, threadIdx);
        continue;
      }
    }
    wave_emul::run_wave(0u, [&] { rays::rk4_trace_kernel<EQ, NS, 0, NV>(D, A); }, threadIdx);
  }
  // what rays_capi.hip launches behind a tolerance kernel (this build hands ill-conditioned steps over like one:
  // emul_trace.cpp defines RAYS_EMUL_HANDOVER): rk4_resume_kernel for the rays that came back with the internal stop code
  if constexpr (!kContinue)
    for (int ray = 0; ray < A.nray; ray++)
      if (A.stop_code[ray] == rays::kStopResumeExact) rays::rk4_resume_ray<EQ, NS, 0, NV>(D, A, ray);
  return 0;
}
extern "C" void rays_emul_rk4_waves_use_w2_body(int on) { g_rk4_w2_body = on; }
// stride > 1: the "long rays first" hand-out order (rays_trace.hpp: take_rays) with that neighbourhood size
extern "C" int rays_emul_trace_rk4_waves(const rays_params_t* p, int nwaves, int stride, int nray, const double* rvec0,
                                         const double* rindex_vec0, double* ray_vec, double* residual, int32_t* npoints,
                                         int32_t* stop_code, double* end_ray_vec, double* end_residuals, double* max_residuals) {
  if (p->ode_solver != RAYS_ODE_RK4 || p->ray_deriv != RAYS_DERIV_COLD || p->multi_spec_damping || nwaves < 1) return 1;
  unsigned counter = 0;
  rays::TraceArgs A = emul_trace_args(nray, rvec0, rindex_vec0,
                                      EmulOut{ray_vec, residual, npoints, stop_code, nullptr, end_ray_vec, end_residuals,
                                              max_residuals}, &counter);
  std::vector<unsigned> sched;
  emul_sched(A, sched, stride);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  return emul_wave_dispatch<RecordingWaves>(Rk4WaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_rk4_waves<S::EQ, S::NS, S::NV>(D, A, nwaves);
  });
}

// The one-ray-per-lane Shampine-Gordon kernel (rays_sg.hpp: sg_trace_kernel) on `nwaves` blocks of one whole wave: the
// phase / interval votes with 64 lanes, rays that end on different trips, lanes that pull the next ray in index order.
template <int EQ, int NS, int NV>
static int run_sg_waves(const rays::DevParams& D, const rays::TraceArgs& A, int nwaves) {
  gridDim.x = (unsigned)nwaves;
  blockDim.x = 64;
  std::vector<double> far((size_t)rays::sg_far_doubles_per_lane<NV>() * 64 * (size_t)nwaves, 0.0);
  rays::TraceArgs A2 = A;
  A2.sg_far = far.data();
  A2.sg_far_lanes = 64ll * nwaves;
  for (int b = 0; b < nwaves; b++) {
    blockIdx.x = (unsigned)b;
    wave_emul::run_wave(0u, [&] { rays::sg_trace_kernel<EQ, NS, 0, NV>(D, A2); }, threadIdx);
  }
  return 0;
}
extern "C" int rays_emul_trace_sg_waves(const rays_params_t* p, int nwaves, int nray, const double* rvec0,
                                        const double* rindex_vec0, double* ray_vec, double* residual, int32_t* npoints,
                                        int32_t* stop_code, double* end_ray_vec, double* end_residuals, double* max_residuals) {
  if (p->ode_solver != RAYS_ODE_SG || p->ray_deriv != RAYS_DERIV_COLD || p->multi_spec_damping || nwaves < 1) return 1;
  unsigned counter = 0;
  const rays::TraceArgs A = emul_trace_args(nray, rvec0, rindex_vec0,
                                            EmulOut{ray_vec, residual, npoints, stop_code, nullptr, end_ray_vec,
                                                    end_residuals, max_residuals}, &counter);
  rays::DevParams D = make_dev_params(*p);
  if (int rc = emul_attach_tables(p, D, kTabAll)) return rc;
  return emul_wave_dispatch<AllShapes>(SgWaveShapes{}, p, [&](auto sh) {
    typedef decltype(sh) S;
    return run_sg_waves<S::EQ, S::NS, S::NV>(D, A, nwaves);
  });
}
