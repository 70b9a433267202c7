// rays_deposition.hip -- kernels of the device-side deposition profiles (see rays_deposition.hpp)
#include <hip/hip_runtime.h>

#include "rays_deposition.hpp"

namespace rays {

namespace {
constexpr int kDepWave = 64;

// one wave per block, one ray per lane; the ray's bins live in LDS (bin-major, lane-interleaved:
// conflict-free) while the binner walks the ray, then go to work[bin][ray] with coalesced stores
__global__ void __launch_bounds__(kDepWave) deposit_rays_kernel(const DevParams P, const DepArgs D) {
  extern __shared__ double rows[];  // [n_bins][64]
  typedef __attribute__((address_space(3))) double* lds_ptr;
  const int lane = threadIdx.x;
  const int iray = blockIdx.x * kDepWave + lane;
  if (iray >= D.nray) return;
  lds_ptr row = (lds_ptr)(rows + lane);
  deposit_ray(P, D, iray, row, kDepWave);
  for (int b = 0; b < D.n_bins; b++) D.work[(long long)b * D.nray + iray] = row[b * kDepWave];
}

// profile(b) = carry(b) + work(b, 1) + work(b, 2) + ... in ray order (sum(work, 2), continued).
// One wave per bin.  Each pass the lanes load U x 64 consecutive rays (coalesced); the running sum
// then takes them one by one: lane l of chunk u is ray base + 64 u + l.
__global__ void __launch_bounds__(kDepWave)
profile_sum_kernel(int n_bins, int nray, const double* __restrict__ work, const double* __restrict__ carry,
                   double* __restrict__ profile) {
  constexpr int U = 8;
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* w = work + (long long)b * nray;
  double s = carry ? carry[b] : 0.;
  for (int base = 0; base < nray; base += U * kDepWave) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int r = base + u * kDepWave + lane;
      v[u] = r < nray ? w[r] : 0.;  // + 0.0 is an exact no-op here (s is never -0.0)
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const unsigned lo = (unsigned)__double_as_longlong(v[u]);
      const unsigned hi = (unsigned)(__double_as_longlong(v[u]) >> 32);
#pragma unroll
      for (int l = 0; l < kDepWave; l++) {
        const unsigned a = __builtin_amdgcn_readlane(lo, l), c = __builtin_amdgcn_readlane(hi, l);
        s = s + __longlong_as_double((long long)(((unsigned long long)c << 32) | a));
      }
    }
  }
  if (lane == 0) profile[b] = s;
}

// The same sum per SEGMENT of rays (the runs of a fused ds scan, the beams of an aiming survey):
//   profile[s][b] = carry[s][b] + work[b][r0] + work[b][r0 + 1] + ... + work[b][r1 - 1],   r0 = off[s], r1 = off[s + 1]
// (off == nullptr: r0 = s * rays_per_seg, r1 = r0 + rays_per_seg), the adds in exactly that order and nothing else added:
// an empty segment gives carry[s][b], or +0.0 without a carry.  One wave per (segment, bin): blockIdx.x + seg0 is the
// segment, blockIdx.y + bin0 the bin.  The loads start at the segment's first ray, wherever it lies, and the last chunk
// walks only the lanes that hold rays of this segment, so it neither takes in the next segment's rays nor adds a padding
// +0.0 (which profile_sum_kernel does: there it shows only when the carry holds -0.0; for every other carry one segment
// [0, nray] gives that kernel's bits).  Every offset read is clamped to [0, nray] and r1 < r0 counts as empty, so no
// offset value makes the kernel read outside work.  carry == profile is allowed: each wave reads its one element first.
__global__ void __launch_bounds__(kDepWave)
profile_sum_segments_kernel(int n_bins, int nray, int seg0, int bin0, const int* __restrict__ off, int rays_per_seg,
                            const double* __restrict__ work, const double* carry, double* profile) {
  constexpr int U = 8;
  const int seg = seg0 + (int)blockIdx.x, b = bin0 + (int)blockIdx.y, lane = threadIdx.x;
  long long r0, r1;
  if (off) {
    r0 = off[seg];
    r1 = off[seg + 1];
  } else {
    r0 = (long long)seg * rays_per_seg;
    r1 = r0 + rays_per_seg;
  }
  r0 = r0 < 0 ? 0 : r0 > nray ? nray : r0;
  r1 = r1 < 0 ? 0 : r1 > nray ? nray : r1;
  if (r1 < r0) r1 = r0;
  const double* w = work + (long long)b * nray;
  const long long at = (long long)seg * n_bins + b;
  double s = carry ? carry[at] : 0.;
  for (long long base = r0; base < r1; base += U * kDepWave) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const long long r = base + u * kDepWave + lane;
      v[u] = r < r1 ? w[r] : 0.;  // (a lane past the segment's end is never read below)
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const long long left = r1 - (base + u * kDepWave);  // wave-uniform
      if (left <= 0) break;
      const unsigned lo = (unsigned)__double_as_longlong(v[u]);
      const unsigned hi = (unsigned)(__double_as_longlong(v[u]) >> 32);
      if (left >= kDepWave) {
#pragma unroll
        for (int l = 0; l < kDepWave; l++) {
          const unsigned a = __builtin_amdgcn_readlane(lo, l), c = __builtin_amdgcn_readlane(hi, l);
          s = s + __longlong_as_double((long long)(((unsigned long long)c << 32) | a));
        }
      } else {
        const int n = __builtin_amdgcn_readfirstlane((int)left);
        for (int l = 0; l < n; l++) {
          const unsigned a = __builtin_amdgcn_readlane(lo, l), c = __builtin_amdgcn_readlane(hi, l);
          s = s + __longlong_as_double((long long)(((unsigned long long)c << 32) | a));
        }
      }
    }
  }
  if (lane == 0) profile[at] = s;
}

// power_runs[r][i] = power[i], r = 0..n_runs-1: the per-ray weights of a fused ds scan, whose ray r * nray + i is fan
// member i (the fused kernels read the weight of a ray at the ray's own index)
constexpr int kTileBlock = 256;
__global__ void __launch_bounds__(kTileBlock)
tile_power_kernel(int nray, long long total, const double* __restrict__ power, double* __restrict__ power_runs) {
  for (long long i = (long long)blockIdx.x * kTileBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kTileBlock)
    power_runs[i] = power[i % nray];
}

// the DepTraceArgs block of a fused trace launch: a by-value kernel argument written to device memory in stream order
// (no host memory has to outlive the asynchronous call)
__global__ void __launch_bounds__(kDepWave) dep_trace_args_kernel(const DepTraceArgs T, DepTraceArgs* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = T;
}
// ... and the Dep2TraceArgs block of a two-profile launch
__global__ void __launch_bounds__(kDepWave) dep2_trace_args_kernel(const Dep2TraceArgs T, Dep2TraceArgs* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = T;
}
}  // namespace

hipError_t launch_dep2_trace_args(const Dep2TraceArgs& T, Dep2TraceArgs* d_out, hipStream_t s) {
  hipLaunchKernelGGL(dep2_trace_args_kernel, dim3(1), dim3(kDepWave), 0, s, T, d_out);
  return hipGetLastError();
}

hipError_t launch_dep_trace_args(const DepTraceArgs& T, DepTraceArgs* d_out, hipStream_t s) {
  hipLaunchKernelGGL(dep_trace_args_kernel, dim3(1), dim3(kDepWave), 0, s, T, d_out);
  return hipGetLastError();
}

// profile(b) = carry(b) + sum over the rays of work(b, :) in ray order (see profile_sum_kernel)
hipError_t launch_profile_sum(int n_bins, int nray, const double* work, const double* carry, double* profile,
                              hipStream_t s) {
  hipLaunchKernelGGL(profile_sum_kernel, dim3(n_bins), dim3(kDepWave), 0, s, n_bins, nray, work, carry, profile);
  return hipGetLastError();
}

// profile[s][b] = carry[s][b] + the sum over the rays of segment s of work(b, :) in ray order (see
// profile_sum_segments_kernel).  d_off: n_seg + 1 offsets on the device, or nullptr with a uniform rays_per_seg.
// The grid is cut so that neither dimension exceeds what a launch takes.
hipError_t launch_profile_sum_segments(int n_bins, int nray, int n_seg, const int* d_off, int rays_per_seg,
                                       const double* work, const double* carry, double* profile, hipStream_t s) {
  constexpr int kSegChunk = 1 << 20, kBinChunk = 65535;
  for (int seg0 = 0; seg0 < n_seg; seg0 += kSegChunk)
    for (int bin0 = 0; bin0 < n_bins; bin0 += kBinChunk) {
      const int ns = n_seg - seg0 < kSegChunk ? n_seg - seg0 : kSegChunk;
      const int nb = n_bins - bin0 < kBinChunk ? n_bins - bin0 : kBinChunk;
      hipLaunchKernelGGL(profile_sum_segments_kernel, dim3(ns, nb), dim3(kDepWave), 0, s, n_bins, nray, seg0, bin0, d_off,
                         rays_per_seg, work, carry, profile);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

// power_runs[n_runs][nray] = power[nray] tiled, in stream order (see tile_power_kernel)
hipError_t launch_tile_power(int nray, long long total, const double* power, double* power_runs, hipStream_t s) {
  if (total <= 0 || nray <= 0) return hipSuccess;
  const long long want = (total + kTileBlock - 1) / kTileBlock;
  hipLaunchKernelGGL(tile_power_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(kTileBlock), 0, s, nray, total,
                     power, power_runs);
  return hipGetLastError();
}

hipError_t launch_deposition(const DevParams& P, const DepArgs& D, const double* carry, double* profile,
                             hipStream_t s) {
  const size_t lds = sizeof(double) * (size_t)D.n_bins * kDepWave;
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  static thread_local int attr_dev = -1;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev != attr_dev) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(deposit_rays_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_dev = dev;
  }
  if (D.nray > 0) {
    hipLaunchKernelGGL(deposit_rays_kernel, dim3((D.nray + kDepWave - 1) / kDepWave), dim3(kDepWave), lds, s, P, D);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(profile_sum_kernel, dim3(D.n_bins), dim3(kDepWave), 0, s, D.n_bins, D.nray, D.work, carry, profile);
  return hipGetLastError();
}

}  // namespace rays
