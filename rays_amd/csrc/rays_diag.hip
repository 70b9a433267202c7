// rays_diag.hip -- kernel, launcher and C ABI of the per-point ray diagnostics (see rays_diag.hpp, rays_hip.h).
// A translation unit of its own (exact flags only: -ffp-contract=off, no RAYS_TOL_FLAVOUR); what it needs of
// rays_capi.hip's state comes through rays_capi_internal.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rays_capi_internal.hpp"
#include "rays_diag.hpp"

#ifdef RAYS_TOL_FLAVOUR
#error "the ray diagnostics exist in the exact arithmetic only"
#endif

namespace rays {

namespace {
constexpr int kDiagWave = 64;
constexpr int kDiagBlock = 256;  // four independent waves

// Mapping: one wave per run of 64 consecutive points of ONE ray (chunk c of ray i: points 64 c .. 64 c + 63), one lane
// per point, so every selected field is stored as one contiguous 512-byte run per wave and the wave's nv-double rows
// are one contiguous span of ray_vec.  The span is read with coalesced loads (consecutive lanes, consecutive doubles)
// into LDS and each lane then takes its own row from there: a lane reading its row straight from global memory would
// touch 64 different 56 .. 152-byte pieces per load instruction.  Rows are padded to an odd number of doubles, so the
// 64 lanes' ds_read_b64 of one column fall on distinct bank pairs.
// A chunk that lies wholly past npoints(iray) does no arithmetic and reads nothing but npoints: in the padded layout
// it writes the +0.0 the reference's allocate(..., source = 0) leaves there (each output slot is written exactly once,
// no memset pass before the kernel); in the packed layout it has nothing to do.
template <int EQ, int NS>
__global__ void __launch_bounds__(kDiagBlock) ray_diag_kernel(const DevParams P, const DiagArgs A) {
  extern __shared__ double stage[];  // [4 waves][64 rows][nv | 1]
  const int lane = threadIdx.x & (kDiagWave - 1), wave = threadIdx.x / kDiagWave;
  const int cpr = (A.npt + kDiagWave - 1) / kDiagWave;  // chunks per ray
  const long long w = (long long)blockIdx.x * (kDiagBlock / kDiagWave) + wave;
  const bool have = w < (long long)A.nray * cpr;  // (no early return: the block meets at the barrier below)
  const int iray = have ? (int)(w / cpr) : 0;
  const int p0 = have ? (int)(w - (long long)iray * cpr) * kDiagWave : 0;
  int np = have ? A.npoints[iray] : 0;
  np = np < A.npt ? np : A.npt;  // (never beyond the arrays, whatever npoints holds)
  const int rows = np - p0 < kDiagWave ? np - p0 : kDiagWave;  // recorded points of this chunk (<= 0: none)
  const int rowpad = A.nv | 1;
  double* st = stage + (size_t)wave * kDiagWave * rowpad;
  const long long first = A.offsets ? A.offsets[iray] + p0 : (long long)iray * A.npt + p0;  // the chunk's first point
  if (rows > 0) {
    const double* __restrict__ src = A.ray_vec + first * A.nv;
    const int n = rows * A.nv;
    int r = lane / A.nv, c = lane - r * A.nv;  // element i = lane + 64 j is column c of row r
    const int dr = kDiagWave / A.nv, dc = kDiagWave - dr * A.nv;
    for (int i = lane; i < n; i += kDiagWave) {
      st[r * rowpad + c] = src[i];
      r += dr;
      c += dc;
      if (c >= A.nv) {
        c -= A.nv;
        r++;
      }
    }
  }
  __syncthreads();
  const int ip = p0 + lane;
  if (!have || ip >= A.npt) return;
  const bool live = lane < rows;
  if (rows <= 0 && A.offsets) return;
  double out[RAYS_DIAG_NFIELDS];
#pragma unroll
  for (int f = 0; f < RAYS_DIAG_NFIELDS; f++) out[f] = 0.;
  if (live) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 7; i++) v[i] = st[lane * rowpad + i];
    v[7] = A.nv > 7 ? st[lane * rowpad + 7] : 0.;
    const double resid = A.residual[first + lane];
    const bool bad = diag_point<EQ, NS>(P, v, resid, A.fields, out);
    if (RAYS_RARE(bad) && A.first_bad) {  // the smallest 1-based index of the ray (0 = none so far)
      const int idx = ip + 1;
      int old = *(volatile int*)&A.first_bad[iray];
      while (old == 0 || old > idx) {
        const int prev = atomicCAS(&A.first_bad[iray], old, idx);
        if (prev == old) break;
        old = prev;
      }
    }
  } else if (A.offsets) {
    return;  // packed layout: no slot past npoints exists
  }
  double* __restrict__ dst = A.out + first + lane;
#pragma unroll
  for (int f = 0; f < RAYS_DIAG_NFIELDS; f++)
    if (A.fields & (1u << f)) {  // wave-uniform
      *dst = out[f];
      dst += A.out_stride;
    }
}

template <int EQ, int NS>
hipError_t launch_diag(const DevParams& P, const DiagArgs& A, hipStream_t s) {
  const long long cpr = (A.npt + kDiagWave - 1) / kDiagWave;
  const long long waves = (long long)A.nray * cpr, per_block = kDiagBlock / kDiagWave;
  const long long blocks = (waves + per_block - 1) / per_block;
  if (blocks <= 0) return hipSuccess;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t lds = sizeof(double) * per_block * kDiagWave * (size_t)(A.nv | 1);
  hipLaunchKernelGGL((ray_diag_kernel<EQ, NS>), dim3((unsigned)blocks), dim3(kDiagBlock), lds, s, P, A);
  return hipGetLastError();
}

// The packed form (rays_diag.hpp: DiagPackedArgs): one wave per 64 consecutive PACKED points -- flat indices 64 w ..
// 64 w + 63, whatever rays they belong to --, so the launched work follows the recorded points, every lane but the last
// wave's tail is live, each selected field is one contiguous 512-byte store per wave and no lane writes a zero.  The
// grid covers `capacity`, the bound the host knows; a wave at or beyond offsets[nray] reads that one value and leaves.
// Packed input: the wave's 64 nv doubles are one contiguous span, staged exactly as above; no ray identity is needed.
// Padded input: the wave's first ray comes from one bisection of `offsets` (wave-uniform, scalar loads), each lane
// settles its own ray from there (diag_locate_from) and hands the start of its row to the lanes that stage it, so the
// loads stay coalesced inside every ray's run.  first_bad needs the ray in either layout, on the rare bad point only.
template <int EQ, int NS>
__global__ void __launch_bounds__(kDiagBlock) ray_diag_packed_kernel(const DevParams P, const DiagPackedArgs A) {
  extern __shared__ double stage[];  // [4 waves][64 rows][nv | 1]
  const int lane = threadIdx.x & (kDiagWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kDiagWave);
  const long long base = ((long long)blockIdx.x * (kDiagBlock / kDiagWave) + wave) * kDiagWave;
  long long limit = A.offsets[A.nray];  // the recorded points
  limit = limit < A.capacity ? limit : A.capacity;
  const long long left = limit - base;  // (no early return: the block meets at the barrier below)
  const int rows = left >= kDiagWave ? kDiagWave : left > 0 ? (int)left : 0;
  const int rowpad = A.nv | 1;
  double* st = stage + (size_t)wave * kDiagWave * rowpad;
  const long long j = base + lane;
  bool live = lane < rows;
  long long row = j;  // the lane's row of ray_vec = its element of residual
  int iray = 0, ip = 0;
  if (rows > 0) {
    if (!A.in_packed) {
      row = 0;
      if (live) {
        iray = diag_locate_from(A.offsets, A.nray, diag_locate(A.offsets, A.nray, base), j);
        const long long pt = j - A.offsets[iray];
        int np = A.npoints[iray];
        np = np < A.npt ? np : A.npt;
        live = pt >= 0 && pt < np;  // (never beyond the arrays, whatever npoints and offsets hold)
        ip = (int)pt;
        if (live) row = (long long)iray * A.npt + pt;
      }
    }
    const int n = rows * A.nv;
    int r = lane / A.nv, c = lane - r * A.nv;  // element i = lane + 64 k is column c of row r
    const int dr = kDiagWave / A.nv, dc = kDiagWave - dr * A.nv;
    for (int k = 0; k < A.nv; k++) {  // (the same trip count in every lane: the shuffle reads live lanes only)
      const long long from = A.in_packed ? base + r : __shfl(row, r);
      if (lane + kDiagWave * k < n) st[r * rowpad + c] = A.ray_vec[from * A.nv + c];
      r += dr;
      c += dc;
      if (c >= A.nv) {
        c -= A.nv;
        r++;
      }
    }
  }
  __syncthreads();
  if (!live) return;
  double out[RAYS_DIAG_NFIELDS];
#pragma unroll
  for (int f = 0; f < RAYS_DIAG_NFIELDS; f++) out[f] = 0.;
  double v[8];
#pragma unroll
  for (int i = 0; i < 7; i++) v[i] = st[lane * rowpad + i];
  v[7] = A.nv > 7 ? st[lane * rowpad + 7] : 0.;
  const bool bad = diag_point<EQ, NS>(P, v, A.residual[row], A.fields, out);
  if (RAYS_RARE(bad) && A.first_bad) {  // the smallest 1-based index of the ray (0 = none so far)
    if (A.in_packed) {
      iray = diag_locate(A.offsets, A.nray, j);
      ip = (int)(j - A.offsets[iray]);
    }
    const int idx = ip + 1;
    int old = *(volatile int*)&A.first_bad[iray];
    while (old == 0 || old > idx) {
      const int prev = atomicCAS(&A.first_bad[iray], old, idx);
      if (prev == old) break;
      old = prev;
    }
  }
  double* __restrict__ dst = A.out + j;  // j < limit <= capacity <= out_stride
#pragma unroll
  for (int f = 0; f < RAYS_DIAG_NFIELDS; f++)
    if (A.fields & (1u << f)) {  // wave-uniform
      *dst = out[f];
      dst += A.out_stride;
    }
}

template <int EQ, int NS>
hipError_t launch_diag_packed(const DevParams& P, const DiagPackedArgs& A, hipStream_t s) {
  const long long waves = (A.capacity + kDiagWave - 1) / kDiagWave, per_block = kDiagBlock / kDiagWave;
  const long long blocks = (waves + per_block - 1) / per_block;
  if (blocks <= 0) return hipSuccess;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  const size_t lds = sizeof(double) * per_block * kDiagWave * (size_t)(A.nv | 1);
  hipLaunchKernelGGL((ray_diag_packed_kernel<EQ, NS>), dim3((unsigned)blocks), dim3(kDiagBlock), lds, s, P, A);
  return hipGetLastError();
}

// ---- point offsets: the exclusive prefix sum of clamp(npoints, 0, npt) in offsets[0 .. nray], in three passes that
// need no memory but `offsets` itself.  Integer sums: exact, whatever the order.
//   1. every tile of 2048 rays writes its own running sums: offsets[i + 1] = the tile's counts up to ray i, so that
//      the tile's last entry (offsets[end of the tile]) is the tile's total;
//   2. one block turns those last entries into their running sum over the tiles: they are final;
//   3. every tile but the first adds the entry in front of it (final since 2) to its other entries.
constexpr int kScanBlock = 256, kScanItems = 8, kScanTile = kScanBlock * kScanItems;

// running sum of x over the block's threads in thread order, this thread's x included; *all = the block's sum
__device__ long long scan_block(long long x, long long* wsum, long long* all) {
  const int lane = threadIdx.x & (kDiagWave - 1), wave = threadIdx.x / kDiagWave;
  for (int d = 1; d < kDiagWave; d += d) {
    const long long y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == kDiagWave - 1) wsum[wave] = x;
  __syncthreads();
  long long sum = 0;
  for (int w = 0; w < kScanBlock / kDiagWave; w++) {
    if (w < wave) x += wsum[w];
    sum += wsum[w];
  }
  *all = sum;
  __syncthreads();  // (wsum is free again)
  return x;
}

__global__ void __launch_bounds__(kScanBlock) offsets_tile_kernel(int nray, int npt, const int* __restrict__ npoints,
                                                                  long long* __restrict__ offsets) {
  __shared__ long long wsum[kScanBlock / kDiagWave];
  if (blockIdx.x == 0 && threadIdx.x == 0) offsets[0] = 0;
  long long carry = 0;
  for (int k = 0; k < kScanItems; k++) {
    const long long i = (long long)blockIdx.x * kScanTile + k * kScanBlock + threadIdx.x;
    long long x = 0, all;
    if (i < nray) {
      const int n = npoints[i];
      x = n < 0 ? 0 : n > npt ? npt : n;
    }
    x = scan_block(x, wsum, &all);
    if (i < nray) offsets[i + 1] = carry + x;
    carry += all;
  }
}

__global__ void __launch_bounds__(kScanBlock) offsets_totals_kernel(int nray, long long ntiles, long long* offsets) {
  __shared__ long long wsum[kScanBlock / kDiagWave];
  long long carry = 0;
  for (long long t0 = 0; t0 < ntiles; t0 += kScanBlock) {
    const long long t = t0 + threadIdx.x;
    long long end = (t + 1) * kScanTile, x = 0, all;
    end = end < nray ? end : nray;
    if (t < ntiles) x = offsets[end];
    x = scan_block(x, wsum, &all);
    if (t < ntiles) offsets[end] = carry + x;
    carry += all;
  }
}

__global__ void __launch_bounds__(kScanBlock) offsets_add_kernel(int nray, long long* offsets) {
  const long long first = ((long long)blockIdx.x + 1) * kScanTile;  // tile blockIdx.x + 1: entries first + 1 .. end - 1
  long long end = first + kScanTile;
  end = end < nray ? end : nray;
  const long long add = offsets[first];
  for (long long i = first + 1 + threadIdx.x; i < end; i += kScanBlock) offsets[i] += add;
}

// The shapes the library is built with: the (equilibrium | unit-exponent bit, species count) set of the trace kernels
// (rays_inst.hip) -- NS = 2 everywhere plus the species counts the fixtures reach in the default build, NS = 1..6
// everywhere under make FULL=1, NS = 2 alone in the developer build (make FAST=1).
struct DiagEntry {
  int eq, ns;
  hipError_t (*launch)(const DevParams&, const DiagArgs&, hipStream_t);
  hipError_t (*launch_packed)(const DevParams&, const DiagPackedArgs&, hipStream_t);
};
#define RAYS_DIAG_ENTRY(EQ, NS) {EQ, NS, &launch_diag<EQ, NS>, &launch_diag_packed<EQ, NS>}
#define RAYS_DIAG_ALL_EQ(NS) \
  RAYS_DIAG_ENTRY(0, NS), RAYS_DIAG_ENTRY(1, NS), RAYS_DIAG_ENTRY(2, NS), RAYS_DIAG_ENTRY(4, NS), RAYS_DIAG_ENTRY(5, NS), \
      RAYS_DIAG_ENTRY(6, NS)
const DiagEntry kDiagEntries[] = {
    RAYS_DIAG_ALL_EQ(2),
#if defined(RAYS_INST_FAST)
#elif defined(RAYS_INST_FULL)
    RAYS_DIAG_ALL_EQ(1), RAYS_DIAG_ALL_EQ(3), RAYS_DIAG_ALL_EQ(4), RAYS_DIAG_ALL_EQ(5), RAYS_DIAG_ALL_EQ(6),
#else
    RAYS_DIAG_ENTRY(4, 1),  // gold_slab_ns1_rk4
    RAYS_DIAG_ENTRY(4, 3),  // gold_slab_shear_gauss_3spec_sg_num
    RAYS_DIAG_ENTRY(4, 6),  // gold_slab_6spec_sg
    RAYS_DIAG_ENTRY(5, 4),  // gold_solovev64_4spec_rk4_num
#endif
};

const DiagEntry* find_diag(int eq, int ns) {
  for (const DiagEntry& e : kDiagEntries)
    if (e.eq == eq && e.ns == ns) return &e;
  return nullptr;
}

int count_bits(unsigned x) {
  int n = 0;
  for (; x; x &= x - 1) n++;
  return n;
}

// what every entry point needs before its launch: the kernels' parameter block and the table entry of p's shape
int diag_prepare(const rays_params_t* p, DevParams* D, const DiagEntry** entry) {
  bool ue = false;
  int rc = capi_dev_params(p, D, &ue);
  if (rc) return rc;
  const int eq = p->equilib_model | (ue ? kEqUnitExp : 0);
  const DiagEntry* e = find_diag(eq, p->nspec + 1);
  if (!e) {
    char msg[256];
    std::snprintf(msg, sizeof msg, "rays_hip_ray_diagnostics: no kernel built for this configuration (equilibrium %d, "
                  "%s profile exponents, %d species): rebuild with `make -C rays_amd/csrc FULL=1` for every species count",
                  p->equilib_model, ue ? "unit" : "general", p->nspec + 1);
    return capi_fail(msg);
  }
  *entry = e;
  return 0;
}

// checks shared by the two entry points + the launch.  `offsets` / `total`: the packed layout (DiagArgs).
int run_diag(const rays_params_t* p, int nray, int npt, const double* d_ray_vec, const double* d_residual,
             const int32_t* d_npoints, const long long* d_offsets, long long total, uint32_t fields, double* d_out,
             int32_t* d_first_bad, hipStream_t stream) {
  DevParams D;
  const DiagEntry* e = nullptr;
  const int rc = diag_prepare(p, &D, &e);
  if (rc) return rc;
  if (d_first_bad) {
    hipError_t he = hipMemsetAsync(d_first_bad, 0, sizeof(int32_t) * (size_t)nray, stream);
    if (he != hipSuccess) return capi_hip_fail(he, "hipMemsetAsync(first_bad_point)");
  }
  DiagArgs A;
  A.nray = nray; A.npt = npt; A.nv = p->nv; A.fields = fields;
  A.ray_vec = d_ray_vec; A.residual = d_residual; A.npoints = d_npoints; A.offsets = d_offsets;
  A.out_stride = d_offsets ? total : (long long)nray * npt;
  A.out = d_out; A.first_bad = d_first_bad;
  const hipError_t he = e->launch(D, A, stream);
  if (he != hipSuccess) return capi_hip_fail(he, "ray diagnostics kernel");
  return 0;
}
}  // namespace

}  // namespace rays

extern "C" {

int rays_hip_ray_diagnostics_device(const rays_params_t* p, int nray, const double* d_ray_vec,
                                    const double* d_residual, const int32_t* d_npoints, uint32_t fields,
                                    double* d_out, int32_t* d_first_bad_point, void* hip_stream) {
  using namespace rays;
  if (!p) return capi_fail("rays_hip: null parameter block");
  if (nray < 0) return capi_fail("rays_hip_ray_diagnostics: bad nray");
  if (fields == 0 || (fields & ~kDiagAllFields)) return capi_fail("rays_hip_ray_diagnostics: `fields` selects no field or an unknown one");
  if (nray > 0 && (!d_ray_vec || !d_residual || !d_npoints || !d_out))
    return capi_fail("rays_hip_ray_diagnostics: null device pointer");
  if (p->nstep_max < 0) return capi_fail("rays_hip: nstep_max < 0");
  return run_diag(p, nray, p->nstep_max + 1, d_ray_vec, d_residual, d_npoints, nullptr, 0, fields, d_out,
                  d_first_bad_point, (hipStream_t)hip_stream);
}

int rays_hip_point_offsets_device(int nray, int nstep_max, const int32_t* d_npoints, int64_t* d_offsets,
                                  void* hip_stream) {
  using namespace rays;
  if (nray < 0) return capi_fail("rays_hip_point_offsets: bad nray");
  if (nstep_max < 0) return capi_fail("rays_hip: nstep_max < 0");
  if (!d_offsets || (nray > 0 && !d_npoints)) return capi_fail("rays_hip_point_offsets: null device pointer");
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are 64-bit");
  long long* off = reinterpret_cast<long long*>(d_offsets);
  hipStream_t s = (hipStream_t)hip_stream;
  const long long ntiles = ((long long)nray + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(offsets_tile_kernel, dim3((unsigned)std::max<long long>(ntiles, 1)), dim3(kScanBlock), 0, s, nray,
                     nstep_max + 1, d_npoints, off);
  if (ntiles > 1) {
    hipLaunchKernelGGL(offsets_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, nray, ntiles, off);
    hipLaunchKernelGGL(offsets_add_kernel, dim3((unsigned)(ntiles - 1)), dim3(kScanBlock), 0, s, nray, off);
  }
  const hipError_t he = hipGetLastError();
  if (he != hipSuccess) return capi_hip_fail(he, "point offsets kernels");
  return 0;
}

int rays_hip_ray_diagnostics_packed_device(const rays_params_t* p, int nray, int in_layout, const double* d_ray_vec,
                                           const double* d_residual, const int32_t* d_npoints, const int64_t* d_offsets,
                                           int64_t out_stride, uint32_t fields, double* d_out,
                                           int32_t* d_first_bad_point, void* hip_stream) {
  using namespace rays;
  if (!p) return capi_fail("rays_hip: null parameter block");
  if (nray < 0) return capi_fail("rays_hip_ray_diagnostics: bad nray");
  if (fields == 0 || (fields & ~kDiagAllFields)) return capi_fail("rays_hip_ray_diagnostics: `fields` selects no field or an unknown one");
  if (in_layout != RAYS_DIAG_IN_PADDED && in_layout != RAYS_DIAG_IN_PACKED)
    return capi_fail("rays_hip_ray_diagnostics: unknown in_layout");
  if (out_stride < 0) return capi_fail("rays_hip_ray_diagnostics: out_stride < 0");
  if (nray > 0 && (!d_ray_vec || !d_residual || !d_npoints || !d_offsets || !d_out))
    return capi_fail("rays_hip_ray_diagnostics: null device pointer");
  if (p->nstep_max < 0) return capi_fail("rays_hip: nstep_max < 0");
  hipStream_t stream = (hipStream_t)hip_stream;
  DevParams D;
  const DiagEntry* e = nullptr;
  const int rc = diag_prepare(p, &D, &e);
  if (rc) return rc;
  if (d_first_bad_point && nray > 0) {
    hipError_t he = hipMemsetAsync(d_first_bad_point, 0, sizeof(int32_t) * (size_t)nray, stream);
    if (he != hipSuccess) return capi_hip_fail(he, "hipMemsetAsync(first_bad_point)");
  }
  DiagPackedArgs A;
  A.nray = nray; A.npt = p->nstep_max + 1; A.nv = p->nv; A.in_packed = in_layout == RAYS_DIAG_IN_PACKED;
  A.fields = fields;
  A.ray_vec = d_ray_vec; A.residual = d_residual; A.npoints = d_npoints;
  A.offsets = reinterpret_cast<const long long*>(d_offsets);
  A.out_stride = out_stride;
  A.capacity = std::min<long long>(out_stride, (long long)nray * A.npt);  // no ray holds more than npt points
  A.out = d_out; A.first_bad = d_first_bad_point;
  const hipError_t he = e->launch_packed(D, A, stream);
  if (he != hipSuccess) return capi_hip_fail(he, "packed ray diagnostics kernel");
  return 0;
}

int rays_hip_ray_diagnostics(const rays_params_t* p, int nray, const double* ray_vec, const double* residual,
                             const int32_t* npoints, uint32_t fields, double* out, int32_t* first_bad_point) {
  using namespace rays;
  if (!p) return capi_fail("rays_hip: null parameter block");
  if (nray < 0) return capi_fail("rays_hip_ray_diagnostics: bad nray");
  if (fields == 0 || (fields & ~kDiagAllFields)) return capi_fail("rays_hip_ray_diagnostics: `fields` selects no field or an unknown one");
  if (p->nstep_max < 0) return capi_fail("rays_hip: nstep_max < 0");
  if (nray == 0) return 0;
  if (!ray_vec || !residual || !npoints || !out) return capi_fail("rays_hip_ray_diagnostics: null array argument");
  const size_t nv = (size_t)p->nv, npt = (size_t)p->nstep_max + 1;
  const int nsel = count_bits(fields);
  for (int i = 0; i < nray; i++)
    if (npoints[i] < 0 || (size_t)npoints[i] > npt) return capi_fail("rays_hip_ray_diagnostics: npoints outside 0 .. nstep_max + 1");
  // rays per block: at most 2**21 trajectory slots, or what the environment asks for
  long long block = std::max<long long>(1, (1ll << 21) / (long long)npt);
  if (const char* e = std::getenv("RAYS_HIP_DIAG_BLOCK_RAYS")) {
    const long long b = std::atoll(e);
    if (b > 0) block = b;
  }
  block = std::min<long long>(block, nray);
  // the block's device arrays, sized for its worst case (every slot recorded) and reused from block to block
  const size_t cap = (size_t)block * npt;
  double *d_rv = nullptr, *d_res = nullptr, *d_out = nullptr;
  int32_t *d_np = nullptr, *d_bad = nullptr;
  long long* d_off = nullptr;
  auto release = [&]() {
    (void)hipFree(d_rv); (void)hipFree(d_res); (void)hipFree(d_out); (void)hipFree(d_np); (void)hipFree(d_bad); (void)hipFree(d_off);
  };
#define DIAG_TRY(call)                                                    \
  do {                                                                    \
    hipError_t e_ = (call);                                               \
    if (e_ != hipSuccess) { release(); return capi_hip_fail(e_, #call); } \
  } while (0)
  DIAG_TRY(hipMalloc(&d_rv, sizeof(double) * cap * nv));
  DIAG_TRY(hipMalloc(&d_res, sizeof(double) * cap));
  DIAG_TRY(hipMalloc(&d_out, sizeof(double) * cap * (size_t)nsel));
  DIAG_TRY(hipMalloc(&d_np, sizeof(int32_t) * (size_t)block));
  DIAG_TRY(hipMalloc(&d_bad, sizeof(int32_t) * (size_t)block));
  DIAG_TRY(hipMalloc(&d_off, sizeof(long long) * (size_t)block));
  std::vector<double> h_rv, h_res, h_out;
  std::vector<long long> h_off((size_t)block);
  const size_t field_stride = (size_t)nray * npt;
  for (long long r0 = 0; r0 < nray; r0 += block) {
    const int nb = (int)std::min<long long>(block, nray - r0);
    long long total = 0;
    int maxnp = 0;
    for (int i = 0; i < nb; i++) {
      h_off[i] = total;
      total += npoints[r0 + i];
      maxnp = std::max(maxnp, (int)npoints[r0 + i]);
    }
    // the reference's arrays are zero wherever no point was recorded
    for (int k = 0; k < nsel; k++)
      for (int i = 0; i < nb; i++) {
        const size_t np = (size_t)npoints[r0 + i];
        std::memset(out + k * field_stride + (size_t)(r0 + i) * npt + np, 0, sizeof(double) * (npt - np));
      }
    if (first_bad_point) std::memset(first_bad_point + r0, 0, sizeof(int32_t) * (size_t)nb);
    if (total == 0) continue;
    h_rv.resize((size_t)total * nv);
    h_res.resize((size_t)total);
    h_out.resize((size_t)total * nsel);
    for (int i = 0; i < nb; i++) {
      const size_t np = (size_t)npoints[r0 + i];
      std::memcpy(h_rv.data() + (size_t)h_off[i] * nv, ray_vec + (size_t)(r0 + i) * npt * nv, sizeof(double) * np * nv);
      std::memcpy(h_res.data() + (size_t)h_off[i], residual + (size_t)(r0 + i) * npt, sizeof(double) * np);
    }
    DIAG_TRY(hipMemcpy(d_rv, h_rv.data(), sizeof(double) * h_rv.size(), hipMemcpyHostToDevice));
    DIAG_TRY(hipMemcpy(d_res, h_res.data(), sizeof(double) * h_res.size(), hipMemcpyHostToDevice));
    DIAG_TRY(hipMemcpy(d_np, npoints + r0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice));
    DIAG_TRY(hipMemcpy(d_off, h_off.data(), sizeof(long long) * (size_t)nb, hipMemcpyHostToDevice));
    const int rc = run_diag(p, nb, maxnp, d_rv, d_res, d_np, d_off, total, fields, d_out, first_bad_point ? d_bad : nullptr,
                            nullptr);
    if (rc) { release(); return rc; }
    DIAG_TRY(hipMemcpy(h_out.data(), d_out, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost));  // (waits for the kernel)
    if (first_bad_point)
      DIAG_TRY(hipMemcpy(first_bad_point + r0, d_bad, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost));
    for (int k = 0; k < nsel; k++)
      for (int i = 0; i < nb; i++)
        std::memcpy(out + k * field_stride + (size_t)(r0 + i) * npt, h_out.data() + (size_t)k * total + h_off[i],
                    sizeof(double) * (size_t)npoints[r0 + i]);
  }
#undef DIAG_TRY
  release();
  return 0;
}

}  // extern "C"
