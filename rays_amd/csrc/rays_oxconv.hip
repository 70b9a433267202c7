// rays_oxconv.hip -- launchers and C ABI of the O-X mode conversion analysis (see rays_oxconv.hpp, rays_hip.h).
// A translation unit of its own (exact flags only: -ffp-contract=off, no RAYS_TOL_FLAVOUR); what it needs of
// rays_capi.hip's state comes through rays_capi_internal.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rays_capi_internal.hpp"
#include "rays_oxconv.hpp"

#ifdef RAYS_TOL_FLAVOUR
#error "the O-X conversion analysis exists in the exact arithmetic only"
#endif

namespace rays {

namespace {

template <int EQ, int NS>
hipError_t launch_ox(const DevParams& P, const OxArgs& A, hipStream_t s) {
  if (A.nray <= 0) return hipSuccess;
  const long long per_block = kOxScanBlock / kOxWave;
  const long long scan_blocks = ((long long)A.nray + per_block - 1) / per_block;
  const long long ascent_blocks = ((long long)A.nray + kOxAscentBlock - 1) / kOxAscentBlock;
  hipLaunchKernelGGL((ox_scan_kernel<EQ, NS>), dim3((unsigned)scan_blocks), dim3(kOxScanBlock), 0, s, P, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ox_ascent_kernel<EQ, NS>), dim3((unsigned)ascent_blocks), dim3(kOxAscentBlock), 0, s, P, A);
  return hipGetLastError();
}

// The shapes the library is built with: the (equilibrium | unit-exponent bit, species count) set of the per-point ray
// diagnostics (rays_diag.hip: kDiagEntries), i.e. of the trace kernels -- NS = 2 everywhere plus the species counts
// the fixtures reach in the default build, NS = 1..6 everywhere under make FULL=1, NS = 2 alone under make FAST=1.
struct OxEntry {
  int eq, ns;
  hipError_t (*launch)(const DevParams&, const OxArgs&, hipStream_t);
};
#define RAYS_OX_ENTRY(EQ, NS) {EQ, NS, &launch_ox<EQ, NS>}
#define RAYS_OX_ALL_EQ(NS) \
  RAYS_OX_ENTRY(0, NS), RAYS_OX_ENTRY(1, NS), RAYS_OX_ENTRY(2, NS), RAYS_OX_ENTRY(4, NS), RAYS_OX_ENTRY(5, NS), RAYS_OX_ENTRY(6, NS)
const OxEntry kOxEntries[] = {
    RAYS_OX_ALL_EQ(2),
#if defined(RAYS_INST_FAST)
#elif defined(RAYS_INST_FULL)
    RAYS_OX_ALL_EQ(1), RAYS_OX_ALL_EQ(3), RAYS_OX_ALL_EQ(4), RAYS_OX_ALL_EQ(5), RAYS_OX_ALL_EQ(6),
#else
    RAYS_OX_ENTRY(4, 1),  // gold_slab_ns1_rk4
    RAYS_OX_ENTRY(4, 3),  // gold_slab_shear_gauss_3spec_sg_num
    RAYS_OX_ENTRY(4, 6),  // gold_slab_6spec_sg
    RAYS_OX_ENTRY(5, 4),  // gold_solovev64_4spec_rk4_num
#endif
};

// the kernels' parameter block and the table entry of p's shape; an unbuilt shape is refused by name
int ox_prepare(const rays_params_t* p, DevParams* D, const OxEntry** entry) {
  bool ue = false;
  const int rc = capi_dev_params(p, D, &ue);
  if (rc) return rc;
  const int eq = p->equilib_model | (ue ? kEqUnitExp : 0);
  for (const OxEntry& e : kOxEntries)
    if (e.eq == eq && e.ns == p->nspec + 1) {
      *entry = &e;
      return 0;
    }
  char msg[256];
  std::snprintf(msg, sizeof msg, "rays_hip_ox_conv: no kernel built for this configuration (equilibrium %d, %s profile "
                "exponents, %d species): rebuild with `make -C rays_amd/csrc FULL=1` for every species count",
                p->equilib_model, ue ? "unit" : "general", p->nspec + 1);
  return capi_fail(msg);
}

int run_ox(const rays_params_t* p, int nray, int npt, bool packed, const double* d_ray_vec, const int32_t* d_npoints,
           const long long* d_offsets, const rays_ox_result_t& out, hipStream_t stream) {
  DevParams D;
  const OxEntry* e = nullptr;
  const int rc = ox_prepare(p, &D, &e);
  if (rc) return rc;
  if (nray == 0) return 0;
  void* ws = nullptr;
  const int wrc = capi_stream_workspace(stream, sizeof(int) * 2 * (size_t)nray, &ws);
  if (wrc) return wrc;
  OxArgs A;
  A.nray = nray; A.npt = npt; A.nv = p->nv; A.packed = packed ? 1 : 0;
  A.ray_vec = d_ray_vec; A.npoints = d_npoints; A.offsets = d_offsets;
  A.scan = static_cast<int*>(ws);
  A.out = out;
  const hipError_t he = e->launch(D, A, stream);
  if (he != hipSuccess) return capi_hip_fail(he, "O-X conversion kernels");
  return 0;
}

struct OxHostMath {  // the host's libm: what the reference binary calls
  static double acos_(double x) { return std::acos(x); }
  static double sin_(double x) { return std::sin(x); }
  static double cos_(double x) { return std::cos(x); }
  static double exp_(double x) { return std::exp(x); }
  static double pow_(double x, double y) { return std::pow(x, y); }
};

}  // namespace

}  // namespace rays

extern "C" {

int rays_hip_ox_conv_device(const rays_params_t* p, int nray, int in_layout, const double* d_ray_vec,
                            const int32_t* d_npoints, const int64_t* d_offsets, const rays_ox_result_t* out,
                            void* hip_stream) {
  using namespace rays;
  if (!p) return capi_fail("rays_hip: null parameter block");
  if (nray < 0) return capi_fail("rays_hip_ox_conv: bad nray");
  if (in_layout != RAYS_DIAG_IN_PADDED && in_layout != RAYS_DIAG_IN_PACKED) return capi_fail("rays_hip_ox_conv: unknown in_layout");
  if (!out) return capi_fail("rays_hip_ox_conv: null result block");
  if (p->nstep_max < 0) return capi_fail("rays_hip: nstep_max < 0");
  const bool packed = in_layout == RAYS_DIAG_IN_PACKED;
  if (nray > 0 && (!d_ray_vec || !d_npoints || (packed && !d_offsets))) return capi_fail("rays_hip_ox_conv: null device pointer");
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are 64-bit");
  return run_ox(p, nray, p->nstep_max + 1, packed, d_ray_vec, d_npoints, reinterpret_cast<const long long*>(d_offsets), *out,
                (hipStream_t)hip_stream);
}

const char* rays_hip_ox_conv_kernel_name_for(const rays_params_t* p) {
  using namespace rays;
  static thread_local char name[64];
  name[0] = 0;
  if (!p) {
    capi_fail("rays_hip: null parameter block");
    return name;
  }
  DevParams D;
  const OxEntry* e = nullptr;
  if (ox_prepare(p, &D, &e) == 0) std::snprintf(name, sizeof name, "ox_scan_kernel<%d, %d>", e->eq, e->ns);
  return name;
}

int rays_hip_ox_conv(const rays_params_t* p, int nray, const double* ray_vec, const int32_t* npoints,
                     const rays_ox_result_t* out, int32_t* number_of_rays_converted, int32_t* converted_ray_number) {
  using namespace rays;
  if (!p) return capi_fail("rays_hip: null parameter block");
  if (nray < 0) return capi_fail("rays_hip_ox_conv: bad nray");
  if (!out) return capi_fail("rays_hip_ox_conv: null result block");
  if (p->nstep_max < 0) return capi_fail("rays_hip: nstep_max < 0");
  if (number_of_rays_converted) *number_of_rays_converted = 0;
  if (nray == 0) return 0;
  if (!ray_vec || !npoints) return capi_fail("rays_hip_ox_conv: null array argument");
  const size_t nv = (size_t)p->nv, npt = (size_t)p->nstep_max + 1;
  for (int i = 0; i < nray; i++)
    if (npoints[i] < 0 || (size_t)npoints[i] > npt) return capi_fail("rays_hip_ox_conv: npoints outside 0 .. nstep_max + 1");
  // rays per block: at most 2**21 trajectory slots, or what the environment asks for
  long long block = std::max<long long>(1, (1ll << 21) / (long long)npt);
  if (const char* e = std::getenv("RAYS_HIP_OX_BLOCK_RAYS")) {
    const long long b = std::atoll(e);
    if (b > 0) block = b;
  }
  block = std::min<long long>(block, nray);
  // the block's device arrays, sized for its worst case (every slot recorded) and reused from block to block
  const size_t nb_max = (size_t)block;
  constexpr int kNDouble = 1 + 1 + 6 * 3 + RAYS_OX_NAUX;  // alpha_max, conv_coeff, six vectors, aux: doubles per ray
  double *d_rv = nullptr, *d_f = nullptr;
  int32_t *d_np = nullptr, *d_i = nullptr;
  long long* d_off = nullptr;
  auto release = [&]() {
    (void)hipFree(d_rv); (void)hipFree(d_f); (void)hipFree(d_np); (void)hipFree(d_i); (void)hipFree(d_off);
  };
#define OX_TRY(call)                                                     \
  do {                                                                   \
    hipError_t e_ = (call);                                              \
    if (e_ != hipSuccess) { release(); return capi_hip_fail(e_, #call); } \
  } while (0)
  OX_TRY(hipMalloc(&d_rv, sizeof(double) * nb_max * npt * nv));
  OX_TRY(hipMalloc(&d_f, sizeof(double) * nb_max * kNDouble));
  OX_TRY(hipMalloc(&d_np, sizeof(int32_t) * nb_max));
  OX_TRY(hipMalloc(&d_i, sizeof(int32_t) * nb_max * 3));
  OX_TRY(hipMalloc(&d_off, sizeof(long long) * (nb_max + 1)));
  std::vector<double> h_rv, h_f(nb_max * kNDouble);
  std::vector<int32_t> h_i(nb_max * 3);
  std::vector<long long> h_off(nb_max + 1);
  int32_t n_conv = 0;
  for (long long r0 = 0; r0 < nray; r0 += block) {
    const size_t nb = (size_t)std::min<long long>(block, nray - r0);
    long long total = 0;
    for (size_t i = 0; i < nb; i++) {
      h_off[i] = total;
      total += npoints[r0 + i];
    }
    h_off[nb] = total;
    h_rv.resize((size_t)total * nv);
    for (size_t i = 0; i < nb; i++)
      std::memcpy(h_rv.data() + (size_t)h_off[i] * nv, ray_vec + (size_t)(r0 + i) * npt * nv,
                  sizeof(double) * (size_t)npoints[r0 + i] * nv);
    if (total) OX_TRY(hipMemcpy(d_rv, h_rv.data(), sizeof(double) * h_rv.size(), hipMemcpyHostToDevice));
    OX_TRY(hipMemcpy(d_np, npoints + r0, sizeof(int32_t) * nb, hipMemcpyHostToDevice));
    OX_TRY(hipMemcpy(d_off, h_off.data(), sizeof(long long) * (nb + 1), hipMemcpyHostToDevice));
    // the block's result arrays, one after another in d_f / d_i
    rays_ox_result_t D;
    D.status = d_i; D.step_number = d_i + nb; D.iterations = d_i + 2 * nb;
    double* f = d_f;
    D.alpha_max = f; f += nb;
    D.conv_coeff = f; f += nb;
    D.x_max = f; f += 3 * nb;
    D.k_max = f; f += 3 * nb;
    D.x_cut = f; f += 3 * nb;
    D.nvecx_c = f; f += 3 * nb;
    D.nvecy_c = f; f += 3 * nb;
    D.nvecz_c = f; f += 3 * nb;
    D.aux = f;
    const int rc = run_ox(p, (int)nb, (int)npt, true, d_rv, d_np, d_off, D, nullptr);
    if (rc) { release(); return rc; }
    OX_TRY(hipMemcpy(h_f.data(), d_f, sizeof(double) * nb * kNDouble, hipMemcpyDeviceToHost));  // (waits for the kernels)
    OX_TRY(hipMemcpy(h_i.data(), d_i, sizeof(int32_t) * nb * 3, hipMemcpyDeviceToHost));
    int32_t* st = h_i.data();
    double* conv = h_f.data() + nb;
    const double* aux = h_f.data() + (2 + 6 * 3) * nb;
    for (size_t i = 0; i < nb; i++) {
      if (!(st[i] & RAYS_OX_FOUND_CUTOFF)) continue;
      // conv_coeff and the comparison with the threshold (:154) once more, with the libm the reference calls
      const double* a = aux + RAYS_OX_NAUX * i;
      conv[i] = ox_conv_value<OxHostMath>(a[RAYS_OX_AUX_COS_THETA], a[RAYS_OX_AUX_GAMMA], a[RAYS_OX_AUX_L], a[RAYS_OX_AUX_NY_C],
                                          a[RAYS_OX_AUX_NZ_C], p->k0);
      st[i] &= ~RAYS_OX_CONVERTED;
      if (conv[i] > kOxThreshold) st[i] |= RAYS_OX_CONVERTED;
    }
    for (size_t i = 0; i < nb; i++)
      if (st[i] & RAYS_OX_CONVERTED) {
        if (converted_ray_number) converted_ray_number[n_conv] = (int32_t)(r0 + i) + 1;
        n_conv++;
      }
    auto take_i = [&](int32_t* dst, size_t k) {
      if (dst) std::memcpy(dst + r0, h_i.data() + k * nb, sizeof(int32_t) * nb);
    };
    auto take_f = [&](double* dst, size_t first, size_t width) {
      if (dst) std::memcpy(dst + (size_t)r0 * width, h_f.data() + first * nb, sizeof(double) * nb * width);
    };
    take_i(out->status, 0); take_i(out->step_number, 1); take_i(out->iterations, 2);
    take_f(out->alpha_max, 0, 1); take_f(out->conv_coeff, 1, 1);
    take_f(out->x_max, 2, 3); take_f(out->k_max, 5, 3); take_f(out->x_cut, 8, 3);
    take_f(out->nvecx_c, 11, 3); take_f(out->nvecy_c, 14, 3); take_f(out->nvecz_c, 17, 3);
    take_f(out->aux, 20, RAYS_OX_NAUX);
  }
#undef OX_TRY
  release();
  if (number_of_rays_converted) *number_of_rays_converted = n_conv;
  return 0;
}

}  // extern "C"
