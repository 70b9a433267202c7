// rays_capi.hip -- the C ABI of librays_hip.so (include/rays_hip.h).
//
// Host side of the drop-in boundary for `call trace_rays` (RAYS_project/RAYS_lib/ray_tracing.f90).
// No oracle, no CPU fallback: every entry point either runs the HIP kernels or fails with an
// error message.
//
// Every device resource behind these entries has one owner in rays_capi_resources.hpp -- the workspaces per (device,
// stream), the tables' device copies, the block cache, the buffers of one call -- and rays_hip_finalize releases them
// all; an entry that fails returns at once and its DeviceBuffers gives the call's blocks back.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rays_hip.h"
#include "rays_launch.hpp"
#include "rays_ray_init.hpp"
#include "rays_deposition.hpp"
#include "rays_capi_internal.hpp"
#include "rays_capi_resources.hpp"

namespace rays {
// The kernel groups linked into this library (rays_launch.hpp: KernelGroup).  The head is a plain pointer with a constant
// initialiser, so it is in place before any object's static initialiser registers, whatever their order.
KernelGroup* g_kernel_groups = nullptr;
void register_kernel_group(KernelGroup* g) {
  g->next = g_kernel_groups;
  g_kernel_groups = g;
}
hipError_t launch_pack(bool pack, int nray, int nv, int nstep_max, const int32_t* npoints,
                       const long long* offsets, double* ray_vec, double* residual, double* packed_vec,
                       double* packed_res, hipStream_t stream);
hipError_t launch_deposition(const DevParams& P, const DepArgs& D, const double* carry, double* profile,
                             hipStream_t s);
// (rays_deposition.hip; weak: a library linked without them refuses the fused entries by name)
__attribute__((weak)) hipError_t launch_dep_trace_args(const DepTraceArgs& T, DepTraceArgs* d_out, hipStream_t s);
__attribute__((weak)) hipError_t launch_dep2_trace_args(const Dep2TraceArgs& T, Dep2TraceArgs* d_out, hipStream_t s);
__attribute__((weak)) hipError_t launch_profile_sum(int n_bins, int nray, const double* work, const double* carry,
                                                    double* profile, hipStream_t s);
__attribute__((weak)) hipError_t launch_profile_sum_segments(int n_bins, int nray, int n_seg, const int* d_off,
                                                             int rays_per_seg, const double* work, const double* carry,
                                                             double* profile, hipStream_t s);
__attribute__((weak)) hipError_t launch_tile_power(int nray, long long total, const double* power, double* power_runs,
                                                   hipStream_t s);
struct FanArgs;
hipError_t launch_ray_init(int eq_model, int ns, const DevParams& P, const FanArgs& F, int n_cand, double* cand,
                           int* keep, int* block_count, int* offs, int* first_of_launch, double* rvec0,
                           double* rindex_vec0, hipStream_t s);
int ray_init_block();
__global__ void probe_kernel(const DevParams P, int eq, int ns, int nv, int n, const double* v,
                             double* cold7, double* num7, double* dvds, double* resid, int* codes);
}  // namespace rays

namespace {
using namespace rays::host;

thread_local std::string g_err;
std::mutex g_mu;
std::vector<int> g_devices;  // devices used by rays_hip_trace
bool g_devices_explicit = false;  // the list came from rays_hip_init_devices (slots as given, never multiplied)

int fail(const std::string& msg) {
  g_err = msg;
  return 1;
}
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return 2;
}
// `what`: the HIP call behind a call of a resource owner (rays_capi_resources.hpp; these report a bare hipError_t)
#define HIP_TRY_AS(what, call)                       \
  do {                                               \
    hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return hip_fail(e_, what); \
  } while (0)
#define HIP_TRY(call) HIP_TRY_AS(#call, call)

struct FlagText {
  int code;
  const char* text;
};
const FlagText kFlags[] = {
    {RAYS_STOP_NONE, ""},
    {RAYS_STOP_SOUT_GT_SMAX, "sout > s_max"},
    {RAYS_STOP_NSTEP_MAX, " nstep > nstep_max"},
    {RAYS_STOP_X_OUT_OF_BOUNDS, "x out_of_bounds"},
    {RAYS_STOP_Y_OUT_OF_BOUNDS, "y out_of_bounds"},
    {RAYS_STOP_Z_OUT_OF_BOUNDS, "z out_of_bounds"},
    {RAYS_STOP_NEGATIVE_DENS, "negative_dens"},
    {RAYS_STOP_NEGATIVE_TEMP, "negative_temp"},
    {RAYS_STOP_R_OUT_OF_BOX, "R out_of_box"},
    {RAYS_STOP_Z_OUT_OF_BOX, "z out_of_box"},
    {RAYS_STOP_AXI_R_OUT_OF_BOX, "R_out_of_box"},
    {RAYS_STOP_AXI_Z_OUT_OF_BOX, "Z_out_of_box"},
    {RAYS_STOP_OUT_OF_PLASMA, "out_of_plasma"},
    {RAYS_STOP_SOLMAG_R_OUT_OF_BOUNDS, "R out_of_bounds"},
    {RAYS_STOP_SOLMAG_Z_OUT_OF_BOUNDS, "z out_of_bounds"},
    {RAYS_STOP_INFINITE_VG_RHS, "infinite Vg"},
    {RAYS_STOP_RAY_STALLED, "ray stalled"},
    {RAYS_STOP_DISP_RESIDUAL, "dispersion_residual"},
    {RAYS_STOP_INFINITE_VG_CHECK, "infinite_Vg"},
    {RAYS_STOP_TOTAL_ABSORPTION, "total_absorption"},
    {RAYS_STOP_ODE_TOTAL_ERROR, "ODE total error"},
    {RAYS_STOP_SG_MAXNUM, "step number .ge. maxnum"},
    {RAYS_STOP_SG_STIFF, "equations stiff"},
    {RAYS_STOP_SG_T_EQ_TOUT, "t == tout"},
    {RAYS_STOP_SG_NEG_ERR, "relerr or abserr < 0"},
    {RAYS_STOP_SG_EPS_LE_0, "eps <= 0"},
};

static_assert(rays::kBlock == rays::PointWindow<7>::kStride, "PointWindow rows are laid out for the launch block size");
#include "rays_dev_params.inc"

// rays_hip_set_numerics: RAYS_NUMERICS_* (include/rays_hip.h)
int initial_numerics() {
  const char* e = std::getenv("RAYS_HIP_NUMERICS");
  return e && (e[0] == 't' || e[0] == 'T' || e[0] == '1') ? RAYS_NUMERICS_TOLERANCE : RAYS_NUMERICS_EXACT;
}
std::atomic<int> g_numerics{initial_numerics()};

// Which build of a configuration's kernel a launch wants:
//   Recording  the kernel that records the trajectories, in the flavour the numerics setting selects
//   ExactTwin  the exact twin of a tolerance kernel, whose resume kernel takes the handed-over steps: always the
//              one-wave-per-SIMD entry (the only one that carries a resume kernel), whatever the fan size or the
//              developer switch
//   Summary    the summary-only variant of the exact kernel (always exact: the numerics setting is a permission, and the
//              tolerance kernels' hand-over reads residual(:)).  Its objects hold the same shapes as the recording ones
//              (rays_inst.hip), so a configuration is traced summary-only exactly when it is traced at all.
//   Deposit    the fused deposition variant of the summary-only kernel (slab and axisym_toroid groups)
//   Window, WindowSummary
//              the continuation variant (windowed tracing) of the exact kernel, recording or summary-only: always the
//              one-ray-per-lane entry, whatever the fan size -- the only one built, and bit-identical to the others
//   Deposit2   the two-profile variant of the fused deposition kernel (axisym_toroid groups)
//   WindowDeposit, WindowDeposit2
//              the continuation variant of the fused deposition kernels
enum class KernelVariant { Recording, ExactTwin, Summary, Deposit, Window, WindowSummary, Deposit2, WindowDeposit, WindowDeposit2 };
// The build of rays_inst.hip that holds a variant's kernels under the exact numerics (from Summary on the two
// enumerations name the same builds in the same order).
rays::KernelBuild build_of(KernelVariant v) {
  static_assert((int)KernelVariant::Summary == (int)rays::KernelBuild::Summary &&
                (int)KernelVariant::WindowSummary == (int)rays::KernelBuild::WindowSummary &&
                (int)KernelVariant::Deposit2 == (int)rays::KernelBuild::Deposit2 &&
                (int)KernelVariant::WindowDeposit2 == (int)rays::KernelBuild::WindowDeposit2, "KernelVariant | KernelBuild");
  return v < KernelVariant::Summary ? rays::KernelBuild::Recording : (rays::KernelBuild)(int)v;
}

// The registered kernel groups by [build][solver][equilibrium][derivative][unit exponents][multi_spec_damping], made
// from the list on first use: a lookup is an array index.  Two groups under one key are a mistake of the build (an
// object linked twice, or compiled with another object's switches): `duplicate` names the key, and every lookup fails.
struct KernelIndex {
  const rays::KernelGroup* g[rays::kKernelBuilds][2][3][2][2][2] = {};
  std::string duplicate;
};
const KernelIndex& kernel_index() {
  static const KernelIndex index = [] {
    KernelIndex x;
    for (const rays::KernelGroup* k = rays::g_kernel_groups; k; k = k->next) {
      const rays::KernelGroup*& slot = x.g[(int)k->build][k->solver][k->eq_model][k->deriv][k->unit_exp != 0][k->multi_spec != 0];
      if (slot) {
        char key[160];
        std::snprintf(key, sizeof key, "rays_hip: two kernel groups registered as build %d, solver %d, equilibrium %d, "
                      "derivative %d, unit exponents %d, multi_spec_damping %d", (int)k->build, k->solver, k->eq_model,
                      k->deriv, k->unit_exp, k->multi_spec);
        x.duplicate = key;
      }
      slot = k;
    }
    return x;
  }();
  return index;
}

// nray: fan size (0 = unknown).  From two waves per SIMD worth of rays on, the two-waves-per-SIMD build
// of the kernel is preferred where one exists (rays_rk4.hpp) -- under the tolerance flavour for the slab only: the
// two-waves build has no hand-over of ill-conditioned steps (rays_rk4_body.inc), which the slab fans do not need
// (no coalescence; surveyed on 32.8 M steps) and every other equilibrium may.
const rays::KernelEntry* find_kernel(const rays_params_t& p, long long nray = 0,
                                     KernelVariant variant = KernelVariant::Recording) {
  using namespace rays;
  const bool force_exact = variant == KernelVariant::ExactTwin;
  const bool tol = variant == KernelVariant::Recording && g_numerics.load() == RAYS_NUMERICS_TOLERANCE &&
                   p.ode_solver == RAYS_ODE_RK4 && p.ray_deriv == RAYS_DERIV_COLD && !p.multi_spec_damping;
  const KernelIndex& index = kernel_index();
  if (!index.duplicate.empty()) return nullptr;  // (rays_hip_check_params reports it)
  const KernelGroup* kg = index.g[(int)(tol ? KernelBuild::Tolerance : build_of(variant))][p.ode_solver][p.equilib_model]
                                 [p.ray_deriv][unit_exponents(p) ? 1 : 0][p.multi_spec_damping ? 1 : 0];
  if (!kg) return nullptr;  // (a group this library was linked without)
  const KernelEntry* e = kg->entries;
  const int n = kg->n;
  int ncu = 256;
  {
    int dev = 0;
    if (nray > 0 && hipGetDevice(&dev) == hipSuccess) ncu = device_cu_count(dev);
  }
  bool big = nray >= 2ll * ncu * 256;  // >= two waves per SIMD
  if (tol && p.equilib_model != RAYS_EQ_SLAB) big = false;
  if (const char* f = std::getenv("RAYS_HIP_FORCE_WAVES_PER_SIMD"))  // developer measurement: "1" | "2"
    big = f[0] == '2';
  if (force_exact) big = false;
  // SG with finite-difference dD (nv = 7) exists in two mappings: one ray per group of four lanes
  // (rays_sg_group.hpp, the default: 212 against 300 ms per pass on the 64k-ray Solovev fan) and one ray per lane
  // (rays_sg.hpp; RAYS_HIP_SG_GROUP=0, for A/B measurements).  Both are bit-identical to the reference.
  bool group = true;
  if (const char* f = std::getenv("RAYS_HIP_SG_GROUP")) group = f[0] != '0';
  const KernelEntry* found = nullptr;
  for (int i = 0; i < n; i++)
    if (e[i].ns == p.nspec + 1 && e[i].nv == p.nv) {
      if (e[i].lanes_per_ray > 1) {
        if (group) return &e[i];
        continue;
      }
      if (e[i].occ == 1 && !found) found = &e[i];
      if (e[i].occ == 2 && big) return &e[i];
    }
  return found;
}

// Z-function spline table: host = fspl[nx][4].  (g_mu guards the three tables and their shapes.)
struct ZfunTable : DeviceTable {
  int nx = 0;
  double xmin = 0., xmax = 0.;
} g_zfun;

int get_zfun_device(const double** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_zfun.nx <= 0) return fail("damping_model = 'damp_fund_ECH' needs rays_hip_set_zfun_table() first");
  HIP_TRY_AS("hipMalloc / hipMemcpy (Z-function table)", g_zfun.device_ptr(out));
  return 0;
}

// axisym_toroid spline tables: host = all arrays back to back
struct AxisymTable : DeviceTable {
  size_t off[11] = {0};      // r_grid z_grid psi rb_grid rb_fspl ne_grid ne_fspl te_grid te_fspl ti_grid ti_fspl
  int nr = 0, nz = 0, n_rb = 0, n_ne = 0, n_te = 0, n_ti = 0;
  bool lin = false;          // tables of 'eqdsk_magnetics_lin_interp': psi = Psi(nr, nz) raw, rb_fspl = T(nr), rb_grid empty
  double dR = 0., dZ = 0.;
} g_axi;

int get_axisym_device(rays::DevParams* D) {
  std::lock_guard<std::mutex> lk(g_mu);
  const bool analytic = D->a_mag_model == RAYS_AXI_MAG_SOLOVEV;  // 'solovev_magnetics': no psi / RBphi tables
  if (analytic && g_axi.host.empty()) {
    D->a_nr = D->a_nz = D->a_n_rb = D->a_n_ne = D->a_n_te = D->a_n_ti = 0;
    D->a_r_grid = D->a_z_grid = D->a_psi_fspl = D->a_rb_grid = D->a_rb_fspl = nullptr;
    D->a_ne_grid = D->a_ne_fspl = D->a_te_grid = D->a_te_fspl = D->a_ti_grid = D->a_ti_fspl = nullptr;
    D->a_tab1d_doubles = 0;
    D->a_lds_tab = D->a_lds_rz = 0;
    set_spline_axes(*D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return 0;
  }
  const bool lin = D->a_mag_model == RAYS_AXI_MAG_EQDSK_LIN;
  if (lin && !g_axi.lin)
    return fail("magnetics_model = 'eqdsk_magnetics_lin_interp' needs rays_hip_set_eqdsk_lin_tables() first");
  if (!analytic && !lin && (g_axi.lin || g_axi.nr <= 1 || g_axi.nz <= 1 || g_axi.n_rb <= 1))
    return fail("equilib_model = 'axisym_toroid' needs rays_hip_set_axisym_tables() first");
  const double* b = nullptr;
  HIP_TRY_AS("hipMalloc / hipMemcpy (axisym tables)", g_axi.device_ptr(&b));
  D->a_nr = g_axi.nr; D->a_nz = g_axi.nz; D->a_n_rb = g_axi.n_rb;
  D->a_n_ne = g_axi.n_ne; D->a_n_te = g_axi.n_te; D->a_n_ti = g_axi.n_ti;
  D->a_r_grid = b + g_axi.off[0]; D->a_z_grid = b + g_axi.off[1]; D->a_psi_fspl = b + g_axi.off[2];
  D->a_rb_grid = b + g_axi.off[3]; D->a_rb_fspl = b + g_axi.off[4];
  D->a_ne_grid = b + g_axi.off[5]; D->a_ne_fspl = b + g_axi.off[6];
  D->a_te_grid = b + g_axi.off[7]; D->a_te_fspl = b + g_axi.off[8];
  D->a_ti_grid = b + g_axi.off[9]; D->a_ti_fspl = b + g_axi.off[10];
  D->a_tab1d_doubles = (int)(g_axi.host.size() - g_axi.off[3]);  // rb .. ti: contiguous at the end of the blob
  for (int k = 0; k < 8; k++) D->a_tab_off[k] = (int)(g_axi.off[3 + k] - g_axi.off[3]);
  D->a_lin_dR = g_axi.dR;
  D->a_lin_dZ = g_axi.dZ;
  D->a_lds_tab = 0;
  D->a_lds_rz = 0;
  {
    const double* h = g_axi.host.data();  // the host image of the same blob
    const auto at = [&](int k, int n) { return n > 1 ? h + g_axi.off[k] : nullptr; };
    set_spline_axes(*D, at(0, g_axi.nr), at(1, g_axi.nz), at(3, g_axi.n_rb), at(5, g_axi.n_ne), at(7, g_axi.n_te),
                    at(9, g_axi.n_ti));
  }
  return 0;
}

// The kernels' parameter block for p with the axisym_toroid tables on the current device (uploaded when stale), for the
// entries that read no Z-function table.
int dev_params_with_axisym(const rays_params_t* p, rays::DevParams* D) {
  *D = make_dev_params(*p);
  return p->equilib_model == RAYS_EQ_AXISYM ? get_axisym_device(D) : 0;
}

// rho(psiN) spline table: host = grid[n] then fspl[n][4]
struct RhoTable : DeviceTable {
  int n = 0;
} g_rho;
int get_rho_device(const double** out, int* n) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_rho.n < 2) return fail("Ptotal_rho needs rays_hip_set_rho_table() first");
  HIP_TRY_AS("hipMalloc / hipMemcpy (rho table)", g_rho.device_ptr(out));
  *n = g_rho.n;
  return 0;
}

// The binning grid of `which` and the rho(psiN) table on the current device: the same members of DepArgs and DepTraceArgs.
template <class Args>
int fill_deposition_grid(const rays_params_t* p, int which, Args* A) {
  A->grid_min = 0.0; A->grid_max = 1.0;  // deposition_profiles_m.f90:176-177
  if (which == RAYS_DEP_PTOTAL_X) { A->grid_min = p->slab.xmin; A->grid_max = p->slab.xmax; }  // :136-137
  A->rho_grid = nullptr; A->rho_fspl = nullptr; A->n_rho = 0;
  if (which == RAYS_DEP_PTOTAL_RHO) {
    const double* t = nullptr;
    int n = 0;
    const int rc = get_rho_device(&t, &n);
    if (rc) return rc;
    A->rho_grid = t; A->rho_fspl = t + n; A->n_rho = n;
  }
  return 0;
}

// Per-device ring of refill counters.  A slot is handed to one launch at a time: the launch records
// the slot's event behind its kernel, and a later launch that comes round to the same slot waits for
// that event first (more than kCounterSlots launches in flight on one device would otherwise share a
// counter and silently skip rays).
constexpr int kCounterSlots = 256;
constexpr int kCounterStride = 32;  // 128 B apart
struct DeviceWorkspace {
  unsigned int* counters = nullptr;
  hipEvent_t done[kCounterSlots] = {};
  bool used[kCounterSlots] = {};
  int next = 0;
};
DeviceWorkspace g_ws[kMaxDevices];

int get_counter(unsigned int** out, int* slot_out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return fail("rays_hip: device ordinal >= 16");
  hipEvent_t wait_for = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceWorkspace& w = g_ws[dev];
    if (!w.counters) HIP_TRY(hipMalloc(&w.counters, sizeof(unsigned int) * kCounterSlots * kCounterStride));
    const int slot = w.next;
    w.next = (w.next + 1) % kCounterSlots;
    if (!w.done[slot]) HIP_TRY(hipEventCreateWithFlags(&w.done[slot], hipEventDisableTiming));
    if (w.used[slot]) wait_for = w.done[slot];
    w.used[slot] = true;
    *out = w.counters + (size_t)slot * kCounterStride;
    *slot_out = slot;
  }
  if (wait_for && hipEventQuery(wait_for) != hipSuccess) {
    (void)hipGetLastError();
    HIP_TRY(hipEventSynchronize(wait_for));  // the launch that last used this slot is still running
  }
  return 0;
}
// One block per (device, stream) each, grown on demand, released by rays_hip_finalize:
StreamWorkspace g_sg_ws;     // the SG kernels' upper storage tiers (TraceArgs::sg_far); a tolerance launch's summaries
StreamWorkspace g_sched_ws;  // state of the "long rays first" hand-out order of the RK4 kernels (TraceArgs::sched;
                             // rays_trace.hpp: take_rays)
// scratch of rays_hip_ode_step_device (a host that calls the entry per time step would otherwise pay four hipMalloc /
// hipFree per call)
StreamWorkspace g_step_ws;
// the DepTraceArgs block of a fused deposition launch (rays_deposition.hpp).  Like g_sg_ws it is keyed by (device, stream
// handle): the 64 bytes of a stream that claim_slot_for_device has destroyed stay under the stale handle until
// rays_hip_finalize, and a new stream that gets the same handle value takes the block over -- harmless, the block is
// rewritten on the stream before every launch that reads it.
StreamWorkspace g_dep_ws;
StreamWorkspace g_dep2_ws;   // the same for the Dep2TraceArgs block of a two-profile launch (rays_hip_trace_profiles*)
StreamWorkspace g_post_ws;   // scratch of a post-processor that lives in a translation unit of its own (rays_oxconv.hip:
                             // the scan's hand-over to the ascent, 8 bytes per ray; capi_stream_workspace)
// A fused ds scan (rays_hip_scan_profiles_device) keeps its tiled power weights in the same block, kDepArgsRoom bytes
// behind the argument block: one weight per ray of the launch.
constexpr size_t kDepArgsRoom = 128;
struct ScanPart {
  const double* ds_run;  // [n_runs] on the device
  int members;           // rays per run: `in` holds one start and one weight per fan member
};
// Neighbourhood size of that order: every second row of 64 rays is traced first (cfg 5b: 4.05 | 3.26 | 3.34 | 3.42 ms for
// index order | 2 | 4 | 8; the model of tools/refill_model.py agrees: the more pilots, the better the later half is
// ordered).  RAYS_HIP_RAY_ORDER=index hands the rays out in index order instead (for A/B measurements; the results
// are the same), RAYS_HIP_RAY_ORDER=pilot2 ... pilot8 sets other neighbourhood sizes (developer switch).
constexpr int kSchedStride = 2;
int sched_stride() {
  const char* f = std::getenv("RAYS_HIP_RAY_ORDER");
  if (!f || !f[0]) return kSchedStride;
  if (f[0] == 'i') return 0;
  const int n = (int)std::strlen(f);
  const int s = f[n - 1] - '0';
  return (s >= 2 && s <= 8) ? s : kSchedStride;
}

// RAYS_HIP_RK4_LOOP=general: every launch of an RK4 trace kernel takes the general step loop, also where its parameters
// allow the lean one (rays_rk4.hpp; developer switch for A/B measurements on one library and for the tests -- the exact
// kernels' results are the same).  Read at every launch.
bool rk4_loop_forced_general() {
  const char* f = std::getenv("RAYS_HIP_RK4_LOOP");
  return f && (f[0] == 'g' || f[0] == 'G');
}
// The loop `kernel` runs for p: 1 = lean, 0 = general.  What the kernel itself decides from its arguments.
int rk4_loop_of(const rays::KernelEntry& kernel, const rays_params_t& p) {
  if (kernel.solver != RAYS_ODE_RK4 || kernel.occ != 1 || !rays::rk4_lean_built(kernel.eq, kernel.ns, kernel.deriv)) return 0;
  rays::TraceArgs A = rays::TraceArgs();
  if (rk4_loop_forced_general()) A.sg_far_lanes = rays::kRk4ForceGeneralLoop;
  return rays::rk4_lean_loop(make_dev_params(p), kernel.ns, A) ? 1 : 0;
}

int counter_launched(int slot, hipStream_t stream) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  HIP_TRY(hipEventRecord(g_ws[dev].done[slot], stream));
  return 0;
}

}  // namespace

extern "C" {

int rays_hip_last_error(char* buf, int len) {
  if (buf && len > 0) {
    std::snprintf(buf, (size_t)len, "%s", g_err.c_str());
  }
  return (int)g_err.size();
}

const char* rays_hip_stop_flag_text(int stop_code) {
  for (const FlagText& f : kFlags)
    if (f.code == stop_code) return f.text;
  return "";
}

int rays_hip_set_zfun_table(const double* fspl_re, int nx, double x_min, double x_max) {
  if (!fspl_re || nx < 2 || !(x_max > x_min)) return fail("rays_hip_set_zfun_table: bad table");
  std::lock_guard<std::mutex> lk(g_mu);
  g_zfun.host.assign(fspl_re, fspl_re + 4 * (size_t)nx);
  g_zfun.nx = nx;
  g_zfun.xmin = x_min;
  g_zfun.xmax = x_max;
  g_zfun.version++;
  return 0;
}

static int set_axisym_tables_impl(const rays_axisym_tables_t* t, bool lin, double dR, double dZ) {
  // (magnetics_model = 'solovev_magnetics' with splined profiles: nr = nz = n_rb = 0, profile tables only)
  const bool profiles_only = t && t->nr == 0 && t->nz == 0 && t->n_rb == 0 && (t->n_ne > 0 || t->n_te > 0 || t->n_ti > 0);
  if (!t || (!profiles_only && !lin && (t->nr < 2 || t->nz < 2 || t->n_rb < 2 || !t->r_grid || !t->z_grid || !t->psi_fspl ||
                                        !t->rb_grid || !t->rb_fspl)))
    return fail("rays_hip_set_axisym_tables: bad tables");
  if ((t->n_ne > 0 && (!t->ne_grid || !t->ne_fspl)) || (t->n_te > 0 && (!t->te_grid || !t->te_fspl)) ||
      (t->n_ti > 0 && (!t->ti_grid || !t->ti_fspl)))
    return fail("rays_hip_set_axisym_tables: profile table pointers missing");
  std::lock_guard<std::mutex> lk(g_mu);
  AxisymTable& h = g_axi;
  h.host.clear();
  const double* src[11] = {t->r_grid, t->z_grid, t->psi_fspl, t->rb_grid, t->rb_fspl, t->ne_grid, t->ne_fspl,
                           t->te_grid, t->te_fspl, t->ti_grid, t->ti_fspl};
  // ('eqdsk_magnetics_lin_interp': raw Psi(nr, nz) and T(nr) in the psi / rb_fspl slots, no rb_grid)
  const size_t len[11] = {(size_t)t->nr, (size_t)t->nz, (size_t)(lin ? 1 : 16) * t->nr * t->nz, lin ? (size_t)0 : (size_t)t->n_rb,
                          (size_t)(lin ? 1 : 4) * t->n_rb, (size_t)(t->n_ne > 0 ? t->n_ne : 0), (size_t)4 * (t->n_ne > 0 ? t->n_ne : 0),
                          (size_t)(t->n_te > 0 ? t->n_te : 0), (size_t)4 * (t->n_te > 0 ? t->n_te : 0),
                          (size_t)(t->n_ti > 0 ? t->n_ti : 0), (size_t)4 * (t->n_ti > 0 ? t->n_ti : 0)};
  for (int k = 0; k < 11; k++) {
    h.off[k] = h.host.size();
    if (len[k]) h.host.insert(h.host.end(), src[k], src[k] + len[k]);
    while (h.host.size() % 16) h.host.push_back(0.);  // keep every table 128-B aligned
  }
  h.nr = t->nr; h.nz = t->nz; h.n_rb = t->n_rb;
  h.n_ne = t->n_ne > 0 ? t->n_ne : 0; h.n_te = t->n_te > 0 ? t->n_te : 0; h.n_ti = t->n_ti > 0 ? t->n_ti : 0;
  h.lin = lin; h.dR = dR; h.dZ = dZ;
  h.version++;
  return 0;
}
int rays_hip_set_axisym_tables(const rays_axisym_tables_t* t) { return set_axisym_tables_impl(t, false, 0., 0.); }
int rays_hip_set_eqdsk_lin_tables(const rays_axisym_tables_t* t, double dR, double dZ) {
  if (!t || t->nr < 2 || t->nz < 2 || t->n_rb != t->nr || !t->r_grid || !t->z_grid || !t->psi_fspl || !t->rb_fspl ||
      !(dR > 0.) || !(dZ > 0.))
    return fail("rays_hip_set_eqdsk_lin_tables: bad tables");
  return set_axisym_tables_impl(t, true, dR, dZ);
}

int rays_hip_sizeof_params(void) { return (int)sizeof(rays_params_t); }

int rays_hip_set_numerics(int mode) {
  if (mode != RAYS_NUMERICS_EXACT && mode != RAYS_NUMERICS_TOLERANCE) {
    g_err = "rays_hip_set_numerics: unknown mode";
    return -1;
  }
  return g_numerics.exchange(mode);
}
int rays_hip_get_numerics(void) { return g_numerics.load(); }

int rays_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rays_hip_init(int ngpu) {
  int n = rays_hip_device_count();
  if (n <= 0) {
    g_err = "rays_hip_init: no HIP device visible";
    return -1;
  }
  if (ngpu <= 0 || ngpu > n) ngpu = n;
  if (ngpu > kMaxDevices) ngpu = kMaxDevices;
  std::lock_guard<std::mutex> lk(g_mu);
  g_devices.clear();
  for (int i = 0; i < ngpu; i++) g_devices.push_back(i);
  g_devices_explicit = false;
  return ngpu;
}

int rays_hip_init_devices(int n, const int* device_ids) {
  const int visible = rays_hip_device_count();
  if (visible <= 0) {
    g_err = "rays_hip_init_devices: no HIP device visible";
    return -1;
  }
  if (n <= 0 || n > kMaxDevices || !device_ids) {
    g_err = "rays_hip_init_devices: 1..16 device slots";
    return -1;
  }
  for (int i = 0; i < n; i++)
    if (device_ids[i] < 0 || device_ids[i] >= visible) {
      g_err = "rays_hip_init_devices: device ordinal out of range";
      return -1;
    }
  std::lock_guard<std::mutex> lk(g_mu);
  g_devices.assign(device_ids, device_ids + n);
  g_devices_explicit = true;
  return n;
}

static void rccl_close_all();
static void drop_kept_result();
static void drop_gathered_result();
static void release_staging();
// Everything the library holds on the devices and in pinned memory goes back to the driver; the settings (tables'
// host copies, numerics, the keep switch) stay, and the next call initialises lazily as the first one did.
int rays_hip_finalize(void) {
  rccl_close_all();
  drop_kept_result();
  drop_gathered_result();
  std::lock_guard<std::mutex> lk(g_mu);
  for (int d = 0; d < kMaxDevices; d++)
    if (g_ws[d].counters) {
      (void)hipSetDevice(d);
      (void)hipDeviceSynchronize();
      (void)hipFree(g_ws[d].counters);
      for (hipEvent_t e : g_ws[d].done)
        if (e) (void)hipEventDestroy(e);
      g_ws[d] = DeviceWorkspace();
    }
  for (StreamWorkspace* w : {&g_sg_ws, &g_sched_ws, &g_step_ws, &g_dep_ws, &g_dep2_ws, &g_post_ws}) w->release_all();
  for (DeviceTable* t : std::initializer_list<DeviceTable*>{&g_zfun, &g_axi, &g_rho}) t->release_all();
  release_staging();
  release_cached_device_blocks();
  g_devices.clear();
  return 0;
}

int rays_hip_check_params(const rays_params_t* p) {
  if (!p) return fail("rays_hip: null parameter block");
  if (p->abi_version != RAYS_ABI_VERSION) return fail("rays_hip: rays_params_t ABI version mismatch");
  if (p->nspec < 0 || p->nspec > RAYS_NSPEC0) return fail("rays_hip: nspec out of range 0..5");
  if (p->ode_solver != RAYS_ODE_RK4 && p->ode_solver != RAYS_ODE_SG)
    return fail("ode_solver, invalid ode solver");  // ode_m.f90:246-249
  if (p->ray_deriv != RAYS_DERIV_COLD && p->ray_deriv != RAYS_DERIV_NUM)
    return fail("EQN_RAY: invalid value, ray_deriv_name");  // eqn_ray.f90:120-122
  if (p->ray_param != RAYS_PARAM_ARCL && p->ray_param != RAYS_PARAM_TIME)
    return fail("EQN_RAY: invalid ray parameter");  // eqn_ray.f90:183-185
  if (p->equilib_model != RAYS_EQ_SLAB && p->equilib_model != RAYS_EQ_SOLOVEV && p->equilib_model != RAYS_EQ_AXISYM)
    return fail("equilibrium_m: invalid equilibrium model (device path: slab | solovev | axisym_toroid)");
  if (p->damping_model != RAYS_DAMP_NONE && p->damping_model != RAYS_DAMP_FUND_ECH)
    return fail("damping: Unimplemented damping model");  // damping_m.f90:103-106
  if (p->multi_spec_damping && !p->damping_model)  // eqn_ray.f90:196-213: the species rows sit inside the damping branch
    return fail("rays_hip: multi_spec_damping without a damping model leaves its rows of the ODE vector undefined");
  if (p->nv != 7 + (p->damping_model ? 1 : 0) + (p->multi_spec_damping ? 1 + p->nspec : 0) +
                   (p->integrate_eq_gradients ? 5 : 0))
    return fail("rays_hip: nv must be 7 (+1 with damping, +1+nspec with multi_spec_damping, +5 with "
                "integrate_eq_gradients) (ode_m.f90:160-173)");
  if (p->nstep_max < 0) return fail("rays_hip: nstep_max < 0");
  if (p->equilib_model == RAYS_EQ_SOLOVEV) {
    if (p->solovev.dens_prof_model != RAYS_SOLOVEV_N_CONSTANT && p->solovev.dens_prof_model != RAYS_SOLOVEV_N_PARABOLIC)
      return fail("solovev_eq invalid dens_prof_model");  // solovev_eq_m.f90:227-229
    for (int is = 0; is <= p->nspec; is++)
      if (p->solovev.t_prof_model[is] != RAYS_SOLOVEV_T_ZERO && p->solovev.t_prof_model[is] != RAYS_SOLOVEV_T_PARABOLIC)
        return fail("SOLOVEV: t_prof_model must be 'zero' or 'parabolic' ('constant' leaves ts undefined in the reference)");
  } else if (p->equilib_model == RAYS_EQ_AXISYM) {
    const rays_axisym_params_t& a = p->axisym;
    if (a.magnetics_model != RAYS_AXI_MAG_EQDSK_SPLINE && a.magnetics_model != RAYS_AXI_MAG_SOLOVEV &&
        a.magnetics_model != RAYS_AXI_MAG_EQDSK_LIN)
      return fail("axisym_toroid: magnetics_model must be 'eqdsk_magnetics_spline_interp', 'eqdsk_magnetics_lin_interp' "
                  "or 'solovev_magnetics'");
    if (a.magnetics_model == RAYS_AXI_MAG_SOLOVEV &&
        (p->solovev.outer_bound < p->solovev.rmaj || p->solovev.outer_bound >= std::sqrt(2.) * p->solovev.rmaj))
      return fail("Inner boundary complex, outer_bound >=  sqrt2*rmaj");  // solovev_magnetics_m.f90:99-103
    if (a.density_prof_model < 0 || a.density_prof_model > RAYS_AXI_N_SPLINE)
      return fail("axisym_toroid_eq: Unknown density_prof_model");
    for (int is = 0; is <= p->nspec; is++)
      if (a.t_prof_model[is] < 0 || a.t_prof_model[is] > RAYS_AXI_T_SPLINE)
        return fail("axisym_toroid_eq: Unknown temperature_prof_model");
    if (!(a.psiB != 0.)) return fail("axisym_toroid: psiB (PSIBOUND - PSIAXIS) is zero");
  } else {
    const rays_slab_params_t& s = p->slab;
    if (s.bx_prof_model != RAYS_SLAB_BX_ZERO) return fail("SLAB: invalid bx_prof_model");
    if (s.by_prof_model < 0 || s.by_prof_model > RAYS_SLAB_BY_LINEAR_SHEAR) return fail("SLAB: invalid by_prof_model");
    if (s.bz_prof_model < 0 || s.bz_prof_model > RAYS_SLAB_BZ_LINEAR_2) return fail("SLAB: invalid bz_prof_model");
    if (s.dens_prof_model < 0 || s.dens_prof_model > RAYS_SLAB_N_GAUSSIAN) return fail("SLAB: invalid dens_prof_model");
    for (int is = 0; is <= p->nspec; is++)
      if (s.t_prof_model[is] < 0 || s.t_prof_model[is] > RAYS_SLAB_T_PARABOLIC) return fail("SLAB: invalid t_prof_model");
  }
  if (p->ode_solver == RAYS_ODE_SG && (p->rel_err0 < (double)1.e-10f || p->abs_err0 < (double)1.e-10f))
    return fail("initialize_SG_ode: rel_err0, abs_err0 too small");  // SG_ode_m.f90:63-66
  if (!kernel_index().duplicate.empty()) return fail(kernel_index().duplicate);
  if (!find_kernel(*p)) {
    char msg[256];
    std::snprintf(msg, sizeof msg, "rays_hip: no kernel built for this configuration (%s, equilibrium %d, %d species, %s dD, "
                  "nv = %d%s): the default library holds nspec = 1 plus the fixtures' shapes -- rebuild with "
                  "`make -C rays_amd/csrc FULL=1` for every species count", p->ode_solver == RAYS_ODE_RK4 ? "RK4" : "SG",
                  p->equilib_model, p->nspec + 1, p->ray_deriv == RAYS_DERIV_COLD ? "cold" : "numerical", p->nv,
                  p->multi_spec_damping ? ", multi_spec_damping" : "");
    return fail(msg);
  }
  return 0;
}

const char* rays_hip_kernel_name(const rays_params_t* p) {
  if (!p || rays_hip_check_params(p)) return "";
  return find_kernel(*p)->name;
}

const char* rays_hip_kernel_name_for(const rays_params_t* p, int nray) {
  if (!p || rays_hip_check_params(p)) return "";
  return find_kernel(*p, nray)->name;
}

int rays_hip_rk4_loop_for(const rays_params_t* p, int nray) {
  if (!p || rays_hip_check_params(p) || p->ode_solver != RAYS_ODE_RK4) return -1;
  return rk4_loop_of(*find_kernel(*p, nray), *p);
}

const char* rays_hip_summary_kernel_name_for(const rays_params_t* p, int nray) {
  if (!p || rays_hip_check_params(p)) return "";
  const rays::KernelEntry* k = find_kernel(*p, nray, KernelVariant::Summary);
  return k ? k->name : "";
}

// Common launcher of the trace kernels: `extra` carries the optional per-ray starting conditions and the
// per-run steps of a fused scan (rays_trace.hpp: TraceArgs).
namespace {
// The device pointers of the tables p's kernels read, on the current device: the Z-function spline (with damping) and
// the axisym_toroid tables (uploaded when stale).
int device_tables(const rays_params_t* p, rays::DevParams* Dp) {
  rays::DevParams& D = *Dp;
  int rc = 0;
  if (p->damping_model == RAYS_DAMP_FUND_ECH) {
    const double* zf = nullptr;
    rc = get_zfun_device(&zf);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    D.zf_fspl = zf;
    D.zf_nx = g_zfun.nx;
    D.zf_xmin = g_zfun.xmin;
    D.zf_xmax = g_zfun.xmax;
  }
  if (p->equilib_model == RAYS_EQ_AXISYM) {
    rc = get_axisym_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    const bool need_ne = p->axisym.density_prof_model == RAYS_AXI_N_SPLINE && g_axi.n_ne < 2;
    bool need_t = false;
    for (int is = 0; is <= p->nspec; is++)
      if (p->axisym.t_prof_model[is] == RAYS_AXI_T_SPLINE && (g_axi.n_te < 2 || g_axi.n_ti < 2)) need_t = true;
    if (need_ne || need_t) return fail("axisym_toroid: spline profile model selected but its table was not set");
  }
  return 0;
}

struct TraceExtras {
  const double* v0 = nullptr;
  const double* s0 = nullptr;
  const double* ds_run = nullptr;
  int rays_per_run = 0;
  // KernelVariant::Deposit: the device block the kernel reads its binning arguments from
  const rays::DepTraceArgs* dep = nullptr;
  // KernelVariant::Deposit2: the same for the two-profile kernel
  const rays::Dep2TraceArgs* dep2 = nullptr;
  // KernelVariant::Window | WindowSummary: the saved ray state and the window's length (rays_trace.hpp:
  // TraceArgs::state); state_init: launch the shape's state_init kernel instead of the trace kernel
  const rays::TraceArgs::State* state = nullptr;
  int n_steps = 0;
  bool state_init = false;
};
// variant: Recording (into `traj`), Summary or Deposit (no trajectory arrays; out.sv is optional).  out.ev, out.er and
// out.mr are optional for a recording launch.  Window (into the slabs `traj`) | WindowSummary | WindowDeposit |
// WindowDeposit2: out.np is npoints_win and the other summaries live in extra.state; the last two also take extra.dep |
// extra.dep2 (the ray_vec slot, which the summary-policy continuation kernels leave null).
int launch_trace(const rays_params_t* p, KernelVariant variant, int nray, const RayInputs& in,
                 const TrajectoryArrays& traj, const SummaryArrays& out, hipStream_t stream, int flags,
                 const TraceExtras& extra = TraceExtras()) {
  const size_t npt = (size_t)p->nstep_max + 1;
  const bool recording = variant == KernelVariant::Recording;
  if (recording && !(flags & RAYS_TRACE_NO_ZERO_FILL)) {  // ray_results_m.f90:154-164
    HIP_TRY(hipMemsetAsync(traj.rv, 0, sizeof(double) * npt * (size_t)p->nv * (size_t)nray, stream));
    HIP_TRY(hipMemsetAsync(traj.res, 0, sizeof(double) * npt * (size_t)nray, stream));
  }
  unsigned int* counter = nullptr;
  int counter_slot = 0;
  int rc = get_counter(&counter, &counter_slot);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(counter, 0, sizeof(unsigned int), stream));
  rays::TraceArgs A;
  A.nray = nray;
  A.rvec0 = in.rvec0;
  A.rindex_vec0 = in.rindex_vec0;
  const bool window_dep = variant == KernelVariant::WindowDeposit || variant == KernelVariant::WindowDeposit2;
  const bool window = variant == KernelVariant::Window || variant == KernelVariant::WindowSummary || window_dep;
  A.ray_vec = recording || variant == KernelVariant::Window ? traj.rv : nullptr;
  A.residual = recording || variant == KernelVariant::Window ? traj.res : nullptr;
  A.npoints = out.np;
  A.stop_code = out.sc;
  A.end_ray_vec = out.ev;
  A.end_residuals = out.er;
  A.max_residuals = out.mr;
  A.next_ray = counter;
  A.v0 = extra.v0;
  A.s0 = extra.s0;
  A.ds_run = extra.ds_run;
  A.rays_per_run = extra.rays_per_run;
  A.sg_far = nullptr;
  A.sg_far_lanes = 0;
  A.sched = nullptr;
  A.sched_stride = 0;
  A.set_start_ray_vec(recording ? nullptr : out.sv);
  if (variant == KernelVariant::Deposit || variant == KernelVariant::WindowDeposit) A.set_dep(extra.dep);
  if (variant == KernelVariant::Deposit2 || variant == KernelVariant::WindowDeposit2) A.set_dep2(extra.dep2);
  if (window) A.set_state(*extra.state, extra.n_steps);
  const rays::KernelEntry* kernel = find_kernel(*p, nray, variant);
  if (!kernel || (extra.state_init && !kernel->resume))
    return fail(window_dep ? "rays_hip: the deposition window kernel of this configuration is not in this build"
                : window ? "rays_hip: the continuation kernel of this configuration is not in this build"
                : variant == KernelVariant::Deposit2
                    ? "rays_hip: the two-profile deposition kernel of this configuration is not in this build"
                : variant == KernelVariant::Deposit
                    ? "rays_hip: the fused deposition kernel of this configuration is not in this build"
                    : "rays_hip: the summary-only kernel of this configuration is not in this build");
  if (extra.state_init) {  // one lane per ray, no refill: neither the counter nor a workspace is used
    rays::DevParams Di = make_dev_params(*p);
    rc = device_tables(p, &Di);
    if (rc) return rc;
    const hipError_t ei = kernel->resume(Di, A, stream);
    if (ei != hipSuccess) return hip_fail(ei, "state_init kernel launch");
    return counter_launched(counter_slot, stream);
  }
  const int stride = kernel->solver == RAYS_ODE_RK4 ? sched_stride() : 0;
  if (kernel->solver == RAYS_ODE_RK4 && rk4_loop_forced_general()) A.sg_far_lanes = rays::kRk4ForceGeneralLoop;
  if (stride > 1) {
    // more rays than one wave per SIMD holds (the kernel decides with the lanes it is launched with)
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if ((long long)nray > (long long)rays::device_cu_count(dev) * rays::kBlock) {
      const size_t words = 4 + rays::sched_pilots((unsigned)nray, stride);
      unsigned int* ws = nullptr;
      HIP_TRY_AS("hipMalloc (ray order workspace)", g_sched_ws.get(stream, sizeof(unsigned int) * words, (void**)&ws));
      HIP_TRY(hipMemsetAsync(ws, 0, sizeof(unsigned int) * words, stream));
      A.sched = ws;
      A.sched_stride = stride;
    }
  }
  if (kernel->sg_far_per_lane > 0) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    // the one-ray-per-lane SG kernels fill the CU's LDS with one workgroup, so at most one 256-lane block per CU is
    // resident; the lane-group kernels (G lanes per ray) hold up to four
    const int G = kernel->lanes_per_ray;
    const long long resident = (long long)rays::device_cu_count(dev) * rays::kBlock * (G > 1 ? 4 : 1);
    const long long rays_per_block = rays::kBlock / G;
    const long long want = ((long long)nray + rays_per_block - 1) / rays_per_block * rays::kBlock;
    A.sg_far_lanes = want < resident ? want : resident;
    double* ws = nullptr;
    const size_t far_bytes = sizeof(double) * (size_t)kernel->sg_far_per_lane * (size_t)A.sg_far_lanes;
    HIP_TRY_AS("hipMalloc (SG workspace)", g_sg_ws.get(stream, far_bytes, (void**)&ws));
    A.sg_far = ws;
  }
  rays::DevParams D = make_dev_params(*p);
  rc = device_tables(p, &D);
  if (rc) return rc;
  // A tolerance-flavour kernel hands its ill-conditioned steps over to the reference's arithmetic (rays_rk4_body.inc:
  // kStopResumeExact): the exact twin's resume kernel follows it on the stream.  The hand-over travels in the per-ray
  // summaries, so they exist for such a launch whether or not the caller asked for them.
  const rays::KernelEntry* twin = nullptr;
  if ((kernel->eq & rays::kEqTol) && kernel->occ == 1) {  // (the two-waves build hands nothing over)
    twin = find_kernel(*p, 0, KernelVariant::ExactTwin);
    if (!twin || !twin->resume) return fail("rays_hip: the tolerance kernel's exact twin is not in this build");
    if (!A.end_ray_vec || !A.max_residuals) {
      double* ws = nullptr;
      // (no SG kernel runs with it at the same time: one stream)
      const size_t sum_bytes = sizeof(double) * ((size_t)p->nv + 1) * (size_t)nray;
      HIP_TRY_AS("hipMalloc (SG workspace)", g_sg_ws.get(stream, sum_bytes, (void**)&ws));
      if (!A.end_ray_vec) A.end_ray_vec = ws;
      if (!A.max_residuals) A.max_residuals = ws + (size_t)p->nv * (size_t)nray;
    }
  }
  int grid = 0;
  hipError_t e = kernel->launch(D, A, stream, &grid);
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  if (twin) {
    e = twin->resume(D, A, stream);
    if (e != hipSuccess) return hip_fail(e, "resume kernel launch");
  }
  return counter_launched(counter_slot, stream);
}
}  // namespace

// rays_capi_internal.hpp: this file's state for the entry points defined in other translation units
extern "C++" {
namespace rays {
int capi_fail(const char* msg) { return fail(msg); }
int capi_hip_fail(hipError_t e, const char* what) { return hip_fail(e, what); }
int capi_stream_workspace(hipStream_t stream, size_t bytes, void** out) {
  HIP_TRY_AS("hipMalloc (post-processor workspace)", g_post_ws.get(stream, bytes, out));
  return 0;
}
int capi_dev_params(const rays_params_t* p, DevParams* D, bool* unit_exp) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  *D = make_dev_params(*p);
  if (unit_exp) *unit_exp = unit_exponents(*p);
  return device_tables(p, D);
}
}  // namespace rays
}  // extern "C++"

int rays_hip_trace_device(const rays_params_t* p, int nray, const double* d_rvec0,
                          const double* d_rindex_vec0, double* d_ray_vec, double* d_residual,
                          int32_t* d_npoints, int32_t* d_stop_code, double* d_end_ray_vec,
                          double* d_end_residuals, double* d_max_residuals, void* hip_stream,
                          int flags) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (nray < 0) return fail("rays_hip_trace_device: nray < 0");
  if (nray == 0) return 0;
  if (!d_rvec0 || !d_rindex_vec0 || !d_ray_vec || !d_residual || !d_npoints || !d_stop_code)
    return fail("rays_hip_trace_device: null device pointer");
  return launch_trace(p, KernelVariant::Recording, nray, {d_rvec0, d_rindex_vec0}, {d_ray_vec, d_residual},
                      {d_npoints, d_stop_code, nullptr, d_end_ray_vec, d_end_residuals, d_max_residuals},
                      (hipStream_t)hip_stream, flags);
}

// ray_scan fused into one launch (ray_scan.f90:33-49, scanner_m.f90:174-205: scan_parameter = 'ds').
int rays_hip_scan_device(const rays_params_t* p, int n_runs, const double* d_ds_values, int nray,
                         const double* d_rvec0, const double* d_rindex_vec0, double* d_ray_vec,
                         double* d_residual, int32_t* d_npoints, int32_t* d_stop_code, double* d_end_ray_vec,
                         double* d_end_residuals, double* d_max_residuals, void* hip_stream, int flags) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (n_runs < 0 || nray < 0) return fail("rays_hip_scan_device: n_runs, nray < 0");
  if (n_runs == 0 || nray == 0) return 0;
  if ((long long)n_runs * nray > 0x7fffffffll) return fail("rays_hip_scan_device: n_runs * nray exceeds 2^31 - 1");
  if (!d_ds_values || !d_rvec0 || !d_rindex_vec0 || !d_ray_vec || !d_residual || !d_npoints || !d_stop_code)
    return fail("rays_hip_scan_device: null device pointer");
  TraceExtras x;
  x.ds_run = d_ds_values;
  x.rays_per_run = nray;
  return launch_trace(p, KernelVariant::Recording, n_runs * nray, {d_rvec0, d_rindex_vec0}, {d_ray_vec, d_residual},
                      {d_npoints, d_stop_code, nullptr, d_end_ray_vec, d_end_residuals, d_max_residuals},
                      (hipStream_t)hip_stream, flags, x);
}

// ---- summary-only tracing: ray ends and residual statistics, no trajectories (include/rays_hip.h) --------------------
int rays_hip_trace_summary_device(const rays_params_t* p, int nray, const double* d_rvec0, const double* d_rindex_vec0,
                                  int32_t* d_npoints, int32_t* d_stop_code, double* d_start_ray_vec,
                                  double* d_end_ray_vec, double* d_end_residuals, double* d_max_residuals,
                                  void* hip_stream) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (nray < 0) return fail("rays_hip_trace_summary_device: nray < 0");
  if (nray == 0) return 0;
  if (!d_rvec0 || !d_rindex_vec0 || !d_npoints || !d_stop_code || !d_end_ray_vec || !d_end_residuals || !d_max_residuals)
    return fail("rays_hip_trace_summary_device: null device pointer");
  return launch_trace(p, KernelVariant::Summary, nray, {d_rvec0, d_rindex_vec0}, {},
                      {d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals},
                      (hipStream_t)hip_stream, RAYS_TRACE_NO_ZERO_FILL);
}

int rays_hip_scan_summary_device(const rays_params_t* p, int n_runs, const double* d_ds_values, int nray,
                                 const double* d_rvec0, const double* d_rindex_vec0, int32_t* d_npoints,
                                 int32_t* d_stop_code, double* d_start_ray_vec, double* d_end_ray_vec,
                                 double* d_end_residuals, double* d_max_residuals, void* hip_stream) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (n_runs < 0 || nray < 0) return fail("rays_hip_scan_summary_device: n_runs, nray < 0");
  if (n_runs == 0 || nray == 0) return 0;
  if ((long long)n_runs * nray > 0x7fffffffll)
    return fail("rays_hip_scan_summary_device: n_runs * nray exceeds 2^31 - 1");
  if (!d_ds_values || !d_rvec0 || !d_rindex_vec0 || !d_npoints || !d_stop_code || !d_end_ray_vec || !d_end_residuals ||
      !d_max_residuals)
    return fail("rays_hip_scan_summary_device: null device pointer");
  TraceExtras x;
  x.ds_run = d_ds_values;
  x.rays_per_run = nray;
  return launch_trace(p, KernelVariant::Summary, n_runs * nray, {d_rvec0, d_rindex_vec0}, {},
                      {d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals},
                      (hipStream_t)hip_stream, RAYS_TRACE_NO_ZERO_FILL, x);
}

// ---- windowed tracing: pause rays after n steps, continue from a saved state (include/rays_hip.h) ----
namespace {
int refuse_state(const char* who, const rays_params_t* p, int nray, const rays_ray_state_t* st) {
  if (nray < 0) return fail(std::string(who) + ": nray < 0");
  if (!st || !st->v || !st->s || !st->nstep || !st->stop_code || !st->resid || !st->flags)
    return fail(std::string(who) + ": null pointer in the ray state");
  if (p->ode_solver == RAYS_ODE_SG && !st->sg_err)
    return fail(std::string(who) + ": SG_ODE needs the ray state's sg_err (rel_err, abs_err persist across output steps)");
  return 0;
}
rays::TraceArgs::State state_of(const rays_ray_state_t* st) {
  return rays::TraceArgs::State{st->v, st->s, st->nstep, st->stop_code, st->resid, st->sg_err, st->flags};
}
}  // namespace

int rays_hip_state_init_device(const rays_params_t* p, int nray, const double* d_rvec0, const double* d_rindex_vec0,
                               const rays_ray_state_t* state, double* d_start_ray_vec, void* hip_stream) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  rc = refuse_state("rays_hip_state_init_device", p, nray, state);
  if (rc) return rc;
  if (!d_rvec0 || !d_rindex_vec0) return fail("rays_hip_state_init_device: null device pointer");
  if (nray == 0) return 0;
  const rays::TraceArgs::State st = state_of(state);
  TraceExtras x;
  x.state = &st;
  x.n_steps = 1;
  x.state_init = true;
  SummaryArrays out = {};
  out.sv = d_start_ray_vec;
  return launch_trace(p, KernelVariant::Window, nray, {d_rvec0, d_rindex_vec0}, {}, out, (hipStream_t)hip_stream,
                      RAYS_TRACE_NO_ZERO_FILL, x);
}

int rays_hip_trace_window_device(const rays_params_t* p, int nray, const rays_ray_state_t* state, int n_steps,
                                 double* d_ray_vec_win, double* d_residual_win, int32_t* d_npoints_win,
                                 void* hip_stream) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  rc = refuse_state("rays_hip_trace_window_device", p, nray, state);
  if (rc) return rc;
  if (n_steps < 1) return fail("rays_hip_trace_window_device: n_steps < 1");
  if (!d_npoints_win) return fail("rays_hip_trace_window_device: null device pointer");
  if (!d_ray_vec_win != !d_residual_win)
    return fail("rays_hip_trace_window_device: ray_vec_win and residual_win are given together or not at all");
  if ((long long)nray * n_steps > 0x7fffffffll)
    return fail("rays_hip_trace_window_device: nray * n_steps exceeds 2^31 - 1");
  if (nray == 0) return 0;
  const rays::TraceArgs::State st = state_of(state);
  TraceExtras x;
  x.state = &st;
  x.n_steps = n_steps;
  SummaryArrays out = {};
  out.np = d_npoints_win;
  return launch_trace(p, d_ray_vec_win ? KernelVariant::Window : KernelVariant::WindowSummary, nray, {nullptr, nullptr},
                      {d_ray_vec_win, d_residual_win}, out, (hipStream_t)hip_stream, RAYS_TRACE_NO_ZERO_FILL, x);
}

namespace rays {
// the five summary arrays of a trace from the saved state (ray_tracing.f90:252-260); a refused ray keeps the zeros of
// initialize_ray_results_m
__global__ void state_summary_kernel(int n, int nv, TraceArgs::State st, int32_t* __restrict__ npoints,
                                     int32_t* __restrict__ stop, double* __restrict__ end_ray_vec,
                                     double* __restrict__ end_residuals, double* __restrict__ max_residuals) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const bool refused = (st.flags[r] & kStateRefused) != 0;
  const int nstep = st.nstep[r];
  npoints[r] = nstep + 1;
  stop[r] = st.stop_code[r];
  for (int c = 0; c < nv; c++) end_ray_vec[(long long)r * nv + c] = refused ? 0. : st.v[(long long)r * nv + c];
  end_residuals[r] = (!refused && nstep >= 1) ? st.resid[3ll * r + 1] : 0.;
  max_residuals[r] = refused ? 0. : st.resid[3ll * r + 2];
}
}  // namespace rays

int rays_hip_state_summary_device(const rays_params_t* p, int nray, const rays_ray_state_t* state, int32_t* d_npoints,
                                  int32_t* d_stop_code, double* d_end_ray_vec, double* d_end_residuals,
                                  double* d_max_residuals, void* hip_stream) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  rc = refuse_state("rays_hip_state_summary_device", p, nray, state);
  if (rc) return rc;
  if (!d_npoints || !d_stop_code || !d_end_ray_vec || !d_end_residuals || !d_max_residuals)
    return fail("rays_hip_state_summary_device: null device pointer");
  if (nray == 0) return 0;
  hipLaunchKernelGGL(rays::state_summary_kernel, dim3((nray + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, nray,
                     (int)p->nv, state_of(state), d_npoints, d_stop_code, d_end_ray_vec, d_end_residuals, d_max_residuals);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rays_hip_state_summary_device");
  return 0;
}

const char* rays_hip_window_kernel_name_for(const rays_params_t* p, int nray, int recording) {
  if (!p || rays_hip_check_params(p)) return "";
  const rays::KernelEntry* k = find_kernel(*p, nray, recording ? KernelVariant::Window : KernelVariant::WindowSummary);
  return k ? k->name : "";
}

// Batched `call ode_solver(eqn_ray, nv, v, s, sout, ray_stop)` (ode_m.f90:218-254) + the check_save that
// trace_rays applies to its result (ray_tracing.f90:212-243): one output step from n arbitrary states.
// Runs the trace kernels with nstep_max = 1 from the caller's v0 / s0 and picks point 2 of each ray.
namespace rays {
__global__ void ode_step_collect_kernel(int n, int nv, const double* __restrict__ ray_vec,
                                        const double* __restrict__ residual, const int32_t* __restrict__ npoints,
                                        const int32_t* __restrict__ stop, const double* __restrict__ end_ray_vec,
                                        double* __restrict__ v1, double* __restrict__ resid, int32_t* __restrict__ code) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const bool stepped = npoints[r] == 2;  // the step was taken and passed check_save
  // not recorded: the state `ode_solver` left behind -- the advanced v when check_save refused the step, v0 when the
  // solver itself stopped (ray_tracing.f90:214-234, RK4_ode_m.f90:83-89) -- is the trace kernels' end_ray_vec
  // (zeros when v0 already failed the initial check_save: that ray never started, ray_tracing.f90:100-112)
  for (int c = 0; c < nv; c++)
    v1[(long long)r * nv + c] = stepped ? ray_vec[((long long)r * 2 + 1) * nv + c] : end_ray_vec[(long long)r * nv + c];
  if (resid) resid[r] = stepped ? residual[(long long)r * 2 + 1] : 0.;
  // a ray that took its one step ends on ' nstep > nstep_max' (or 'sout > s_max'), which is not a stop of this step
  code[r] = stepped ? RAYS_STOP_NONE : stop[r];
}
}  // namespace rays

int rays_hip_ode_step_device(const rays_params_t* p, int n, const double* d_v0, const double* d_s0,
                             double* d_v1, double* d_resid, int32_t* d_stop_code, void* hip_stream) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (n < 0) return fail("rays_hip_ode_step_device: n < 0");
  if (n == 0) return 0;
  if (!d_v0 || !d_v1 || !d_stop_code) return fail("rays_hip_ode_step_device: null device pointer");
  hipStream_t stream = (hipStream_t)hip_stream;
  rays_params_t q = *p;
  q.nstep_max = 1;
  q.s_max = 1.7976931348623157e308;
  const size_t nv = (size_t)p->nv, N = (size_t)n;
  // one block: ray_vec[n][2][nv] | residual[n][2] | end_ray_vec[n][nv] | npoints[n] | stop_code[n]
  const size_t off_res = sizeof(double) * 2 * nv * N, off_ev = off_res + sizeof(double) * 2 * N,
               off_np = off_ev + sizeof(double) * nv * N, off_sc = off_np + sizeof(int32_t) * N,
               total = off_sc + sizeof(int32_t) * N;
  char* base = nullptr;
  HIP_TRY_AS("hipMalloc (ode_step scratch)", g_step_ws.get(stream, total, (void**)&base));
  double *d_rv = reinterpret_cast<double*>(base), *d_res = reinterpret_cast<double*>(base + off_res),
         *d_ev = reinterpret_cast<double*>(base + off_ev);
  int32_t *d_np = reinterpret_cast<int32_t*>(base + off_np), *d_sc = reinterpret_cast<int32_t*>(base + off_sc);
  TraceExtras x;
  x.v0 = d_v0;
  x.s0 = d_s0;
  // rvec0 / rindex_vec0 are not read when v0 is given; any valid pointer will do
  rc = launch_trace(&q, KernelVariant::Recording, n, {d_v0, d_v0}, {d_rv, d_res}, {d_np, d_sc, nullptr, d_ev}, stream,
                    RAYS_TRACE_NO_ZERO_FILL, x);
  if (rc) return rc;
  hipLaunchKernelGGL(rays::ode_step_collect_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, (int)nv, d_rv,
                     d_res, d_np, d_sc, d_ev, d_v1, d_resid, d_stop_code);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "rays_hip_ode_step_device");
  return 0;  // asynchronous on `stream` like rays_hip_trace_device (the scratch block outlives the call)
}

// Pinned staging for the packed device-to-host copy of rays_hip_trace: two buffers per device,
// allocated once (pinning is slow) and kept.  `points` = trajectory points one buffer holds.
struct StagingBuffers {
  double* vec[2] = {nullptr, nullptr};
  double* res[2] = {nullptr, nullptr};
  long long points = 0;
  size_t nv = 0;
};
// Fixed storage: every device's host thread keeps a pointer into it for the whole copy phase, so
// the elements must never move (one per slot of the device list, like the block caches).
static StagingBuffers g_staging[kMaxDevices];
static void free_staging(StagingBuffers& sb) {
  for (int b = 0; b < 2; b++) {
    if (sb.vec[b]) (void)hipHostFree(sb.vec[b]);
    if (sb.res[b]) (void)hipHostFree(sb.res[b]);
  }
  sb = StagingBuffers();
}
static StagingBuffers* staging_for_slot(int dev, size_t nv, long long min_points) {
  if (dev < 0 || dev >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  StagingBuffers& sb = g_staging[dev];
  if (sb.points == 0 || sb.nv < nv || sb.points < min_points) {
    free_staging(sb);
    // 1 M points per buffer (8 (nv + 1) MB, e.g. 64 MB for nv = 7), and never less than one whole ray
    const long long pts = std::max(1ll << 20, min_points);
    for (int b = 0; b < 2; b++) {
      if (hipHostMalloc((void**)&sb.vec[b], sizeof(double) * nv * (size_t)pts, hipHostMallocPortable) != hipSuccess ||
          hipHostMalloc((void**)&sb.res[b], sizeof(double) * (size_t)pts, hipHostMallocPortable) != hipSuccess) {
        sb.points = 0;
        return nullptr;
      }
    }
    sb.points = pts;
    sb.nv = nv;
  }
  return &sb;
}
static void release_staging() {  // caller holds g_mu
  for (StagingBuffers& sb : g_staging) free_staging(sb);
}

// ---- the device-resident image of the last rays_hip_trace call (rays_hip_keep_last_result) -------------------------
// The reference's drivers trace and then post-process in one process (RAYS_P.f90:19-44: trace_rays, then the
// deposition profiles of the same ray_results_m arrays).  With the switch on, a block of rays_hip_trace leaves its
// padded ray_vec slab and its npoints on the device it traced on instead of giving them back to the block cache, and
// rays_hip_deposition_last bins them in place: the trajectories cross PCIe once (to the caller's arrays), never back.
struct KeptBlock {
  int slot = -1, dev = -1, r0 = 0, r1 = 0;
  double* d_ray_vec = nullptr;
  int32_t* d_npoints = nullptr;
};
struct KeptResult {
  bool keep = false;
  int nray = 0, nv = 0, nstep_max = 0;
  std::vector<KeptBlock> blocks;  // in ray order once complete
} g_kept;
static void drop_kept_result() {  // caller holds no lock
  std::vector<KeptBlock> old;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    old.swap(g_kept.blocks);
    g_kept.nray = 0;
  }
  if (old.empty()) return;
  CurrentDevice restore;
  for (const KeptBlock& b : old) {
    (void)hipSetDevice(b.dev);
    cached_free(b.slot, b.d_ray_vec);  // (freed, not cached, when the slot serves another device by now)
    cached_free(b.slot, b.d_npoints);
  }
}

// ---- the block driver of the sharded entries (rays_hip_trace, _summary, _deposition, _gather) ------------------------
// The device list of a call: the slots of rays_hip_init[_devices], initialised lazily with every visible device.
// *explicit_list: the list came from rays_hip_init_devices.  0, or 3 when no device can be had.
extern "C++" {
static int call_devices(std::vector<int>* devs, bool* explicit_list = nullptr) {
  const auto snapshot = [&] {
    std::lock_guard<std::mutex> lk(g_mu);
    *devs = g_devices;
    if (explicit_list) *explicit_list = g_devices_explicit;
    return !devs->empty();
  };
  return snapshot() || (rays_hip_init(0) >= 0 && snapshot()) ? 0 : 3;
}

// Cuts [0, nray) into one contiguous block per slot of `devs`, like the reference's OpenMP schedule(static)
// (ray_tracing.f90:62), builds the blocks in `blk`, runs work(block) for each on a host thread of its own and joins
// them.  The first failing block in block order is the one reported.  The blocks stay with the caller, who may go on
// using their streams and buffers; they drain and release themselves when `blk` goes out of scope (RayBlock).
template <class Block, class Work>
static int run_blocks(const std::vector<int>& devs, int nray, std::deque<Block>* blk, Work work) {
  const int G = (int)devs.size();
  const int per = (nray + G - 1) / G;
  for (int g = 0; g < G; g++) {
    blk->emplace_back(g);
    Block& b = blk->back();
    b.dev = devs[g];
    b.r0 = std::min(nray, g * per);
    b.r1 = std::min(nray, (g + 1) * per);
  }
  std::vector<std::thread> th;
  for (Block& b : *blk)
    th.emplace_back([&work, &b] {
      b.rc = work(b);
      if (b.rc) b.err = g_err;  // (the message is this worker thread's)
    });
  for (auto& t : th) t.join();
  for (const Block& b : *blk)
    if (b.rc) {
      g_err = b.err;
      return b.rc;
    }
  return 0;
}
}  // extern "C++"

// The padded arrays are ~80 % zeros (a ray uses npoints of nstep_max+1 slots; 4.7 GB for the 64k
// fan, 0.82 GB of it data).  Pack on the device, copy the packed block through two pinned
// staging buffers, and scatter it into the caller's arrays with host threads while the next
// chunk is in flight.  Entries past npoints are not written: like the reference's trace_rays,
// which relies on initialize_ray_results_m having zero-filled the arrays (ray_results_m.f90:
// 154-164), this entry leaves them as the caller passed them.
// npoints: the block's counts on the host; host: the block's slabs of the caller's arrays.
static int copy_packed_to_host(const RayBlock& B, const rays_params_t* p, const int32_t* npoints,
                               const TrajectoryArrays& d, const TrajectoryArrays& host) {
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  const int slot = B.slot, n = B.n();
  const hipStream_t st = B.st();
  int32_t* const d_np = B.d.np;
  double *const d_rv = d.rv, *const d_res = d.res, *const ray_vec = host.rv, *const residual = host.res;
  std::vector<long long> offs((size_t)n + 1);
  offs[0] = 0;
  for (int i = 0; i < n; i++) offs[(size_t)i + 1] = offs[i] + (npoints[i] > 0 ? npoints[i] : 0);
  const long long total = offs[n];
  DeviceBuffers bufs(slot);
  long long* d_off = nullptr;
  double *d_pv = nullptr, *d_pr = nullptr;
  HIP_TRY_AS("hipMalloc(&d_off)", bufs.alloc(&d_off, (size_t)n + 1));
  if (total == 0) return 0;
  const auto failed = [] { return fail("rays_hip_trace: packed device-to-host copy failed (out of memory?)"); };
  EventPair ev;
  StagingBuffers* sb = nullptr;
  if (bufs.alloc(&d_pv, nv * (size_t)total) != hipSuccess || bufs.alloc(&d_pr, (size_t)total) != hipSuccess ||
      hipMemcpyAsync(d_off, offs.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      rays::launch_pack(true, n, (int)nv, p->nstep_max, d_np, d_off, d_rv, d_res, d_pv, d_pr, st) != hipSuccess ||
      !(sb = staging_for_slot(slot, nv, (long long)npt)) || ev.create() != hipSuccess)
    return failed();
  struct Chunk { int a, b, buf; };
  auto scatter = [&](const Chunk& c) {   // host side of one chunk: packed staging -> padded arrays
    const long long base = offs[c.a];
    const double* sv = sb->vec[c.buf];
    const double* sr = sb->res[c.buf];
    const int nt = 16;
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
      th.emplace_back([&, t]() {
        for (int i = c.a + t; i < c.b; i += nt) {
          const long long np_i = offs[(size_t)i + 1] - offs[i];
          if (np_i <= 0) continue;
          std::memcpy(ray_vec + npt * nv * (size_t)i, sv + (offs[i] - base) * (long long)nv,
                      sizeof(double) * nv * (size_t)np_i);
          std::memcpy(residual + npt * (size_t)i, sr + (offs[i] - base), sizeof(double) * (size_t)np_i);
        }
      });
    for (auto& x : th) x.join();
  };
  // chunks of rays whose packed size fits one staging buffer
  int buf = 0;
  Chunk pending{0, 0, -1};
  for (int c0 = 0; c0 < n;) {
    int c1 = c0;
    while (c1 < n && offs[(size_t)c1 + 1] - offs[c0] <= sb->points) c1++;
    if (c1 == c0) return failed();  // a ray has at most nstep_max+1 <= sb->points points (staging_for_slot)
    const long long pts = offs[c1] - offs[c0];
    if (pts > 0 &&
        (hipMemcpyAsync(sb->vec[buf], d_pv + offs[c0] * (long long)nv, sizeof(double) * nv * (size_t)pts,
                        hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipMemcpyAsync(sb->res[buf], d_pr + offs[c0], sizeof(double) * (size_t)pts, hipMemcpyDeviceToHost,
                        st) != hipSuccess ||
         hipEventRecord(ev[buf], st) != hipSuccess))
      return failed();
    if (pending.buf >= 0) scatter(pending);   // overlaps the copy just queued
    pending.buf = -1;
    if (pts > 0) {
      if (hipEventSynchronize(ev[buf]) != hipSuccess) return failed();
      pending = Chunk{c0, c1, buf};
      buf ^= 1;
    }
    c0 = c1;
  }
  if (pending.buf >= 0) scatter(pending);
  return 0;
}

// One device's share of rays_hip_trace: rays [r0, r1) -> contiguous slabs of the host arrays.
static int trace_block_on_device(RayBlock& B, const rays_params_t* p, const RayInputs& in, const TrajectoryArrays& traj,
                                 const SummaryArrays& out) {
  const int n = B.n(), r0 = B.r0;
  if (n <= 0) return 0;
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  const bool timing = std::getenv("RAYS_HIP_TIMING") != nullptr;  // phase times of this entry on stderr
  auto t_prev = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[rays_hip_trace dev %d] %-28s %8.2f ms\n", B.dev, what,
                 std::chrono::duration<double, std::milli>(now - t_prev).count());
    t_prev = now;
  };
  HIP_TRY_AS("hipSetDevice / hipStreamCreate", B.open());
  const hipStream_t st = B.st();
  lap("stream");
  TrajectoryArrays d;
  HIP_TRY_AS("hipMalloc (result arrays)", d.alloc(B.bufs, (size_t)n, npt, nv));
  HIP_TRY_AS("hipMalloc (result arrays)", B.d.alloc(B.bufs, (size_t)n, nv, false));
  lap("device allocations");
  HIP_TRY_AS("hipMalloc / hipMemcpyAsync (block inputs)", B.upload(in));
  // no zero-fill of the device arrays: only recorded points are read back
  int rc = launch_trace(p, KernelVariant::Recording, n, B.in, d, B.d, st, RAYS_TRACE_NO_ZERO_FILL);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out.np + r0, B.d.np, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  lap("inputs + trace kernel");
  rc = copy_packed_to_host(B, p, out.np + r0, d, {traj.rv + npt * nv * (size_t)r0, traj.res + npt * (size_t)r0});
  lap("pack + copy + host scatter");
  if (rc) return rc;
  SummaryArrays rest = out;  // (npoints is there already)
  rest.np = nullptr;
  HIP_TRY_AS("hipMemcpyAsync (summaries)", B.download(rest, nv));
  HIP_TRY(hipStreamSynchronize(st));
  lap("summaries");
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_kept.keep) {  // the slab and its counts stay on the device: theirs is the kept result now
      KeptBlock b;
      b.slot = B.slot; b.dev = B.dev; b.r0 = B.r0; b.r1 = B.r1;
      b.d_ray_vec = B.bufs.detach(d.rv);
      b.d_npoints = B.bufs.detach(B.d.np);
      g_kept.blocks.push_back(b);
    }
  }
  B.bufs.release();
  lap("device frees");
  return 0;
}

int rays_hip_trace(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                   double* ray_vec, double* residual, int32_t* npoints, int32_t* stop_code,
                   double* end_ray_vec, double* end_residuals, double* max_residuals,
                   double* elapsed_s) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (nray < 0) return fail("rays_hip_trace: nray < 0");
  if (nray > 0 && (!rvec0 || !rindex_vec0 || !ray_vec || !residual || !npoints || !stop_code))
    return fail("rays_hip_trace: null array argument");
  std::vector<int> devs;
  bool explicit_list = false;
  if (call_devices(&devs, &explicit_list)) return 3;
  {
    // Large fans: several slots per device, so that one slot's packed device-to-host copy (what bounds this
    // entry: 0.8 GB at ~50 GB/s for the 64k fan) runs while the other slots still trace.  Measured on the 64k
    // fan: 22.0 ms with one slot, 20.9 / 18.8 / 21.0 ms with 2 / 4 / 8.  RAYS_HIP_SLOTS_PER_DEVICE overrides;
    // a list given through rays_hip_init_devices is taken as it is.
    int k = (long long)nray >= 32768ll * (long long)devs.size() ? 4 : 1;
    if (const char* e = std::getenv("RAYS_HIP_SLOTS_PER_DEVICE")) k = std::atoi(e);
    while (k > 1 && (size_t)k * devs.size() > (size_t)kMaxDevices) k--;
    if (!explicit_list && k > 1) {
      std::vector<int> slots;
      for (int d : devs)
        for (int i = 0; i < k; i++) slots.push_back(d);
      devs.swap(slots);
    }
  }
  drop_kept_result();  // the image of an earlier call (if any) goes back to the block cache
  const auto t0 = std::chrono::steady_clock::now();
  std::deque<RayBlock> blk;
  rc = run_blocks(devs, nray, &blk, [&](RayBlock& B) {
    return trace_block_on_device(B, p, {rvec0, rindex_vec0}, {ray_vec, residual},
                                 {npoints, stop_code, nullptr, end_ray_vec, end_residuals, max_residuals});
  });
  if (rc) {
    drop_kept_result();
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_kept.keep) {
      std::sort(g_kept.blocks.begin(), g_kept.blocks.end(), [](const KeptBlock& a, const KeptBlock& b) { return a.r0 < b.r0; });
      g_kept.nray = nray;
      g_kept.nv = p->nv;
      g_kept.nstep_max = p->nstep_max;
    }
  }
  if (elapsed_s)
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// The host form of summary-only tracing: sharded like rays_hip_trace (contiguous blocks, one thread per device of
// rays_hip_init[_devices]; one slot per device -- there is no large copy for further slots to overlap).  Only the
// summaries exist on the device and cross PCIe.
int rays_hip_trace_summary(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                           int32_t* npoints, int32_t* stop_code, double* start_ray_vec, double* end_ray_vec,
                           double* end_residuals, double* max_residuals, double* elapsed_s) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (nray < 0) return fail("rays_hip_trace_summary: nray < 0");
  if (nray > 0 && (!rvec0 || !rindex_vec0 || !npoints || !stop_code || !end_ray_vec || !end_residuals || !max_residuals))
    return fail("rays_hip_trace_summary: null array argument");
  std::vector<int> devs;
  if (call_devices(&devs)) return 3;
  drop_kept_result();  // the image of an earlier rays_hip_trace (if any) is not this call's result: it goes back
  const auto t0 = std::chrono::steady_clock::now();
  const SummaryArrays out = {npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals};
  std::deque<RayBlock> blk;
  rc = run_blocks(devs, nray, &blk, [&](RayBlock& B) {
    if (B.n() <= 0) return 0;
    HIP_TRY_AS("hipSetDevice / hipStreamCreate", B.open());
    HIP_TRY_AS("hipMalloc (result arrays)", B.d.alloc(B.bufs, (size_t)B.n(), (size_t)p->nv, start_ray_vec != nullptr));
    HIP_TRY_AS("hipMalloc / hipMemcpyAsync (block inputs)", B.upload({rvec0, rindex_vec0}));
    const int rc_b = launch_trace(p, KernelVariant::Summary, B.n(), B.in, {}, B.d, B.st(), RAYS_TRACE_NO_ZERO_FILL);
    if (rc_b) return rc_b;
    HIP_TRY_AS("hipMemcpyAsync (summaries)", B.download(out, (size_t)p->nv));
    HIP_TRY(hipStreamSynchronize(B.st()));
    B.bufs.release();
    return 0;
  });
  if (rc) return rc;
  if (elapsed_s)
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// The host form of windowed tracing: the outputs of rays_hip_trace, bit for bit, with device memory bounded by the ray
// state plus two window slabs whatever nstep_max is.  One device (the first slot of the device list).  Window k is
// copied out -- whole slabs through the slot's pinned staging, on a copy stream of the call's own -- and scattered
// into the caller's arrays while window k + 1 runs.  A ray under way records exactly n_steps points per window, so the
// fan has ended when no ray of a window did; the window launched ahead of that test finds every ray ended and changes
// nothing.
int rays_hip_trace_windowed(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                            int n_steps, double* ray_vec, double* residual, int32_t* npoints, int32_t* stop_code,
                            double* end_ray_vec, double* end_residuals, double* max_residuals, double* elapsed_s) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (nray < 0) return fail("rays_hip_trace_windowed: nray < 0");
  if (n_steps < 1) return fail("rays_hip_trace_windowed: n_steps < 1");
  if (nray > 0 && (!rvec0 || !rindex_vec0 || !ray_vec || !residual || !npoints || !stop_code))
    return fail("rays_hip_trace_windowed: null array argument");
  if ((long long)nray * n_steps > 0x7fffffffll) return fail("rays_hip_trace_windowed: nray * n_steps exceeds 2^31 - 1");
  std::vector<int> devs;
  if (call_devices(&devs)) return 3;
  devs.resize(1);
  drop_kept_result();  // the image of an earlier rays_hip_trace (if any) is not this call's result: it goes back
  const auto t0 = std::chrono::steady_clock::now();
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv, W = (size_t)n_steps;
  std::deque<RayBlock> blk;
  rc = run_blocks(devs, nray, &blk, [&](RayBlock& B) {
    const int n = B.n();
    if (n <= 0) return 0;
    const size_t N = (size_t)n;
    HIP_TRY_AS("hipSetDevice / hipStreamCreate", B.open());
    const hipStream_t st = B.st();
    SlotStream copy_stream;
    HIP_TRY_AS("hipStreamCreate", copy_stream.open(kNoSlot));
    const hipStream_t cs = copy_stream.get();
    EventPair traced, copied;
    HIP_TRY_AS("hipEventCreate", traced.create());
    HIP_TRY_AS("hipEventCreate", copied.create());
    rays_ray_state_t S = {};
    TrajectoryArrays slab[2];
    int32_t* d_npw[2] = {nullptr, nullptr};
    const auto alloc_all = [&] {
      hipError_t e = B.bufs.alloc(&S.v, nv * N);
      if (e == hipSuccess) e = B.bufs.alloc(&S.s, N);
      if (e == hipSuccess) e = B.bufs.alloc(&S.nstep, N);
      if (e == hipSuccess) e = B.bufs.alloc(&S.stop_code, N);
      if (e == hipSuccess) e = B.bufs.alloc(&S.resid, 3 * N);
      if (e == hipSuccess) e = B.bufs.alloc(&S.sg_err, 2 * N);
      if (e == hipSuccess) e = B.bufs.alloc(&S.flags, N);
      for (int b = 0; b < 2 && e == hipSuccess; b++) {
        e = slab[b].alloc(B.bufs, N, W, nv);
        if (e == hipSuccess) e = B.bufs.alloc(&d_npw[b], N);
      }
      return e == hipSuccess ? B.d.alloc(B.bufs, N, nv, true) : e;
    };
    HIP_TRY_AS("hipMalloc (ray state, window slabs)", alloc_all());
    HIP_TRY_AS("hipMalloc / hipMemcpyAsync (block inputs)", B.upload({rvec0, rindex_vec0}));
    StagingBuffers* sb = staging_for_slot(B.slot, nv, (long long)(N * W));
    if (!sb) return fail("rays_hip_trace_windowed: pinned staging buffers could not be allocated");
    int rc_b = rays_hip_state_init_device(p, n, B.in.rvec0, B.in.rindex_vec0, &S, B.d.sv, st);
    if (rc_b) return rc_b;
    // point 1 of every ray: the start vector, residual 0
    std::vector<double> start(nv * N);
    HIP_TRY(hipMemcpyAsync(start.data(), B.d.sv, sizeof(double) * nv * N, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < N; i++) {
      std::memcpy(ray_vec + npt * nv * (i + (size_t)B.r0), start.data() + nv * i, sizeof(double) * nv);
      residual[npt * (i + (size_t)B.r0)] = 0.;
    }
    std::vector<int32_t> npw[2] = {std::vector<int32_t>(N), std::vector<int32_t>(N)};
    std::vector<int32_t> have(N, 1);  // points of each ray in the caller's arrays so far
    const auto launch = [&](int b) {
      const int r = rays_hip_trace_window_device(p, n, &S, n_steps, slab[b].rv, slab[b].res, d_npw[b], st);
      if (r) return r;
      HIP_TRY(hipEventRecord(traced[b], st));
      return 0;
    };
    rc_b = launch(0);
    if (rc_b) return rc_b;
    for (int k = 0;; k++) {
      const int b = k & 1;
      // window k: slab -> pinned staging on the copy stream, once its kernel has ended
      HIP_TRY(hipEventSynchronize(traced[b]));
      HIP_TRY(hipMemcpyAsync(sb->vec[b], slab[b].rv, sizeof(double) * nv * N * W, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(sb->res[b], slab[b].res, sizeof(double) * N * W, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(npw[b].data(), d_npw[b], sizeof(int32_t) * N, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipEventRecord(copied[b], cs));
      // window k + 1 into the other slab, whose copy (window k - 1) the host has already waited for
      rc_b = launch(b ^ 1);
      if (rc_b) return rc_b;
      HIP_TRY(hipEventSynchronize(copied[b]));
      bool any_full = false;
      const int nt = 16;
      std::vector<std::thread> th;
      for (int t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
          for (size_t i = (size_t)t; i < N; i += (size_t)nt) {
            const size_t m = (size_t)npw[b][i];
            if (m == 0) continue;
            const size_t ray = i + (size_t)B.r0, at = (size_t)have[i];
            std::memcpy(ray_vec + (npt * ray + at) * nv, sb->vec[b] + i * W * nv, sizeof(double) * nv * m);
            std::memcpy(residual + npt * ray + at, sb->res[b] + i * W, sizeof(double) * m);
            have[i] += (int32_t)m;
          }
        });
      for (auto& x : th) x.join();
      for (size_t i = 0; i < N; i++) any_full = any_full || npw[b][i] == n_steps;
      if (!any_full) break;
    }
    rc_b = rays_hip_state_summary_device(p, n, &S, B.d.np, B.d.sc, B.d.ev, B.d.er, B.d.mr, st);
    if (rc_b) return rc_b;
    SummaryArrays out = {npoints, stop_code, nullptr, end_ray_vec, end_residuals, max_residuals};
    HIP_TRY_AS("hipMemcpyAsync (summaries)", B.download(out, nv));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipStreamSynchronize(cs));
    B.bufs.release();
    return 0;
  });
  if (rc) return rc;
  if (elapsed_s)
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

int rays_hip_keep_last_result(int on) {
  if (std::getenv("RAYS_HIP_NO_KEEP_LAST_RESULT")) on = 0;  // measurement switch: A/B against the host-array path
  bool was;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    was = g_kept.keep;
    g_kept.keep = on != 0;
  }
  if (!on) drop_kept_result();
  return was ? 1 : 0;
}

int rays_hip_pack_device(int nray, int nv, int nstep_max, const int32_t* d_npoints,
                         const int64_t* d_offsets, const double* d_ray_vec, const double* d_residual,
                         double* d_packed_vec, double* d_packed_res, void* hip_stream) {
  hipError_t e = rays::launch_pack(true, nray, nv, nstep_max, d_npoints, (const long long*)d_offsets,
                                   const_cast<double*>(d_ray_vec), const_cast<double*>(d_residual),
                                   d_packed_vec, d_packed_res, (hipStream_t)hip_stream);
  return e == hipSuccess ? 0 : hip_fail(e, "rays_hip_pack_device");
}

int rays_hip_unpack_device(int nray, int nv, int nstep_max, const int32_t* d_npoints,
                           const int64_t* d_offsets, const double* d_packed_vec,
                           const double* d_packed_res, double* d_ray_vec, double* d_residual,
                           void* hip_stream) {
  hipError_t e = rays::launch_pack(false, nray, nv, nstep_max, d_npoints, (const long long*)d_offsets,
                                   d_ray_vec, d_residual, const_cast<double*>(d_packed_vec),
                                   const_cast<double*>(d_packed_res), (hipStream_t)hip_stream);
  return e == hipSuccess ? 0 : hip_fail(e, "rays_hip_unpack_device");
}

int rays_hip_set_rho_table(const double* grid, const double* fspl, int n) {
  if (!grid || !fspl || n < 2) return fail("rays_hip_set_rho_table: bad table");
  std::lock_guard<std::mutex> lk(g_mu);
  g_rho.host.assign(grid, grid + n);
  g_rho.host.insert(g_rho.host.end(), fspl, fspl + 4 * (size_t)n);
  g_rho.n = n;
  g_rho.version++;
  return 0;
}

// deposit_rays_kernel keeps 64 rows of n_bins doubles in LDS (rays_deposition.hip): 320 bins are the 160 KB of a CU
static int refuse_bin_count(int n_bins) {
  if (n_bins > RAYS_DEP_MAX_BINS)
    return fail("rays_hip_deposition: n_bins = " + std::to_string(n_bins) + " exceeds the limit of " +
                std::to_string(RAYS_DEP_MAX_BINS) + " bins (RAYS_DEP_MAX_BINS: one wave's rows must fit in 160 KB of LDS)");
  return 0;
}

// What a deposition may be asked for: rays_hip_check_params, then the checks rays_hip_deposition_device and the fused
// entries share.  `who` names the entry in the messages of its own; `fused` selects the fused entries' wording and
// order (their nray and bin count checks; rays_hip_deposition_device checks its own, behind these).
static int refuse_deposition(const char* who, bool fused, const rays_params_t* p, int nray, int which, int n_bins) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  const std::string w(who);
  if (fused && nray < 0) return fail(w + ": nray < 0");
  if (p->equilib_model != RAYS_EQ_AXISYM && p->equilib_model != RAYS_EQ_SLAB)  // deposition_profiles_m.f90:129-222
    return fail("initialize_deposition_profiles: unimplemented equilib_model");
  if (p->nv < 8 || p->damping_model == RAYS_DAMP_NONE)
    return fail(w + ": needs a run with damping (ray_vec(8) = absorbed power fraction)");
  if (p->equilib_model == RAYS_EQ_AXISYM && p->axisym.magnetics_model != RAYS_AXI_MAG_EQDSK_SPLINE && which == RAYS_DEP_PTOTAL_RHO)
    return fail("axisym_toroid_rho: rho is only implemented for eqdsk_magnetics_spline_interp");  // axisym_toroid_eq_m.f90:398-430
  if (p->equilib_model == RAYS_EQ_SLAB ? which != RAYS_DEP_PTOTAL_X
                                       : (which != RAYS_DEP_PTOTAL_PSI && which != RAYS_DEP_PTOTAL_RHO))
    return fail("initialize_deposition_profiles: unimplemented profile for this equilib_model");  // :162-169, 204-212
  if (!fused) {
    if (n_bins < 1 || nray < 0) return fail("rays_hip_deposition: bad n_bins / nray");
    return refuse_bin_count(n_bins);
  }
  if (n_bins < 1 || n_bins > RAYS_DEP_MAX_BINS)
    return fail(w + ": n_bins = " + std::to_string(n_bins) + " is outside 1.." + std::to_string(RAYS_DEP_MAX_BINS) +
                " (RAYS_DEP_MAX_BINS)");
  return 0;
}

int rays_hip_deposition_device(const rays_params_t* p, int which, int n_bins, int nray, const double* d_ray_vec,
                               const int32_t* d_npoints, const double* d_initial_ray_power, double* d_work,
                               const double* d_profile_in, double* d_profile_out, void* hip_stream) {
  int rc = refuse_deposition("rays_hip_deposition", false, p, nray, which, n_bins);
  if (rc) return rc;
  if (!d_ray_vec || !d_npoints || !d_initial_ray_power || !d_work || !d_profile_out)
    return fail("rays_hip_deposition: null device pointer");
  rays::DevParams D;
  rc = dev_params_with_axisym(p, &D);
  if (rc) return rc;
  rays::DepArgs A;
  A.which = which;
  A.n_bins = n_bins; A.nray = nray; A.nv = p->nv; A.npt = p->nstep_max + 1;
  A.ray_vec = d_ray_vec; A.npoints = d_npoints; A.power = d_initial_ray_power; A.work = d_work;
  rc = fill_deposition_grid(p, which, &A);
  if (rc) return rc;
  hipError_t e = rays::launch_deposition(D, A, d_profile_in, d_profile_out, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_fail(e, "deposition kernels");
  return 0;
}

// The device's work[n_bins][n] as n rows of the reference's work(n_bins, nray) = C [nray][n_bins]
static hipError_t work_to_host(const double* d_work, int n_bins, int n, double* work_rows, std::vector<double>* wbuf) {
  wbuf->resize((size_t)n_bins * (size_t)n);
  const hipError_t e = hipMemcpy(wbuf->data(), d_work, sizeof(double) * wbuf->size(), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  for (int r = 0; r < n; r++)
    for (int b = 0; b < n_bins; b++) work_rows[(size_t)r * n_bins + b] = (*wbuf)[(size_t)b * n + r];
  return hipSuccess;
}

// Host-pointer form of the deposition profiles: what a Fortran post-processor holding the ray_results_m arrays
// calls instead of calculate_deposition_profiles (deposition_profiles_m.f90:228-260).  Only points 1..maxval(npoints)
// of every ray cross PCIe (a strided copy); work comes back in the reference's work(n_bins, nray) layout.
int rays_hip_deposition(const rays_params_t* p, int which, int n_bins, int nray, const double* ray_vec,
                        const int32_t* npoints, const double* initial_ray_power, double* work, double* profile) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (n_bins < 1 || nray < 0) return fail("rays_hip_deposition: bad n_bins / nray");
  if (refuse_bin_count(n_bins)) return 1;
  if (nray == 0) {
    if (profile) std::memset(profile, 0, sizeof(double) * (size_t)n_bins);
    return 0;
  }
  if (!ray_vec || !npoints || !initial_ray_power || !profile) return fail("rays_hip_deposition: null array argument");
  const size_t nv = (size_t)p->nv, npt = (size_t)p->nstep_max + 1;
  int maxnp = 1;
  for (int i = 0; i < nray; i++) maxnp = std::max(maxnp, (int)npoints[i]);
  if ((size_t)maxnp > npt) return fail("rays_hip_deposition: npoints exceeds nstep_max + 1");
  const bool timing = std::getenv("RAYS_HIP_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  rays_params_t q = *p;
  q.nstep_max = maxnp - 1;  // the device copy holds maxnp points per ray
  DeviceBuffers bufs;
  double *d_rv = nullptr, *d_pw = nullptr, *d_work = nullptr, *d_prof = nullptr;
  int32_t* d_np = nullptr;
  HIP_TRY_AS("hipMalloc(&d_rv)", bufs.alloc(&d_rv, nv * (size_t)maxnp * (size_t)nray));
  HIP_TRY_AS("hipMalloc(&d_pw)", bufs.alloc(&d_pw, (size_t)nray));
  HIP_TRY_AS("hipMalloc(&d_work)", bufs.alloc(&d_work, (size_t)n_bins * (size_t)nray));
  HIP_TRY_AS("hipMalloc(&d_prof)", bufs.alloc(&d_prof, (size_t)n_bins));
  HIP_TRY_AS("hipMalloc(&d_np)", bufs.alloc(&d_np, (size_t)nray));
  HIP_TRY(hipMemcpy2D(d_rv, sizeof(double) * nv * (size_t)maxnp, ray_vec, sizeof(double) * nv * npt,
                      sizeof(double) * nv * (size_t)maxnp, (size_t)nray, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_pw, initial_ray_power, sizeof(double) * (size_t)nray, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_np, npoints, sizeof(int32_t) * (size_t)nray, hipMemcpyHostToDevice));
  rc = rays_hip_deposition_device(&q, which, n_bins, nray, d_rv, d_np, d_pw, d_work, nullptr, d_prof, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(profile, d_prof, sizeof(double) * (size_t)n_bins, hipMemcpyDeviceToHost));
  std::vector<double> wbuf;
  if (work) HIP_TRY_AS("hipMemcpy (work)", work_to_host(d_work, n_bins, nray, work, &wbuf));
  bufs.release();
  if (timing)
    std::fprintf(stderr, "[rays_hip_deposition] %d rays, %.1f MB of trajectories uploaded: %.2f ms\n", nray,
                 1e-6 * sizeof(double) * nv * (double)maxnp * (double)nray,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}

// The ray-ordered carry of the profiles of a call's blocks: blocks are binned in ray order, each continuing the running
// sums of the one before it (rays_hip_deposition_device's d_profile_in), so the profile is the reference's ray-ordered
// sum bit for bit, whatever the number of blocks / devices.  sum_block(block, scratch, carry_in, carry_out, &d_work), on
// the block's device: sums the block's rows onto carry_in (host; null for the first block) into carry_out (host), returns
// when carry_out is there, and names the block's work[n_bins][n] on the device; `scratch` lives until work is copied.
extern "C++" {
template <class Blocks, class SumBlock>
static int chain_profiles(Blocks& blocks, int n_bins, double* work, double* profile, SumBlock sum_block) {
  std::vector<double> carry((size_t)n_bins, 0.0), wbuf;
  bool have_carry = false;
  CurrentDevice restore;
  for (auto& b : blocks) {
    const int n = b.r1 - b.r0;
    if (n <= 0) continue;
    HIP_TRY(hipSetDevice(b.dev));
    DeviceBuffers scratch;
    const double* d_work = nullptr;
    const int rc = sum_block(b, scratch, have_carry ? carry.data() : nullptr, carry.data(), &d_work);
    if (rc) return rc;
    have_carry = true;
    if (work) HIP_TRY_AS("hipMemcpy (work)", work_to_host(d_work, n_bins, n, work + (size_t)b.r0 * n_bins, &wbuf));
  }
  std::memcpy(profile, carry.data(), sizeof(double) * (size_t)n_bins);
  return 0;
}
}  // extern "C++"

// The deposition profiles of the rays the last rays_hip_trace call traced, binned where they lie (see KeptResult).
int rays_hip_deposition_last(const rays_params_t* p, int which, int n_bins, int nray, const double* initial_ray_power,
                             double* work, double* profile) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (n_bins < 1 || nray < 0 || !initial_ray_power || !profile) return fail("rays_hip_deposition_last: bad argument");
  if (refuse_bin_count(n_bins)) return 1;
  std::vector<KeptBlock> blocks;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_kept.keep || g_kept.blocks.empty() || g_kept.nray != nray || g_kept.nv != p->nv || g_kept.nstep_max != p->nstep_max) {
      g_err = "rays_hip_deposition_last: no device-resident result of a rays_hip_trace call with this shape "
              "(rays_hip_keep_last_result(1) before the trace; same nray, nv, nstep_max)";
      return RAYS_HIP_NO_KEPT_RESULT;
    }
    blocks = g_kept.blocks;
  }
  const bool timing = std::getenv("RAYS_HIP_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t B = (size_t)n_bins;
  rc = chain_profiles(blocks, n_bins, work, profile, [&](const KeptBlock& b, DeviceBuffers& bufs, const double* carry_in,
                                                         double* carry_out, const double** d_work_out) {
    const int n = b.r1 - b.r0;
    double *d_pw = nullptr, *d_work = nullptr, *d_in = nullptr, *d_out = nullptr;
    HIP_TRY_AS("hipMalloc(&d_pw)", bufs.alloc(&d_pw, (size_t)n));
    HIP_TRY_AS("hipMalloc(&d_work)", bufs.alloc(&d_work, B * (size_t)n));
    HIP_TRY_AS("hipMalloc(&d_in)", bufs.alloc(&d_in, B));
    HIP_TRY_AS("hipMalloc(&d_out)", bufs.alloc(&d_out, B));
    HIP_TRY(hipMemcpy(d_pw, initial_ray_power + b.r0, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    if (carry_in) HIP_TRY(hipMemcpy(d_in, carry_in, sizeof(double) * B, hipMemcpyHostToDevice));
    const int rc_b = rays_hip_deposition_device(p, which, n_bins, n, b.d_ray_vec, b.d_npoints, d_pw, d_work,
                                                carry_in ? d_in : nullptr, d_out, nullptr);
    if (rc_b) return rc_b;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(carry_out, d_out, sizeof(double) * B, hipMemcpyDeviceToHost));
    *d_work_out = d_work;
    return 0;
  });
  if (rc) return rc;
  if (timing)
    std::fprintf(stderr, "[rays_hip_deposition_last] %d rays in %zu device-resident block(s), no trajectory upload: %.2f ms\n",
                 nray, blocks.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}

// ---- fused trace and deposition: the absorbed-power profile without trajectories (include/rays_hip.h) ---------------
// What the entries refuse before anything is allocated or launched; `who` names the entry in the messages of its own.
static int refuse_trace_deposition(const char* who, const rays_params_t* p, int nray, int which, int n_bins) {
  int rc = refuse_deposition(who, true, p, nray, which, n_bins);
  if (rc) return rc;
  if (which == RAYS_DEP_PTOTAL_RHO) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_rho.n < 2) return fail("Ptotal_rho needs rays_hip_set_rho_table() first");
  }
  if (!find_kernel(*p, nray, KernelVariant::Deposit) || !rays::launch_dep_trace_args || !rays::launch_profile_sum)
    return fail(std::string(who) + ": the fused deposition kernel of this configuration is not in this build");
  return 0;
}

// zero work, the DepTraceArgs block, the fused trace (in.power: the rays' initial power).  Arguments already checked.
// scan: nray = n_runs * scan->members rays, ray r * members + i being member i at step scan->ds_run[r]; its weights are
// tiled into the workspace behind the argument block.
static int trace_deposition_launch(const rays_params_t* p, int nray, const RayInputs& in, int which, int n_bins,
                                   const SummaryArrays& out, double* d_work, hipStream_t stream,
                                   const ScanPart* scan = nullptr) {
  rays::DepTraceArgs T;
  T.which = which;
  T.n_bins = n_bins;
  T.power = in.power;
  T.work = d_work;
  T.pad_ = 0;
  int rc = fill_deposition_grid(p, which, &T);
  if (rc) return rc;
  static_assert(sizeof(rays::DepTraceArgs) <= kDepArgsRoom, "the argument block fits its room");
  char* ws = nullptr;
  const size_t bytes = scan ? kDepArgsRoom + sizeof(double) * (size_t)nray : sizeof(rays::DepTraceArgs);
  HIP_TRY_AS("hipMalloc (deposition arguments)", g_dep_ws.get(stream, bytes, (void**)&ws));
  rays::DepTraceArgs* d_T = reinterpret_cast<rays::DepTraceArgs*>(ws);
  HIP_TRY(hipMemsetAsync(d_work, 0, sizeof(double) * (size_t)n_bins * (size_t)nray, stream));
  TraceExtras x;
  if (scan) {
    double* power_runs = reinterpret_cast<double*>(ws + kDepArgsRoom);
    const hipError_t et = rays::launch_tile_power(scan->members, nray, in.power, power_runs, stream);
    if (et != hipSuccess) return hip_fail(et, "power tiling kernel");
    T.power = power_runs;
    x.ds_run = scan->ds_run;
    x.rays_per_run = scan->members;
  }
  hipError_t e = rays::launch_dep_trace_args(T, d_T, stream);
  if (e != hipSuccess) return hip_fail(e, "deposition arguments kernel");
  x.dep = d_T;
  return launch_trace(p, KernelVariant::Deposit, nray, in, {}, out, stream, RAYS_TRACE_NO_ZERO_FILL, x);
}

int rays_hip_trace_deposition_device(const rays_params_t* p, int nray, const double* d_rvec0, const double* d_rindex_vec0,
                                     const double* d_initial_ray_power, int which, int n_bins, int32_t* d_npoints,
                                     int32_t* d_stop_code, double* d_start_ray_vec, double* d_end_ray_vec,
                                     double* d_end_residuals, double* d_max_residuals, double* d_work,
                                     const double* d_profile_in, double* d_profile_out, void* hip_stream) {
  if (!p) return fail("rays_hip_trace_deposition_device: null parameter block");
  int rc = refuse_trace_deposition("rays_hip_trace_deposition_device", p, nray, which, n_bins);
  if (rc) return rc;
  if (!d_profile_out) return fail("rays_hip_trace_deposition_device: null device pointer");
  const hipStream_t stream = (hipStream_t)hip_stream;
  if (nray == 0) {  // the sum over no rays: the carried profile, or zeros
    if (d_profile_in) {
      if (d_profile_in != d_profile_out)
        HIP_TRY(hipMemcpyAsync(d_profile_out, d_profile_in, sizeof(double) * (size_t)n_bins, hipMemcpyDeviceToDevice, stream));
    } else {
      HIP_TRY(hipMemsetAsync(d_profile_out, 0, sizeof(double) * (size_t)n_bins, stream));
    }
    return 0;
  }
  if (!d_rvec0 || !d_rindex_vec0 || !d_initial_ray_power || !d_npoints || !d_stop_code || !d_end_ray_vec ||
      !d_end_residuals || !d_max_residuals || !d_work)
    return fail("rays_hip_trace_deposition_device: null device pointer");
  rc = trace_deposition_launch(p, nray, {d_rvec0, d_rindex_vec0, d_initial_ray_power}, which, n_bins,
                               {d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals},
                               d_work, stream);
  if (rc) return rc;
  // + the ray-ordered profile sum
  const hipError_t e = rays::launch_profile_sum(n_bins, nray, d_work, d_profile_in, d_profile_out, stream);
  if (e != hipSuccess) return hip_fail(e, "profile sum kernel");
  return 0;
}

const char* rays_hip_deposition_kernel_name_for(const rays_params_t* p, int nray) {
  if (!p || rays_hip_check_params(p)) return "";
  const rays::KernelEntry* k = find_kernel(*p, nray, KernelVariant::Deposit);
  return k ? k->name : "";
}

namespace {
// A block of rays_hip_trace_deposition: work stays on the device (owned by the block's bufs) until the blocks' profiles
// have been chained in ray order.
struct DepositionBlock : RayBlock {
  using RayBlock::RayBlock;
  double *d_work = nullptr, *d_in = nullptr, *d_out = nullptr;
};
}  // namespace

// The host form: sharded like rays_hip_trace_summary (the devices of rays_hip_init[_devices], contiguous blocks, one
// thread per device, that entry's resource owners); then the blocks' rows are summed in ray order, each block continuing
// the running sums of the one before it, as rays_hip_deposition_last does.
int rays_hip_trace_deposition(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                              const double* initial_ray_power, int which, int n_bins, int32_t* npoints,
                              int32_t* stop_code, double* start_ray_vec, double* end_ray_vec, double* end_residuals,
                              double* max_residuals, double* work, double* profile, double* elapsed_s) {
  if (!p) return fail("rays_hip_trace_deposition: null parameter block");
  int rc = refuse_trace_deposition("rays_hip_trace_deposition", p, nray, which, n_bins);
  if (rc) return rc;
  if (!profile) return fail("rays_hip_trace_deposition: null array argument");
  if (nray > 0 && (!rvec0 || !rindex_vec0 || !initial_ray_power || !npoints || !stop_code || !end_ray_vec ||
                   !end_residuals || !max_residuals))
    return fail("rays_hip_trace_deposition: null array argument");
  std::vector<int> devs;
  if (call_devices(&devs)) return 3;
  drop_kept_result();  // the image of an earlier rays_hip_trace (if any) is not this call's result: it goes back
  const auto t0 = std::chrono::steady_clock::now();
  const SummaryArrays out = {npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals};
  const size_t nb = (size_t)n_bins;
  std::deque<DepositionBlock> blk;
  // every block traced and binned; the summaries go to the caller's arrays
  rc = run_blocks(devs, nray, &blk, [&](DepositionBlock& B) {
    if (B.n() <= 0) return 0;
    HIP_TRY_AS("hipSetDevice / hipStreamCreate", B.open());
    HIP_TRY_AS("hipMalloc (result arrays)", B.d.alloc(B.bufs, (size_t)B.n(), (size_t)p->nv, start_ray_vec != nullptr));
    HIP_TRY_AS("hipMalloc(&d_work)", B.bufs.alloc(&B.d_work, nb * (size_t)B.n()));
    HIP_TRY_AS("hipMalloc(&d_in)", B.bufs.alloc(&B.d_in, nb));
    HIP_TRY_AS("hipMalloc(&d_out)", B.bufs.alloc(&B.d_out, nb));
    HIP_TRY_AS("hipMalloc / hipMemcpyAsync (block inputs)", B.upload({rvec0, rindex_vec0, initial_ray_power}));
    const int rc_b = trace_deposition_launch(p, B.n(), B.in, which, n_bins, B.d, B.d_work, B.st());
    if (rc_b) return rc_b;
    HIP_TRY_AS("hipMemcpyAsync (summaries)", B.download(out, (size_t)p->nv));
    HIP_TRY(hipStreamSynchronize(B.st()));
    return 0;
  });
  if (rc) return rc;
  rc = chain_profiles(blk, n_bins, work, profile, [&](DepositionBlock& B, DeviceBuffers&, const double* carry_in,
                                                      double* carry_out, const double** d_work_out) {
    if (carry_in) HIP_TRY(hipMemcpyAsync(B.d_in, carry_in, sizeof(double) * nb, hipMemcpyHostToDevice, B.st()));
    const hipError_t e = rays::launch_profile_sum(n_bins, B.n(), B.d_work, carry_in ? B.d_in : nullptr, B.d_out, B.st());
    if (e != hipSuccess) return hip_fail(e, "profile sum kernel");
    HIP_TRY(hipMemcpyAsync(carry_out, B.d_out, sizeof(double) * nb, hipMemcpyDeviceToHost, B.st()));
    HIP_TRY(hipStreamSynchronize(B.st()));
    *d_work_out = B.d_work;
    return 0;
  });
  if (rc) return rc;
  if (elapsed_s)
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// ---- fused deposition into every profile of the equilibrium in one pass (include/rays_hip.h) --------------------------
int rays_hip_deposition_profile_set(const rays_params_t* p, int* which) {
  if (!p || !which || rays_hip_check_params(p)) return 0;
  if (p->equilib_model == RAYS_EQ_SLAB) {  // deposition_profiles_m.f90:129-160
    which[0] = RAYS_DEP_PTOTAL_X;
    return 1;
  }
  if (p->equilib_model != RAYS_EQ_AXISYM) return 0;
  which[0] = RAYS_DEP_PTOTAL_PSI;  // :162-222: Ptotal_psi, then Ptotal_rho where the equilibrium has rho
  if (p->axisym.magnetics_model != RAYS_AXI_MAG_EQDSK_SPLINE) return 1;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_rho.n < 2) return 1;
  }
  which[1] = RAYS_DEP_PTOTAL_RHO;
  return 2;
}

// What the two entries refuse before anything is allocated or launched: the single-profile entry's checks for each
// record, then the list's own.
static int refuse_trace_profiles(const char* who, const rays_params_t* p, int nray, int n_profiles,
                                 const rays_dep_profile_t* profiles) {
  const std::string w(who);
  if (!p) return fail(w + ": null parameter block");
  if (n_profiles < 1 || n_profiles > RAYS_DEP_MAX_PROFILES)
    return fail(w + ": n_profiles = " + std::to_string(n_profiles) + " is outside 1.." +
                std::to_string(RAYS_DEP_MAX_PROFILES) + " (RAYS_DEP_MAX_PROFILES)");
  if (!profiles) return fail(w + ": null profile list");
  for (int i = 0; i < n_profiles; i++) {
    const int rc = refuse_trace_deposition(who, p, nray, profiles[i].which, profiles[i].n_bins);
    if (rc) return rc;
  }
  if (n_profiles == 2) {
    if (profiles[0].which == profiles[1].which) return fail(w + ": the same profile twice");
    if (!find_kernel(*p, nray, KernelVariant::Deposit2) || !rays::launch_dep2_trace_args)
      return fail(w + ": the two-profile deposition kernel of this configuration is not in this build");
  }
  return 0;
}

// zero both work arrays, the Dep2TraceArgs block, the two-profile trace.  Arguments already checked.
static int trace_profiles_launch(const rays_params_t* p, int nray, const RayInputs& in, const rays_dep_profile_t* pr,
                                 double* const d_work[2], const SummaryArrays& out, hipStream_t stream,
                                 const ScanPart* scan = nullptr) {
  rays::Dep2TraceArgs T;
  T.power = in.power;
  T.rho_grid = nullptr; T.rho_fspl = nullptr; T.n_rho = 0; T.pad_ = 0;
  for (int i = 0; i < 2; i++) {
    rays::DepTraceArgs G;  // (the grid limits and the rho table of this record, as the single-profile launch takes them)
    const int rc = fill_deposition_grid(p, pr[i].which, &G);
    if (rc) return rc;
    T.prof[i].which = pr[i].which;
    T.prof[i].n_bins = pr[i].n_bins;
    T.prof[i].grid_min = G.grid_min;
    T.prof[i].grid_max = G.grid_max;
    T.prof[i].work = d_work[i];
    if (pr[i].which == RAYS_DEP_PTOTAL_RHO) { T.rho_grid = G.rho_grid; T.rho_fspl = G.rho_fspl; T.n_rho = G.n_rho; }
  }
  static_assert(sizeof(rays::Dep2TraceArgs) <= kDepArgsRoom, "the argument block fits its room");
  char* ws = nullptr;
  const size_t bytes = scan ? kDepArgsRoom + sizeof(double) * (size_t)nray : sizeof(rays::Dep2TraceArgs);
  HIP_TRY_AS("hipMalloc (deposition arguments)", g_dep2_ws.get(stream, bytes, (void**)&ws));
  rays::Dep2TraceArgs* d_T = reinterpret_cast<rays::Dep2TraceArgs*>(ws);
  for (int i = 0; i < 2; i++)
    HIP_TRY(hipMemsetAsync(d_work[i], 0, sizeof(double) * (size_t)pr[i].n_bins * (size_t)nray, stream));
  TraceExtras x;
  if (scan) {  // (as in trace_deposition_launch)
    double* power_runs = reinterpret_cast<double*>(ws + kDepArgsRoom);
    const hipError_t et = rays::launch_tile_power(scan->members, nray, in.power, power_runs, stream);
    if (et != hipSuccess) return hip_fail(et, "power tiling kernel");
    T.power = power_runs;
    x.ds_run = scan->ds_run;
    x.rays_per_run = scan->members;
  }
  const hipError_t e = rays::launch_dep2_trace_args(T, d_T, stream);
  if (e != hipSuccess) return hip_fail(e, "deposition arguments kernel");
  x.dep2 = d_T;
  return launch_trace(p, KernelVariant::Deposit2, nray, in, {}, out, stream, RAYS_TRACE_NO_ZERO_FILL, x);
}

int rays_hip_trace_profiles_device(const rays_params_t* p, int nray, const double* d_rvec0, const double* d_rindex_vec0,
                                   const double* d_initial_ray_power, int n_profiles, const rays_dep_profile_t* profiles,
                                   int32_t* d_npoints, int32_t* d_stop_code, double* d_start_ray_vec, double* d_end_ray_vec,
                                   double* d_end_residuals, double* d_max_residuals, void* hip_stream) {
  const char* who = "rays_hip_trace_profiles_device";
  int rc = refuse_trace_profiles(who, p, nray, n_profiles, profiles);
  if (rc) return rc;
  for (int i = 0; i < n_profiles; i++)
    if (!profiles[i].work || !profiles[i].profile) return fail(std::string(who) + ": null work or profile");
  if (n_profiles == 1)
    return rays_hip_trace_deposition_device(p, nray, d_rvec0, d_rindex_vec0, d_initial_ray_power, profiles[0].which,
                                            profiles[0].n_bins, d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec,
                                            d_end_residuals, d_max_residuals, profiles[0].work, profiles[0].profile_in,
                                            profiles[0].profile, hip_stream);
  const hipStream_t stream = (hipStream_t)hip_stream;
  if (nray == 0) {  // the sums over no rays: the carried profiles, or zeros
    for (int i = 0; i < 2; i++) {
      const size_t bytes = sizeof(double) * (size_t)profiles[i].n_bins;
      if (!profiles[i].profile_in) HIP_TRY(hipMemsetAsync(profiles[i].profile, 0, bytes, stream));
      else if (profiles[i].profile_in != profiles[i].profile)
        HIP_TRY(hipMemcpyAsync(profiles[i].profile, profiles[i].profile_in, bytes, hipMemcpyDeviceToDevice, stream));
    }
    return 0;
  }
  if (!d_rvec0 || !d_rindex_vec0 || !d_initial_ray_power || !d_npoints || !d_stop_code || !d_end_ray_vec ||
      !d_end_residuals || !d_max_residuals)
    return fail(std::string(who) + ": null device pointer");
  double* const d_work[2] = {profiles[0].work, profiles[1].work};
  rc = trace_profiles_launch(p, nray, {d_rvec0, d_rindex_vec0, d_initial_ray_power}, profiles, d_work,
                             {d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals},
                             stream);
  if (rc) return rc;
  for (int i = 0; i < 2; i++) {  // + the ray-ordered sums, each continued from its own carry
    const hipError_t e = rays::launch_profile_sum(profiles[i].n_bins, nray, profiles[i].work, profiles[i].profile_in,
                                                  profiles[i].profile, stream);
    if (e != hipSuccess) return hip_fail(e, "profile sum kernel");
  }
  return 0;
}

const char* rays_hip_profiles_kernel_name_for(const rays_params_t* p, int nray, int n_profiles) {
  if (!p || n_profiles < 1 || n_profiles > RAYS_DEP_MAX_PROFILES || rays_hip_check_params(p)) return "";
  const rays::KernelEntry* k = find_kernel(*p, nray, n_profiles == 2 ? KernelVariant::Deposit2 : KernelVariant::Deposit);
  return k ? k->name : "";
}

// ---- segmented deposition: the fused ds scan and one profile per beam (include/rays_hip.h) -----------
static int refuse_segments(const std::string& w, int n_seg, const int32_t* d_seg_offsets, int rays_per_seg) {
  if (n_seg < 0) return fail(w + ": n_seg < 0");
  if (n_seg > 0 && !d_seg_offsets && rays_per_seg < 1)
    return fail(w + ": neither segment offsets nor a positive rays_per_seg");
  if (!rays::launch_profile_sum_segments) return fail(w + ": the segmented profile sum is not in this build");
  return 0;
}

int rays_hip_profile_sum_segments_device(int n_bins, int nray, int n_seg, const int32_t* d_seg_offsets, int rays_per_seg,
                                         const double* d_work, const double* d_profile_in, double* d_profile_out,
                                         void* hip_stream) {
  const std::string w = "rays_hip_profile_sum_segments_device";
  if (n_bins < 1) return fail(w + ": n_bins < 1");
  if (nray < 0) return fail(w + ": nray < 0");
  const int rc = refuse_segments(w, n_seg, d_seg_offsets, rays_per_seg);
  if (rc) return rc;
  if (n_seg == 0) return 0;
  if ((nray > 0 && !d_work) || !d_profile_out) return fail(w + ": null work or profile");
  const hipError_t e = rays::launch_profile_sum_segments(n_bins, nray, n_seg, d_seg_offsets, rays_per_seg, d_work,
                                                         d_profile_in, d_profile_out, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_fail(e, "segmented profile sum kernel");
  return 0;
}

// The fused pass of one or two profiles over `total` rays -- a scan's n_runs * members, or a fan as it is -- and the sums
// per segment.  Arguments already checked.
static int trace_profiles_segments(const char* who, const rays_params_t* p, int total, const RayInputs& in, int n_profiles,
                                   const rays_dep_profile_t* profiles, const SummaryArrays& out, const ScanPart* scan,
                                   int n_seg, const int32_t* d_seg_offsets, int rays_per_seg, hipStream_t stream) {
  if (total > 0) {
    if (!in.rvec0 || !in.rindex_vec0 || !in.power || !out.np || !out.sc || !out.ev || !out.er || !out.mr)
      return fail(std::string(who) + ": null device pointer");
    int rc = 0;
    if (n_profiles == 1) {
      rc = trace_deposition_launch(p, total, in, profiles[0].which, profiles[0].n_bins, out, profiles[0].work, stream, scan);
    } else {
      double* const d_work[2] = {profiles[0].work, profiles[1].work};
      rc = trace_profiles_launch(p, total, in, profiles, d_work, out, stream, scan);
    }
    if (rc) return rc;
  }
  for (int i = 0; i < n_profiles; i++) {  // + the ray-ordered sums per segment, each continued from its own carry
    const hipError_t e = rays::launch_profile_sum_segments(profiles[i].n_bins, total, n_seg, d_seg_offsets, rays_per_seg,
                                                           profiles[i].work, profiles[i].profile_in, profiles[i].profile,
                                                           stream);
    if (e != hipSuccess) return hip_fail(e, "segmented profile sum kernel");
  }
  return 0;
}

int rays_hip_scan_profiles_device(const rays_params_t* p, int n_runs, const double* d_ds_values, int nray,
                                  const double* d_rvec0, const double* d_rindex_vec0, const double* d_initial_ray_power,
                                  int n_profiles, const rays_dep_profile_t* profiles, int32_t* d_npoints,
                                  int32_t* d_stop_code, double* d_start_ray_vec, double* d_end_ray_vec,
                                  double* d_end_residuals, double* d_max_residuals, void* hip_stream) {
  const char* who = "rays_hip_scan_profiles_device";
  const std::string w(who);
  int rc = refuse_trace_profiles(who, p, nray, n_profiles, profiles);
  if (rc) return rc;
  if (n_runs < 0) return fail(w + ": n_runs < 0");
  if ((long long)n_runs * nray > 0x7fffffffll) return fail(w + ": n_runs * nray exceeds 2^31 - 1");
  if (n_runs > 0 && !d_ds_values) return fail(w + ": null d_ds_values");
  rc = refuse_segments(w, n_runs, nullptr, nray > 0 ? nray : 1);
  if (rc) return rc;
  if (!rays::launch_tile_power) return fail(w + ": the power tiling kernel is not in this build");
  for (int i = 0; i < n_profiles; i++)
    if (!profiles[i].work || !profiles[i].profile) return fail(w + ": null work or profile");
  if (n_runs == 0) return 0;
  const int total = n_runs * nray;
  // (the kernel is chosen for the launch's ray count, not for one run's)
  if (total > 0 && !find_kernel(*p, total, n_profiles == 2 ? KernelVariant::Deposit2 : KernelVariant::Deposit))
    return fail(w + ": the fused deposition kernel of this configuration is not in this build");
  const ScanPart scan = {d_ds_values, nray};
  // (nray == 0: every run is an empty segment of no rays -- profile_in, or zeros)
  return trace_profiles_segments(who, p, total, {d_rvec0, d_rindex_vec0, d_initial_ray_power}, n_profiles, profiles,
                                 {d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals},
                                 &scan, n_runs, nullptr, nray > 0 ? nray : 1, (hipStream_t)hip_stream);
}

int rays_hip_trace_profiles_segments_device(const rays_params_t* p, int nray, const double* d_rvec0,
                                            const double* d_rindex_vec0, const double* d_initial_ray_power, int n_profiles,
                                            const rays_dep_profile_t* profiles, int n_seg, const int32_t* d_seg_offsets,
                                            int rays_per_seg, int32_t* d_npoints, int32_t* d_stop_code,
                                            double* d_start_ray_vec, double* d_end_ray_vec, double* d_end_residuals,
                                            double* d_max_residuals, void* hip_stream) {
  const char* who = "rays_hip_trace_profiles_segments_device";
  const std::string w(who);
  int rc = refuse_trace_profiles(who, p, nray, n_profiles, profiles);
  if (rc) return rc;
  rc = refuse_segments(w, n_seg, d_seg_offsets, rays_per_seg);
  if (rc) return rc;
  for (int i = 0; i < n_profiles; i++)
    if (!profiles[i].work || (n_seg > 0 && !profiles[i].profile)) return fail(w + ": null work or profile");
  return trace_profiles_segments(who, p, nray, {d_rvec0, d_rindex_vec0, d_initial_ray_power}, n_profiles, profiles,
                                 {d_npoints, d_stop_code, d_start_ray_vec, d_end_ray_vec, d_end_residuals, d_max_residuals},
                                 nullptr, n_seg, d_seg_offsets, rays_per_seg, (hipStream_t)hip_stream);
}

// ---- deposition windows: the fused kernels continued from a saved ray state (include/rays_hip.h) ----
// The rows of work are accumulators: nothing here zeroes them, so a sequence of windows performs the additions of one
// fused pass in the same order.  The argument block is written per call into the owner the one-shot entries use (one
// caller thread per (device, stream)).
int rays_hip_trace_window_profiles_device(const rays_params_t* p, int nray, const rays_ray_state_t* state, int n_steps,
                                          const double* d_initial_ray_power, int n_profiles,
                                          const rays_dep_profile_t* profiles, int32_t* d_npoints_win, void* hip_stream) {
  const char* who = "rays_hip_trace_window_profiles_device";
  int rc = refuse_trace_profiles(who, p, nray, n_profiles, profiles);
  if (rc) return rc;
  rc = refuse_state(who, p, nray, state);
  if (rc) return rc;
  if (n_steps < 1) return fail(std::string(who) + ": n_steps < 1");
  if (!d_npoints_win) return fail(std::string(who) + ": null device pointer");
  if ((long long)nray * n_steps > 0x7fffffffll) return fail(std::string(who) + ": nray * n_steps exceeds 2^31 - 1");
  if (!d_initial_ray_power) return fail(std::string(who) + ": null initial_ray_power");
  for (int i = 0; i < n_profiles; i++)
    if (!profiles[i].work) return fail(std::string(who) + ": null work");
  const KernelVariant variant = n_profiles == 2 ? KernelVariant::WindowDeposit2 : KernelVariant::WindowDeposit;
  if (!find_kernel(*p, nray, variant))
    return fail(std::string(who) + ": the deposition window kernel of this configuration is not in this build");
  if (nray == 0) return 0;
  const hipStream_t stream = (hipStream_t)hip_stream;
  const rays::TraceArgs::State st = state_of(state);
  TraceExtras x;
  x.state = &st;
  x.n_steps = n_steps;
  if (n_profiles == 1) {
    rays::DepTraceArgs T;
    T.which = profiles[0].which;
    T.n_bins = profiles[0].n_bins;
    T.power = d_initial_ray_power;
    T.work = profiles[0].work;
    T.pad_ = 0;
    rc = fill_deposition_grid(p, profiles[0].which, &T);
    if (rc) return rc;
    rays::DepTraceArgs* d_T = nullptr;
    HIP_TRY_AS("hipMalloc (deposition arguments)", g_dep_ws.get(stream, sizeof(rays::DepTraceArgs), (void**)&d_T));
    const hipError_t e = rays::launch_dep_trace_args(T, d_T, stream);
    if (e != hipSuccess) return hip_fail(e, "deposition arguments kernel");
    x.dep = d_T;
  } else {
    rays::Dep2TraceArgs T;
    T.power = d_initial_ray_power;
    T.rho_grid = nullptr; T.rho_fspl = nullptr; T.n_rho = 0; T.pad_ = 0;
    for (int i = 0; i < 2; i++) {
      rays::DepTraceArgs G;  // (the grid limits and the rho table of this record, as the single-profile launch takes them)
      rc = fill_deposition_grid(p, profiles[i].which, &G);
      if (rc) return rc;
      T.prof[i].which = profiles[i].which;
      T.prof[i].n_bins = profiles[i].n_bins;
      T.prof[i].grid_min = G.grid_min;
      T.prof[i].grid_max = G.grid_max;
      T.prof[i].work = profiles[i].work;
      if (profiles[i].which == RAYS_DEP_PTOTAL_RHO) { T.rho_grid = G.rho_grid; T.rho_fspl = G.rho_fspl; T.n_rho = G.n_rho; }
    }
    rays::Dep2TraceArgs* d_T = nullptr;
    HIP_TRY_AS("hipMalloc (deposition arguments)", g_dep2_ws.get(stream, sizeof(rays::Dep2TraceArgs), (void**)&d_T));
    const hipError_t e = rays::launch_dep2_trace_args(T, d_T, stream);
    if (e != hipSuccess) return hip_fail(e, "deposition arguments kernel");
    x.dep2 = d_T;
  }
  SummaryArrays out = {};
  out.np = d_npoints_win;
  rc = launch_trace(p, variant, nray, {nullptr, nullptr}, {}, out, stream, RAYS_TRACE_NO_ZERO_FILL, x);
  if (rc) return rc;
  for (int i = 0; i < n_profiles; i++) {  // + the ray-ordered sums over the work so far, where the caller wants them
    if (!profiles[i].profile) continue;
    const hipError_t e = rays::launch_profile_sum(profiles[i].n_bins, nray, profiles[i].work, profiles[i].profile_in,
                                                  profiles[i].profile, stream);
    if (e != hipSuccess) return hip_fail(e, "profile sum kernel");
  }
  return 0;
}

const char* rays_hip_window_profiles_kernel_name_for(const rays_params_t* p, int nray, int n_profiles) {
  if (!p || n_profiles < 1 || n_profiles > RAYS_DEP_MAX_PROFILES || rays_hip_check_params(p)) return "";
  const rays::KernelEntry* k =
      find_kernel(*p, nray, n_profiles == 2 ? KernelVariant::WindowDeposit2 : KernelVariant::WindowDeposit);
  return k ? k->name : "";
}

namespace {
// A block of rays_hip_trace_profiles: both work arrays stay on the device (owned by the block's bufs) until both
// profiles have been chained in ray order.
struct ProfilesBlock : RayBlock {
  using RayBlock::RayBlock;
  double *d_work[2] = {nullptr, nullptr}, *d_in[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
};
}  // namespace

int rays_hip_trace_profiles(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                            const double* initial_ray_power, int n_profiles, const rays_dep_profile_t* profiles,
                            int32_t* npoints, int32_t* stop_code, double* start_ray_vec, double* end_ray_vec,
                            double* end_residuals, double* max_residuals, double* elapsed_s) {
  const char* who = "rays_hip_trace_profiles";
  int rc = refuse_trace_profiles(who, p, nray, n_profiles, profiles);
  if (rc) return rc;
  for (int i = 0; i < n_profiles; i++) {
    if (profiles[i].profile_in) return fail(std::string(who) + ": profile_in is for the device form (the host form chains its own blocks)");
    if (!profiles[i].profile) return fail(std::string(who) + ": null array argument");
  }
  if (n_profiles == 1)
    return rays_hip_trace_deposition(p, nray, rvec0, rindex_vec0, initial_ray_power, profiles[0].which, profiles[0].n_bins,
                                     npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals,
                                     profiles[0].work, profiles[0].profile, elapsed_s);
  if (nray > 0 && (!rvec0 || !rindex_vec0 || !initial_ray_power || !npoints || !stop_code || !end_ray_vec ||
                   !end_residuals || !max_residuals))
    return fail(std::string(who) + ": null array argument");
  std::vector<int> devs;
  if (call_devices(&devs)) return 3;
  drop_kept_result();  // the image of an earlier rays_hip_trace (if any) is not this call's result: it goes back
  const auto t0 = std::chrono::steady_clock::now();
  const SummaryArrays out = {npoints, stop_code, start_ray_vec, end_ray_vec, end_residuals, max_residuals};
  std::deque<ProfilesBlock> blk;
  // every block traced and binned into its two work arrays; the summaries go to the caller's arrays
  rc = run_blocks(devs, nray, &blk, [&](ProfilesBlock& B) {
    if (B.n() <= 0) return 0;
    HIP_TRY_AS("hipSetDevice / hipStreamCreate", B.open());
    HIP_TRY_AS("hipMalloc (result arrays)", B.d.alloc(B.bufs, (size_t)B.n(), (size_t)p->nv, start_ray_vec != nullptr));
    for (int i = 0; i < 2; i++) {
      const size_t nb = (size_t)profiles[i].n_bins;
      HIP_TRY_AS("hipMalloc(&d_work)", B.bufs.alloc(&B.d_work[i], nb * (size_t)B.n()));
      HIP_TRY_AS("hipMalloc(&d_in)", B.bufs.alloc(&B.d_in[i], nb));
      HIP_TRY_AS("hipMalloc(&d_out)", B.bufs.alloc(&B.d_out[i], nb));
    }
    HIP_TRY_AS("hipMalloc / hipMemcpyAsync (block inputs)", B.upload({rvec0, rindex_vec0, initial_ray_power}));
    const int rc_b = trace_profiles_launch(p, B.n(), B.in, profiles, B.d_work, B.d, B.st());
    if (rc_b) return rc_b;
    HIP_TRY_AS("hipMemcpyAsync (summaries)", B.download(out, (size_t)p->nv));
    HIP_TRY(hipStreamSynchronize(B.st()));
    return 0;
  });
  if (rc) return rc;
  for (int i = 0; i < 2; i++) {  // each profile chained over the blocks in ray order, on this thread
    const int n_bins = profiles[i].n_bins;
    const size_t nb = (size_t)n_bins;
    rc = chain_profiles(blk, n_bins, profiles[i].work, profiles[i].profile,
                        [&](ProfilesBlock& B, DeviceBuffers&, const double* carry_in, double* carry_out,
                            const double** d_work_out) {
      if (carry_in) HIP_TRY(hipMemcpyAsync(B.d_in[i], carry_in, sizeof(double) * nb, hipMemcpyHostToDevice, B.st()));
      const hipError_t e = rays::launch_profile_sum(n_bins, B.n(), B.d_work[i], carry_in ? B.d_in[i] : nullptr, B.d_out[i], B.st());
      if (e != hipSuccess) return hip_fail(e, "profile sum kernel");
      HIP_TRY(hipMemcpyAsync(carry_out, B.d_out[i], sizeof(double) * nb, hipMemcpyDeviceToHost, B.st()));
      HIP_TRY(hipStreamSynchronize(B.st()));
      *d_work_out = B.d_work[i];
      return 0;
    });
    if (rc) return rc;
  }
  if (elapsed_s)
    *elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

int rays_hip_sizeof_fan(void) { return (int)sizeof(rays_fan_t); }

#include "rays_fan_setup.inc"

static int ray_init_run(const rays_params_t* p, const rays_fan_t* fan, int nray_max, double* d_rvec0,
                        double* d_rindex_vec0, int32_t* nray, hipStream_t stream,
                        std::vector<int>* first_of_launch_host, int* per_r_launch) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (!nray || !d_rvec0 || !d_rindex_vec0) return fail("rays_hip_ray_init: null pointer");
  rays::FanArgs F;
  std::vector<double> launch;
  const char* why = "";
  if (fan_setup(p, fan, nray_max, &F, &launch, per_r_launch, &why)) return fail(why);
  const int n_cand = F.n_launch * F.n_a * F.n_b;
  const int nb = (n_cand + rays::ray_init_block() - 1) / rays::ray_init_block();
  rays::DevParams D;
  rc = dev_params_with_axisym(p, &D);
  if (rc) return rc;
  DeviceBuffers bufs;
  double *d_launch = nullptr, *d_cand = nullptr;
  int *d_keep = nullptr, *d_bc = nullptr, *d_offs = nullptr, *d_first = nullptr;
  HIP_TRY_AS("hipMalloc(&d_launch)", bufs.alloc(&d_launch, launch.size()));
  HIP_TRY_AS("hipMalloc(&d_cand)", bufs.alloc(&d_cand, 3 * (size_t)n_cand));
  HIP_TRY_AS("hipMalloc(&d_keep)", bufs.alloc(&d_keep, (size_t)n_cand));
  HIP_TRY_AS("hipMalloc(&d_bc)", bufs.alloc(&d_bc, (size_t)nb));
  HIP_TRY_AS("hipMalloc(&d_offs)", bufs.alloc(&d_offs, (size_t)(nb + 1)));
  HIP_TRY_AS("hipMalloc(&d_first)", bufs.alloc(&d_first, (size_t)F.n_launch));
  HIP_TRY(hipMemcpyAsync(d_launch, launch.data(), sizeof(double) * launch.size(), hipMemcpyHostToDevice, stream));
  F.launch = d_launch;
  HIP_TRY(rays::launch_ray_init(p->equilib_model, p->nspec + 1, D, F, n_cand, d_cand, d_keep, d_bc, d_offs,
                                d_first, d_rvec0, d_rindex_vec0, stream));
  int total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_offs + nb, sizeof(int), hipMemcpyDeviceToHost, stream));
  if (first_of_launch_host) {
    first_of_launch_host->resize(F.n_launch);
    HIP_TRY(hipMemcpyAsync(first_of_launch_host->data(), d_first, sizeof(int) * F.n_launch, hipMemcpyDeviceToHost,
                           stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  *nray = total;
  if (total == 0) return fail("No successful ray initializations");  // simple_slab_ray_init_m.f90:172
  return 0;
}

int rays_hip_ray_init_device(const rays_params_t* p, const rays_fan_t* fan, int nray_max, double* d_rvec0,
                             double* d_rindex_vec0, int32_t* nray, void* hip_stream) {
  int per_r = 0;
  return ray_init_run(p, fan, nray_max, d_rvec0, d_rindex_vec0, nray, (hipStream_t)hip_stream, nullptr, &per_r);
}

int rays_hip_ray_init(const rays_params_t* p, const rays_fan_t* fan, int nray_max, double* rvec0,
                      double* rindex_vec0, double* ray_pwr_wt, int32_t* nray) {
  if (!rvec0 || !rindex_vec0 || !nray) return fail("rays_hip_ray_init: null pointer");
  if (nray_max <= 0) return fail("rays_hip_ray_init: nray_max <= 0");
  {  // configuration errors first (they need no device), as the reference's launchers `stop 1`
    int rc0 = rays_hip_check_params(p);
    if (rc0) return rc0;
    rays::FanArgs F;
    std::vector<double> launch;
    int per_r0 = 0;
    const char* why = "";
    if (fan_setup(p, fan, nray_max, &F, &launch, &per_r0, &why)) return fail(why);
  }
  DeviceBuffers bufs;
  double *d_r = nullptr, *d_n = nullptr;
  HIP_TRY_AS("hipMalloc(&d_r)", bufs.alloc(&d_r, 3 * (size_t)nray_max));
  if (bufs.alloc(&d_n, 3 * (size_t)nray_max) != hipSuccess) return fail("rays_hip_ray_init: out of device memory");
  std::vector<int> first;
  int per_r = 0;
  int rc = ray_init_run(p, fan, nray_max, d_r, d_n, nray, nullptr, &first, &per_r);
  if (rc) return rc;
  const size_t n = (size_t)*nray;
  hipError_t e = hipMemcpy(rvec0, d_r, sizeof(double) * 3 * n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(rindex_vec0, d_n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy (ray init results)");
  if (!ray_pwr_wt) return 0;
  if (fan->model == RAYS_RAY_INIT_SIMPLE_SLAB) {  // :179,182: 1/nray, divided by nray once more
    for (size_t i = 0; i < n; i++) ray_pwr_wt[i] = 1.0 / (double)n / (double)n;
  } else if (fan->model == RAYS_RAY_INIT_AXISYM_R_Z_NPHI_NTHETA) {
    for (size_t i = 0; i < n; i++) ray_pwr_wt[i] = 1.0 / (double)n;
  } else {
    // solovev_ray_init_nphi_ntheta_m.f90:196: only ray_pwr_wt(count) = 1. after each r-launch
    // loop, and the whole array divided by nray at the end (:206); the other entries are left
    // unset by the reference (zero here)
    for (size_t i = 0; i < n; i++) ray_pwr_wt[i] = 0.;
    const int nl = (int)first.size();
    for (int ir = 0; per_r > 0 && ir < nl / per_r; ir++) {
      const int end = (ir + 1) * per_r < nl ? first[(ir + 1) * per_r] : (int)n;  // count after this r loop
      if (end >= 1) ray_pwr_wt[end - 1] = 1. / (double)n;
    }
  }
  return 0;
}

// Diagnostic entry (tests): evaluate the RHS pieces at n states on the current device.
// v[n][nv] host; outputs host: cold7[n][7], num7[n][7], dvds[n][nv], resid[n], codes[n][4]
// (codes: equilibrium err, eqn_ray stop code, check_save flag, check_save stop_ode).
int rays_hip_probe(const rays_params_t* p, int n, const double* v, double* cold7, double* num7,
                   double* dvds, double* resid, int32_t* codes) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  // what probe_kernel (rays_probe.hip) evaluates: the nv = 7 rows of the three equilibria with two or three species --
  // any other shape returns from the kernel with nothing written
  if (p->nv != 7 || (p->nspec + 1 != 2 && p->nspec + 1 != 3) || p->equilib_model < 0 || p->equilib_model > 2) {
    char msg[200];
    std::snprintf(msg, sizeof msg, "rays_hip_probe: no kernel built for this configuration (equilibrium %d, %d species, "
                  "nv = %d): the probe evaluates nv = 7 with 2 or 3 species", p->equilib_model, p->nspec + 1, p->nv);
    return fail(msg);
  }
  if (n <= 0) return 0;
  if (!v || !cold7 || !num7 || !dvds || !resid || !codes) return fail("rays_hip_probe: null pointer");
  const size_t nv = (size_t)p->nv;
  DeviceBuffers bufs;
  double *d_v = nullptr, *d_c = nullptr, *d_n = nullptr, *d_f = nullptr, *d_r = nullptr;
  int* d_k = nullptr;
  HIP_TRY_AS("hipMalloc(&d_v)", bufs.alloc(&d_v, nv * n));
  HIP_TRY_AS("hipMalloc(&d_c)", bufs.alloc(&d_c, 7 * (size_t)n));
  HIP_TRY_AS("hipMalloc(&d_n)", bufs.alloc(&d_n, 7 * (size_t)n));
  HIP_TRY_AS("hipMalloc(&d_f)", bufs.alloc(&d_f, nv * n));
  HIP_TRY_AS("hipMalloc(&d_r)", bufs.alloc(&d_r, (size_t)n));
  HIP_TRY_AS("hipMalloc(&d_k)", bufs.alloc(&d_k, 4 * (size_t)n));
  HIP_TRY(hipMemcpy(d_v, v, sizeof(double) * nv * n, hipMemcpyHostToDevice));
  rays::DevParams D;
  rc = dev_params_with_axisym(p, &D);
  if (rc) return rc;
  hipLaunchKernelGGL(rays::probe_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, D, p->equilib_model,
                     p->nspec + 1, p->nv, n, d_v, d_c, d_n, d_f, d_r, d_k);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(cold7, d_c, sizeof(double) * 7 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(num7, d_n, sizeof(double) * 7 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dvds, d_f, sizeof(double) * nv * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(resid, d_r, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(codes, d_k, sizeof(int) * 4 * n, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

#include "rays_gather.inc"
static void rccl_close_all() { rccl_close(); }
