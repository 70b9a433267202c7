// rays_gather.inc -- multi-GPU trace with a device-resident result: the final trajectory gather over RCCL.
// Included by rays_capi.hip at file scope (after its extern "C" block).
//
// SURVEY.md 8(e): rays shard into contiguous blocks (the reference's OpenMP schedule(static),
// ray_tracing.f90:62-64); the only exchange is the gather of every block's trajectories to the root.  The
// blocks travel PACKED (a ray uses npoints of its nstep_max+1 slots), as one grouped batch of
// ncclSend/ncclRecv: every peer sends to the root over its own xGMI link, so the transfers are
// link-parallel.  RCCL is opened lazily with dlopen (librccl.so is 0.5 GB; a single-GPU process never
// loads it), one communicator per selected device, single process (ncclCommInitAll).
namespace {

typedef void* rccl_comm_t;
struct Rccl {
  void* lib = nullptr;
  int (*CommInitAll)(rccl_comm_t*, int, const int*) = nullptr;
  int (*CommDestroy)(rccl_comm_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::vector<int> devices;        // the device list the communicators were built for
  std::vector<rccl_comm_t> comms;  // comms[i] <-> devices[i]
};
Rccl g_rccl;
constexpr int kNcclInt32 = 2, kNcclDouble = 8;  // rccl.h: ncclInt32, ncclFloat64

int rccl_fail(int rc, const char* what) {
  g_err = std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
  return 4;
}
#define RCCL_TRY(call)                              \
  do {                                              \
    int r_ = (call);                                \
    if (r_ != 0) return rccl_fail(r_, #call);       \
  } while (0)

int rccl_open(const std::vector<int>& devs) {
  if (!g_rccl.lib) {
    // RAYS_HIP_RCCL_LIB: another build of the library (or, in the CPU test tier, tests/hip_emul's stand-in)
    const char* override_path = std::getenv("RAYS_HIP_RCCL_LIB");
    void* h = override_path ? dlopen(override_path, RTLD_NOW | RTLD_LOCAL) : dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h && !override_path) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(std::string("rays_hip_trace_gather: cannot load librccl.so: ") + dlerror());
    g_rccl.lib = h;
#define RCCL_SYM(field, name)                                                             \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name));                \
  if (!g_rccl.field) return fail(std::string("rays_hip_trace_gather: librccl.so lacks ") + name);
    RCCL_SYM(CommInitAll, "ncclCommInitAll")
    RCCL_SYM(CommDestroy, "ncclCommDestroy")
    RCCL_SYM(GroupStart, "ncclGroupStart")
    RCCL_SYM(GroupEnd, "ncclGroupEnd")
    RCCL_SYM(Send, "ncclSend")
    RCCL_SYM(Recv, "ncclRecv")
    RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef RCCL_SYM
  }
  if (g_rccl.devices != devs) {
    for (rccl_comm_t c : g_rccl.comms) (void)g_rccl.CommDestroy(c);
    g_rccl.comms.assign(devs.size(), nullptr);
    g_rccl.devices.clear();
    RCCL_TRY(g_rccl.CommInitAll(g_rccl.comms.data(), (int)devs.size(), devs.data()));
    g_rccl.devices = devs;
  }
  return 0;
}

void rccl_close() {
  for (rccl_comm_t c : g_rccl.comms)
    if (c && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c);
  g_rccl.comms.clear();
  g_rccl.devices.clear();
}

// One device's share: trace rays [r0, r1) into slabs on that device; peers also pack them.
struct GatherBlock : RayBlock {
  using RayBlock::RayBlock;  // (bufs: everything below but the root's slabs, which are the gathered result's)
  TrajectoryArrays t;
  long long* d_off = nullptr;
  double *d_pv = nullptr, *d_pr = nullptr;  // packed (peers: send buffers)
  std::vector<int32_t> np;                  // host copy of the block's npoints
  std::vector<long long> offs;
  long long total = 0;
};

// The gathered result: library-owned until the next rays_hip_trace_gather call / rays_hip_finalize
// (never destroyed: no HIP call may run during static destruction, when the runtime may be gone already)
DeviceBuffers& g_gathered = *new DeviceBuffers(kResultSlot);

// Phase 1 on one device (its own host thread): trace block g, slot g of the block cache.  A: the root's global arrays.
int gather_trace_block(GatherBlock& b, const SummaryArrays& A, const TrajectoryArrays& At, const rays_params_t* p,
                       int nray, const RayInputs& in) {
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  const int g = b.slot, n = b.n();
  // (slot g may hold another device's stream and blocks -- rays_hip_trace: slots per device; the stream is opened for an
  // empty block too: phase 2 runs on the root's)
  HIP_TRY_AS("hipSetDevice / hipStreamCreate", b.open());
  const hipStream_t st = b.st();
  if (n <= 0) return 0;
  if (g == 0) {  // the root traces straight into its slab of the global arrays
    b.d = A;
    b.t = At;
    HIP_TRY(hipMemsetAsync(At.rv, 0, sizeof(double) * npt * nv * (size_t)nray, st));  // ray_results_m.f90:154-164
    HIP_TRY(hipMemsetAsync(At.res, 0, sizeof(double) * npt * (size_t)nray, st));
  } else {
    HIP_TRY_AS("hipMalloc (result arrays)", b.t.alloc(b.bufs, (size_t)n, npt, nv));
    HIP_TRY_AS("hipMalloc (result arrays)", b.d.alloc(b.bufs, (size_t)n, nv, false));
  }
  HIP_TRY_AS("hipMalloc / hipMemcpyAsync (block inputs)", b.upload(in));
  const int rc = launch_trace(p, KernelVariant::Recording, n, b.in, b.t, b.d, st, RAYS_TRACE_NO_ZERO_FILL);
  if (rc || g == 0) return rc;
  // pack: the block's points back to back
  b.np.resize(n);
  HIP_TRY(hipMemcpyAsync(b.np.data(), b.d.np, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  b.offs.resize((size_t)n + 1);
  b.offs[0] = 0;
  for (int i = 0; i < n; i++) b.offs[(size_t)i + 1] = b.offs[i] + (b.np[i] > 0 ? b.np[i] : 0);
  b.total = b.offs[n];
  HIP_TRY_AS("hipMalloc(&b.d_off)", b.bufs.alloc(&b.d_off, (size_t)n + 1));
  HIP_TRY_AS("hipMalloc(&b.d_pv)", b.bufs.alloc(&b.d_pv, nv * (size_t)std::max(b.total, 1ll)));
  HIP_TRY_AS("hipMalloc(&b.d_pr)", b.bufs.alloc(&b.d_pr, (size_t)std::max(b.total, 1ll)));
  HIP_TRY(hipMemcpyAsync(b.d_off, b.offs.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(rays::launch_pack(true, n, (int)nv, p->nstep_max, b.d.np, b.d_off, b.t.rv, b.t.res, b.d_pv, b.d_pr, st));
  return 0;
}

// Phase 2, the gather.  One grouped batch: peer g sends on its stream, the root receives on its own (rs) into rx's
// buffers and unpacks them into the peers' slabs of the global arrays.  Asynchronous: the caller drains the streams.
int gather_to_root(const std::deque<GatherBlock>& blk, const SummaryArrays& A, const TrajectoryArrays& At,
                   const rays_params_t* p, int root, DeviceBuffers& rx) {
  const int G = (int)blk.size();
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  const hipStream_t rs = blk[0].st();
  std::vector<double*> rx_pv(G, nullptr), rx_pr(G, nullptr);
  std::vector<long long*> rx_off(G, nullptr);
  if (hipSetDevice(root) != hipSuccess) return fail("rays_hip_trace_gather: hipSetDevice(root)");
  for (int g = 1; g < G; g++) {
    const GatherBlock& b = blk[g];
    const int n = b.r1 - b.r0;
    if (n <= 0) continue;
    if (rx.alloc(&rx_pv[g], nv * (size_t)std::max(b.total, 1ll)) != hipSuccess ||
        rx.alloc(&rx_pr[g], (size_t)std::max(b.total, 1ll)) != hipSuccess ||
        rx.alloc(&rx_off[g], (size_t)n + 1) != hipSuccess ||
        hipMemcpyAsync(rx_off[g], b.offs.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice,
                       rs) != hipSuccess)
      return fail("rays_hip_trace_gather: out of device memory on the root");
  }
  int r = g_rccl.GroupStart();
  for (int g = 1; g < G && r == 0; g++) {
    const GatherBlock& b = blk[g];
    const size_t n = (size_t)(b.r1 - b.r0);
    if (n == 0) continue;
    // peer g -> root: summaries straight into the global arrays, trajectories packed
    r = g_rccl.Send(b.d.np, n, kNcclInt32, 0, g_rccl.comms[g], b.st());
    if (!r) r = g_rccl.Recv(A.np + b.r0, n, kNcclInt32, g, g_rccl.comms[0], rs);
    if (!r) r = g_rccl.Send(b.d.sc, n, kNcclInt32, 0, g_rccl.comms[g], b.st());
    if (!r) r = g_rccl.Recv(A.sc + b.r0, n, kNcclInt32, g, g_rccl.comms[0], rs);
    if (!r) r = g_rccl.Send(b.d.ev, n * nv, kNcclDouble, 0, g_rccl.comms[g], b.st());
    if (!r) r = g_rccl.Recv(A.ev + nv * (size_t)b.r0, n * nv, kNcclDouble, g, g_rccl.comms[0], rs);
    if (!r) r = g_rccl.Send(b.d.er, n, kNcclDouble, 0, g_rccl.comms[g], b.st());
    if (!r) r = g_rccl.Recv(A.er + b.r0, n, kNcclDouble, g, g_rccl.comms[0], rs);
    if (!r) r = g_rccl.Send(b.d.mr, n, kNcclDouble, 0, g_rccl.comms[g], b.st());
    if (!r) r = g_rccl.Recv(A.mr + b.r0, n, kNcclDouble, g, g_rccl.comms[0], rs);
    if (b.total > 0) {
      if (!r) r = g_rccl.Send(b.d_pv, (size_t)b.total * nv, kNcclDouble, 0, g_rccl.comms[g], b.st());
      if (!r) r = g_rccl.Recv(rx_pv[g], (size_t)b.total * nv, kNcclDouble, g, g_rccl.comms[0], rs);
      if (!r) r = g_rccl.Send(b.d_pr, (size_t)b.total, kNcclDouble, 0, g_rccl.comms[g], b.st());
      if (!r) r = g_rccl.Recv(rx_pr[g], (size_t)b.total, kNcclDouble, g, g_rccl.comms[0], rs);
    }
  }
  const int r2 = g_rccl.GroupEnd();
  if (r || r2) return rccl_fail(r ? r : r2, "grouped ncclSend/ncclRecv");
  // unpack every peer's block into its slab of the global arrays (zero-filled in phase 1)
  for (int g = 1; g < G; g++) {
    const GatherBlock& b = blk[g];
    const int n = b.r1 - b.r0;
    if (n <= 0 || b.total == 0) continue;
    if (rays::launch_pack(false, n, (int)nv, p->nstep_max, A.np + b.r0, rx_off[g], At.rv + npt * nv * (size_t)b.r0,
                          At.res + npt * (size_t)b.r0, rx_pv[g], rx_pr[g], rs) != hipSuccess)
      return fail("rays_hip_trace_gather: unpack kernel launch failed");
  }
  return 0;
}

}  // namespace

static void drop_gathered_result() { g_gathered.release(); }

extern "C" int rays_hip_trace_gather(const rays_params_t* p, int nray, const double* rvec0, const double* rindex_vec0,
                                     rays_device_result_t* out) {
  int rc = rays_hip_check_params(p);
  if (rc) return rc;
  if (!out) return fail("rays_hip_trace_gather: null result block");
  if (nray < 0) return fail("rays_hip_trace_gather: nray < 0");
  if (nray > 0 && (!rvec0 || !rindex_vec0)) return fail("rays_hip_trace_gather: null array argument");
  std::vector<int> devs;
  if (call_devices(&devs)) return 3;
  for (size_t i = 0; i < devs.size(); i++)
    for (size_t j = i + 1; j < devs.size(); j++)
      if (devs[i] == devs[j]) return fail("rays_hip_trace_gather: the device list must not repeat a device (RCCL: one rank per device)");
  const int G = (int)devs.size(), root = devs[0];
  const size_t npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  std::memset(out, 0, sizeof *out);
  out->device = root;
  out->nray = nray;
  if (nray == 0) return 0;
  if (G > 1) {
    rc = rccl_open(devs);
    if (rc) return rc;
  }
  // ---- the root's global arrays: the previous call's result is valid until now ---------------------------------
  HIP_TRY(hipSetDevice(root));
  g_gathered.release();
  claim_slot_for_device(kResultSlot, root);
  SummaryArrays A;
  TrajectoryArrays At;
  HIP_TRY_AS("hipMalloc (result arrays)", At.alloc(g_gathered, (size_t)nray, npt, nv));
  HIP_TRY_AS("hipMalloc (result arrays)", A.alloc(g_gathered, (size_t)nray, nv, false));
  // ---- phase 1: every device traces its block (one host thread per device) ------------------------------------
  // (rx gives its buffers back to the cache when this call returns -- after blk, declared behind it, has drained its
  // streams)
  DeviceBuffers rx(0);  // the root's receive buffers, from the root block's slot
  std::deque<GatherBlock> blk;
  rc = run_blocks(devs, nray, &blk,
                  [&](GatherBlock& b) { return gather_trace_block(b, A, At, p, nray, {rvec0, rindex_vec0}); });
  if (rc) return rc;
  // ---- phase 2: the gather ---------------------------------------------------------------------------------------
  int result = G > 1 ? gather_to_root(blk, A, At, p, root, rx) : 0;
  // ---- completion: every stream drained here, where a failure can still be reported (RayBlock's destructor drains
  // again, silently, on every way out of this call) ---------------------------------------------------------------
  for (const GatherBlock& b : blk) {
    if (!b.st()) continue;
    if (hipSetDevice(b.dev) == hipSuccess && hipStreamSynchronize(b.st()) != hipSuccess && !result)
      result = fail("rays_hip_trace_gather: stream synchronisation failed");
  }
  (void)hipSetDevice(root);
  if (result) return result;
  out->ray_vec = At.rv; out->residual = At.res; out->npoints = A.np; out->stop_code = A.sc;
  out->end_ray_vec = A.ev; out->end_residuals = A.er; out->max_residuals = A.mr;
  return 0;
}

// Copies a gathered result (or any device-resident result on `device`) into host arrays: the
// ray_results_m image.  Entries past npoints are copied too (zeros).
extern "C" int rays_hip_result_to_host(const rays_params_t* p, const rays_device_result_t* r, double* ray_vec,
                                       double* residual, int32_t* npoints, int32_t* stop_code, double* end_ray_vec,
                                       double* end_residuals, double* max_residuals) {
  if (!p || !r) return fail("rays_hip_result_to_host: null argument");
  const size_t n = (size_t)r->nray, npt = (size_t)p->nstep_max + 1, nv = (size_t)p->nv;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(r->device));
  if (ray_vec) HIP_TRY(hipMemcpy(ray_vec, r->ray_vec, sizeof(double) * npt * nv * n, hipMemcpyDeviceToHost));
  if (residual) HIP_TRY(hipMemcpy(residual, r->residual, sizeof(double) * npt * n, hipMemcpyDeviceToHost));
  if (npoints) HIP_TRY(hipMemcpy(npoints, r->npoints, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (stop_code) HIP_TRY(hipMemcpy(stop_code, r->stop_code, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (end_ray_vec) HIP_TRY(hipMemcpy(end_ray_vec, r->end_ray_vec, sizeof(double) * nv * n, hipMemcpyDeviceToHost));
  if (end_residuals) HIP_TRY(hipMemcpy(end_residuals, r->end_residuals, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (max_residuals) HIP_TRY(hipMemcpy(max_residuals, r->max_residuals, sizeof(double) * n, hipMemcpyDeviceToHost));
  return 0;
}
