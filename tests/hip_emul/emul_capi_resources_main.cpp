// TEST INFRASTRUCTURE ONLY: the owners of the C ABI's device resources (rays_amd/csrc/rays_capi_resources.hpp) alone,
// as a stand-alone host program on the emulated HIP runtime with four devices, for sanitizer runs
// (tests/test_cpu_capi_resources.py builds it with -fsanitize=address,undefined; leak detection on).  Exits 0 only if
// every check held and nothing of the emulated runtime is left alive.
#define RAYS_EMUL_RUNTIME 1
#include <hip/hip_runtime.h>
RAYS_EMUL_DEFINE_GLOBALS
#include "../../rays_amd/csrc/rays_capi_resources.hpp"

using namespace rays::host;

#include "emul_capi_check.hpp"

static long long live_device() {
  hip_emul::State& s = hip_emul::state();
  std::lock_guard<std::mutex> lk(s.mu);
  return (long long)s.allocs.size();
}
static bool on_device(const void* p, size_t bytes, int dev) { return hip_emul::owner(p, bytes) == dev; }

// a workspace that grows, shrinks its request and grows again, on two streams of two devices
static void workspace() {
  StreamWorkspace ws;
  hipStream_t st[2][2];
  for (int d = 0; d < 2; d++) {
    CHECK(hipSetDevice(d + 1) == hipSuccess);
    for (int k = 0; k < 2; k++) CHECK(hipStreamCreate(&st[d][k]) == hipSuccess);
  }
  const long long before = live_device();
  for (int d = 0; d < 2; d++)
    for (int k = 0; k < 2; k++) {
      CHECK(hipSetDevice(d + 1) == hipSuccess);
      void *a = nullptr, *b = nullptr, *c = nullptr;
      CHECK(ws.get(st[d][k], 1000, &a) == hipSuccess && on_device(a, 1000, d + 1));
      std::memset(a, 1, 1000);
      CHECK(ws.get(st[d][k], 10, &b) == hipSuccess && b == a);   // a smaller request: the same block
      CHECK(ws.get(st[d][k], 1000, &b) == hipSuccess && b == a);
      CHECK(ws.get(st[d][k], 5000, &c) == hipSuccess && on_device(c, 5000, d + 1));   // (the old block is freed)
      std::memset(c, 2, 5000);
      CHECK(live_device() == before + 2 * d + k + 1);            // one block per (device, stream)
    }
  // the stream of another device than the current one: the regrow's synchronisation refuses it, the block stays
  void* x = nullptr;
  CHECK(hipSetDevice(1) == hipSuccess);
  CHECK(ws.get(st[1][0], 100, &x) == hipSuccess);                // (device 1, a stream of device 2): a first block
  CHECK(ws.get(st[1][0], 200, &x) == hipErrorInvalidHandle);
  (void)hipGetLastError();
  hip_emul::state().wrong_device = 0;
  ws.release_all();
  CHECK(live_device() == before);
  ws.release_all();                                               // idempotent; leaves another device current
  CHECK(hipSetDevice(1) == hipSuccess);
  CHECK(ws.get(st[0][0], 64, &x) == hipSuccess && on_device(x, 64, 1));   // usable again
  ws.release_all();
  for (int d = 0; d < 2; d++)
    for (int k = 0; k < 2; k++) CHECK(hipStreamDestroy(st[d][k]) == hipSuccess);
}

// a table uploaded on two devices, re-versioned, released and fetched again
static void table() {
  DeviceTable t;
  t.host.assign(100, 1.5);
  t.version++;
  const double* p[2] = {nullptr, nullptr};
  for (int d = 0; d < 2; d++) {
    CHECK(hipSetDevice(2 * d) == hipSuccess);                     // devices 0 and 2
    CHECK(t.device_ptr(&p[d]) == hipSuccess && on_device(p[d], 800, 2 * d) && p[d][99] == 1.5);
    const double* again = nullptr;
    CHECK(t.device_ptr(&again) == hipSuccess && again == p[d]);   // no second upload
  }
  CHECK(live_device() == 2);
  t.host.assign(300, 2.5);                                        // a new table: larger, new version
  t.version++;
  const double* q = nullptr;
  CHECK(t.device_ptr(&q) == hipSuccess && on_device(q, 2400, 2) && q[299] == 2.5);   // device 2: uploaded anew
  CHECK(live_device() == 2);
  t.release_all();
  CHECK(live_device() == 0);
  CHECK(hipSetDevice(0) == hipSuccess);
  CHECK(t.device_ptr(&q) == hipSuccess && on_device(q, 2400, 0) && q[0] == 2.5);     // from the host copy again
  t.release_all();
  t.release_all();
  CHECK(live_device() == 0);
}

// a call that returns early with some blocks allocated and one handed out
static hipError_t early_exit(int slot, double** kept) {
  DeviceBuffers bufs(slot);
  double *a = nullptr, *b = nullptr;
  int* c = nullptr;
  hipError_t e = bufs.alloc(&a, 100);
  if (e == hipSuccess) e = bufs.alloc(&b, 200);
  if (e == hipSuccess) e = bufs.alloc(&c, 50);
  if (e != hipSuccess) return e;
  std::memset(a, 0, 800); std::memset(b, 0, 1600); std::memset(c, 0, 200);
  *kept = bufs.detach(b);
  return hipErrorInvalidValue;   // "a later step failed": a and c go back, b is the caller's
}
static void buffers() {
  CHECK(hipSetDevice(3) == hipSuccess);
  double* kept = nullptr;
  CHECK(early_exit(kNoSlot, &kept) == hipErrorInvalidValue);
  CHECK(live_device() == 1 && on_device(kept, 1600, 3));          // plain blocks: freed at once
  cached_free(kNoSlot, kept);
  CHECK(live_device() == 0);
  claim_slot_for_device(5, 3);
  CHECK(early_exit(5, &kept) == hipErrorInvalidValue);
  CHECK(live_device() == 3);                                      // cached blocks: two idle in slot 5, one out
  {
    DeviceBuffers again(5);
    int* c = nullptr;
    CHECK(again.alloc(&c, 40) == hipSuccess && live_device() == 3);   // served from the idle list (160 <= 200 bytes)
    again.release();
    again.release();
  }
  cached_free(5, kept);
  CHECK(live_device() == 3);
}

// a slot claimed for another device while a block from it is out; the block then given back
static void moved_slot() {
  CHECK(hipSetDevice(0) == hipSuccess);
  claim_slot_for_device(2, 0);
  SlotStream s0;
  CHECK(s0.open(2) == hipSuccess && s0.get()->device == 0);
  void *out = nullptr, *idle = nullptr;
  CHECK(cached_malloc(2, &out, 4096) == hipSuccess && cached_malloc(2, &idle, 4096) == hipSuccess);
  cached_free(2, idle);
  const long long before = live_device();
  CHECK(hipSetDevice(1) == hipSuccess);
  claim_slot_for_device(2, 1);                                    // device 0's idle block and stream go
  CHECK(live_device() == before - 1);
  SlotStream s1;
  CHECK(s1.open(2) == hipSuccess && s1.get()->device == 1);
  cached_free(2, out);                                            // a device-0 block: freed, not cached
  CHECK(live_device() == before - 2);
  void* p = nullptr;
  CHECK(cached_malloc(2, &p, 4096) == hipSuccess && on_device(p, 4096, 1));
  cached_free(2, p);
  void* q = nullptr;
  CHECK(cached_malloc(2, &q, 4000) == hipSuccess && q == p);      // a device-1 block: cached and handed out again
  cached_free(2, q);
  SlotStream own;                                                 // no slot: a stream of the call's own
  CHECK(own.open(kNoSlot) == hipSuccess && own.get() && own.get()->device == 1);
  EventPair ev;
  CHECK(ev.create() == hipSuccess && ev[0] && ev[1] && ev[0] != ev[1]);
}

int main() {
  if (hip_emul::device_count() < 4) { std::fprintf(stderr, "needs 4 emulated devices\n"); return 2; }
  CHECK(hipSetDevice(2) == hipSuccess);
  {
    CurrentDevice restore;
    workspace();
    table();
    buffers();
    moved_slot();
  }
  int dev = -1;
  CHECK(hipGetDevice(&dev) == hipSuccess && dev == 2);
  release_cached_device_blocks();
  release_cached_device_blocks();
  hip_emul::State& s = hip_emul::state();
  CHECK(live_device() == 0 && s.live_pinned == 0 && s.live_streams == 0 && s.live_events == 0);
  CHECK(s.wrong_device == 0);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("capi resources ok\n");
  return 0;
}
