// rays_capi_resources.hpp -- the owners of the device resources behind the C ABI (rays_capi.hip, rays_gather.inc).
//
// Host code on the HIP runtime API and the standard library only: no kernel, no rays_params_t, no error text.  Every
// function reports a hipError_t; the entry points turn it into their message.  Each resource has ONE owner here, and
// every owner has a release that rays_hip_finalize calls:
//   StreamWorkspace   one growable device block per (device, stream)
//   DeviceTable       a host table with a lazily uploaded copy per device
//   the block cache   device blocks and the stream of a slot of the device list, kept between calls
//   DeviceBuffers     the device blocks of ONE call, given back when the call ends, however it ends
//   SlotStream, EventPair, CurrentDevice   the same for a call's stream, its two copy events, the caller's device
//   RayBlock          one block of a sharded call: its slot's stream and buffers, drained before the buffers go back
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace rays {
namespace host {

constexpr int kMaxDevices = 16;           // device ordinals and slots of the device list: 0 .. kMaxDevices - 1
constexpr int kResultSlot = kMaxDevices;  // cache slot of the gathered result (rays_hip_trace_gather)
constexpr int kNoSlot = -1;               // no cache: plain hipMalloc / hipFree

// Puts the calling thread's current device back when the scope ends.
class CurrentDevice {
 public:
  CurrentDevice() { have_ = hipGetDevice(&dev_) == hipSuccess; }
  ~CurrentDevice() { if (have_) (void)hipSetDevice(dev_); }
  CurrentDevice(const CurrentDevice&) = delete;
  CurrentDevice& operator=(const CurrentDevice&) = delete;

 private:
  int dev_ = 0;
  bool have_ = false;
};

// One device block per (device, stream), grown on demand and kept: launches on a stream run one after another, so they
// may share it.  A request the block already holds reuses it; a larger one waits for the stream (an earlier launch may
// still use the old block), frees it and allocates the new size.
class StreamWorkspace {
 public:
  hipError_t get(hipStream_t stream, size_t bytes, void** out) {  // on the current device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu_);
    Block& w = blocks_[std::make_pair(dev, stream)];
    if (w.bytes < bytes) {
      if (w.ptr) {
        e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        (void)hipFree(w.ptr);
      }
      w.ptr = nullptr;
      w.bytes = 0;
      e = hipMalloc(&w.ptr, bytes);
      if (e != hipSuccess) return e;
      w.bytes = bytes;
    }
    *out = w.ptr;
    return hipSuccess;
  }
  void release_all() {  // changes the current device
    std::lock_guard<std::mutex> lk(mu_);
    for (auto& kv : blocks_)
      if (kv.second.ptr) {
        (void)hipSetDevice(kv.first.first);
        (void)hipDeviceSynchronize();
        (void)hipFree(kv.second.ptr);
      }
    blocks_.clear();
  }

 private:
  struct Block {
    void* ptr = nullptr;
    size_t bytes = 0;
  };
  std::mutex mu_;
  std::map<std::pair<int, hipStream_t>, Block> blocks_;
};

// A host table and its copies on the devices, uploaded on first use there and again after the host copy changed
// (`version`: bump it with every change of `host`).  No lock of its own: the table's shape lives with its user, who
// serialises access to both.
struct DeviceTable {
  std::vector<double> host;
  unsigned long long version = 0;

  hipError_t device_ptr(const double** out) {  // on the current device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((int)copies_.size() <= dev) copies_.resize(dev + 1);
    Copy& c = copies_[dev];
    if (c.version != version) {
      if (c.ptr) (void)hipFree(c.ptr);
      c.ptr = nullptr;
      c.version = 0;
      e = hipMalloc(&c.ptr, sizeof(double) * host.size());
      if (e == hipSuccess) e = hipMemcpy(c.ptr, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice);
      if (e != hipSuccess) return e;
      c.version = version;
    }
    *out = c.ptr;
    return hipSuccess;
  }
  void release_all() {  // the host copy stays: the next device_ptr uploads again
    for (Copy& c : copies_) {
      if (c.ptr) (void)hipFree(c.ptr);
      c = Copy();
    }
  }

 private:
  struct Copy {
    double* ptr = nullptr;
    unsigned long long version = 0;  // 0: stale (a table that was set has version >= 1)
  };
  std::vector<Copy> copies_;
};

// Device buffers of rays_hip_trace are kept between calls (a host that traces repeatedly -- ray_scan, a
// time loop -- otherwise pays ~6 ms per call for hipMalloc/hipFree of the 64k fan's 5 GB): a released
// block goes to its slot's free list and serves the next request of a similar size.  Everything is
// returned to the driver by release_cached_device_blocks, or at once when an allocation fails.
// (One cache per SLOT of the device list rays_hip_init[_devices] selected -- a device may appear in
// several slots, each with its own host thread, stream and buffers -- plus kResultSlot.)
struct DeviceBlockCache {
  struct Block { void* p; size_t cap; };
  struct Live { size_t cap; int device; };  // device: the one the slot served when the block was handed out
  int device = -1;
  std::mutex mu;
  std::vector<Block> idle;
  std::map<void*, Live> live;
  hipStream_t stream = nullptr;  // the entry's stream on this device (creating one costs ~8 ms per call)
  void drop_idle() {  // caller holds mu and has the device current
    for (auto& b : idle) (void)hipFree(b.p);
    idle.clear();
  }
};
inline DeviceBlockCache g_blocks[kMaxDevices + 1];
inline bool cache_slot(int slot) { return slot >= 0 && slot <= kMaxDevices; }

inline hipError_t cached_malloc(int slot, void** out, size_t bytes) {
  if (!cache_slot(slot)) return hipMalloc(out, bytes);
  DeviceBlockCache& c = g_blocks[slot];
  std::lock_guard<std::mutex> lk(c.mu);
  size_t best = c.idle.size();
  for (size_t i = 0; i < c.idle.size(); i++)
    if (c.idle[i].cap >= bytes && c.idle[i].cap <= bytes + bytes / 4 + (1u << 20) &&
        (best == c.idle.size() || c.idle[i].cap < c.idle[best].cap))
      best = i;
  if (best < c.idle.size()) {
    *out = c.idle[best].p;
    c.live[*out] = {c.idle[best].cap, c.device};
    c.idle.erase(c.idle.begin() + (long)best);
    return hipSuccess;
  }
  hipError_t e = hipMalloc(out, bytes ? bytes : 1);
  if (e != hipSuccess) {  // give the idle blocks back and try once more
    (void)hipGetLastError();
    c.drop_idle();
    e = hipMalloc(out, bytes ? bytes : 1);
  }
  if (e == hipSuccess) c.live[*out] = {bytes ? bytes : 1, c.device};
  return e;
}
inline hipError_t cached_stream(int slot, hipStream_t* out, bool* owned) {
  *owned = !cache_slot(slot);
  if (*owned) return hipStreamCreate(out);
  DeviceBlockCache& c = g_blocks[slot];
  std::lock_guard<std::mutex> lk(c.mu);
  if (!c.stream) {
    hipError_t e = hipStreamCreate(&c.stream);
    if (e != hipSuccess) return e;
  }
  *out = c.stream;
  return hipSuccess;
}
// A block whose slot has moved on to another device since it was handed out (a kept result outlives the call that
// allocated it) goes back to the driver: in the idle list it would be handed to a kernel on the wrong device.
inline void cached_free(int slot, void* ptr) {
  if (!ptr) return;
  if (!cache_slot(slot)) { (void)hipFree(ptr); return; }
  DeviceBlockCache& c = g_blocks[slot];
  std::lock_guard<std::mutex> lk(c.mu);
  auto it = c.live.find(ptr);
  if (it == c.live.end()) { (void)hipFree(ptr); return; }
  if (it->second.device == c.device) c.idle.push_back({ptr, it->second.cap});
  else (void)hipFree(ptr);
  c.live.erase(it);
}

// A cache slot serves one device at a time (its stream and idle blocks live there).  Every user of a slot -- the
// blocks of rays_hip_trace and of rays_hip_trace_gather alike -- claims it for the device it is about to use: a slot
// that last served another device (e.g. four slots on device 0 for a large fan, then one slot per device for a
// gather) first gives that device's blocks and stream back.  Caller has `dev` current; it is current on return.
inline void claim_slot_for_device(int slot, int dev) {
  if (!cache_slot(slot)) return;
  DeviceBlockCache& c = g_blocks[slot];
  std::lock_guard<std::mutex> lk(c.mu);
  if (c.device >= 0 && c.device != dev) {
    (void)hipSetDevice(c.device);
    c.drop_idle();
    if (c.stream) (void)hipStreamDestroy(c.stream);
    c.stream = nullptr;
    (void)hipSetDevice(dev);
  }
  c.device = dev;
}

inline void release_cached_device_blocks() {  // changes the current device
  for (DeviceBlockCache& c : g_blocks) {
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.device >= 0) (void)hipSetDevice(c.device);
    c.drop_idle();
    if (c.stream) (void)hipStreamDestroy(c.stream);
    c.stream = nullptr;
    c.device = -1;  // (a block still out is freed, not cached, when it comes back)
  }
}

// The device blocks of one call: from a cache slot, or plain hipMalloc with kNoSlot.  Whatever it still owns when it
// goes out of scope returns to the slot's cache (or is freed); detach() hands a block to a longer-lived owner, who
// gives it back with cached_free(slot, ptr).
class DeviceBuffers {
 public:
  explicit DeviceBuffers(int slot = kNoSlot) : slot_(slot) {}
  ~DeviceBuffers() { release(); }
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;

  template <class T>
  hipError_t alloc(T** out, size_t count) {
    void* p = nullptr;
    const hipError_t e = cached_malloc(slot_, &p, sizeof(T) * count);
    if (e != hipSuccess) return e;
    ptrs_.push_back(p);
    *out = static_cast<T*>(p);
    return hipSuccess;
  }
  template <class T>
  T* detach(T* p) {
    ptrs_.erase(std::remove(ptrs_.begin(), ptrs_.end(), static_cast<void*>(p)), ptrs_.end());
    return p;
  }
  void release() {
    for (void* p : ptrs_) cached_free(slot_, p);
    ptrs_.clear();
  }

 private:
  int slot_;
  std::vector<void*> ptrs_;
};

// The stream of a cache slot (kept by the cache), or a stream of the call's own without one (destroyed with it).
class SlotStream {
 public:
  SlotStream() = default;
  ~SlotStream() { if (owned_ && st_) (void)hipStreamDestroy(st_); }
  SlotStream(const SlotStream&) = delete;
  SlotStream& operator=(const SlotStream&) = delete;
  hipError_t open(int slot) { return cached_stream(slot, &st_, &owned_); }
  hipStream_t get() const { return st_; }

 private:
  hipStream_t st_ = nullptr;
  bool owned_ = false;
};

// The two events of a double-buffered copy.
class EventPair {
 public:
  EventPair() = default;
  ~EventPair() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  hipError_t create() {
    const hipError_t e = hipEventCreate(&ev_[0]);
    return e != hipSuccess ? e : hipEventCreate(&ev_[1]);
  }
  hipEvent_t operator[](int i) const { return ev_[i]; }

 private:
  hipEvent_t ev_[2] = {nullptr, nullptr};
};

// The per-ray arrays of a trace, on a device or on the host: the inputs, the summaries every trace kernel writes
// (sv, the state each ray started from, is optional) and the trajectories the recording kernels write as well.
struct RayInputs {
  const double *rvec0 = nullptr, *rindex_vec0 = nullptr, *power = nullptr;  // power: fused deposition only
};
struct SummaryArrays {
  int32_t *np = nullptr, *sc = nullptr;
  double *sv = nullptr, *ev = nullptr, *er = nullptr, *mr = nullptr;
  hipError_t alloc(DeviceBuffers& bufs, size_t n, size_t nv, bool with_sv) {
    hipError_t e = bufs.alloc(&np, n);
    if (e == hipSuccess) e = bufs.alloc(&sc, n);
    if (e == hipSuccess && with_sv) e = bufs.alloc(&sv, nv * n);
    if (e == hipSuccess) e = bufs.alloc(&ev, nv * n);
    if (e == hipSuccess) e = bufs.alloc(&er, n);
    return e == hipSuccess ? bufs.alloc(&mr, n) : e;
  }
};
struct TrajectoryArrays {
  double *rv = nullptr, *res = nullptr;
  hipError_t alloc(DeviceBuffers& bufs, size_t n, size_t npt, size_t nv) {
    const hipError_t e = bufs.alloc(&rv, npt * nv * n);
    return e == hipSuccess ? bufs.alloc(&res, npt * n) : e;
  }
};

// One block of a call that shards its rays over the slots of the device list: rays [r0, r1) on `dev`, with the slot's
// stream and cached buffers.  The worker thread of the block opens it and leaves rc / err behind.  THE rule of these
// calls lives in the destructor: however the call ends -- this block's worker failed half-way, another block's did, a
// later phase of the call failed -- nothing of the block is still in flight when its buffers go back to the slot's
// cache (bufs is destroyed after the destructor's body), and the caller's current device is as it was.
struct RayBlock {
  const int slot;
  int dev = 0, r0 = 0, r1 = 0;
  SlotStream stream;
  DeviceBuffers bufs;
  RayInputs in;      // the device copies of the block's inputs
  SummaryArrays d;   // the block's summaries on the device
  int rc = 0;
  std::string err;   // the worker thread's message when rc != 0

  explicit RayBlock(int s) : slot(s), bufs(s) {}
  ~RayBlock() {
    if (!st()) return;
    CurrentDevice restore;
    if (hipSetDevice(dev) == hipSuccess) (void)hipStreamSynchronize(st());
  }
  int n() const { return r1 - r0; }
  hipStream_t st() const { return stream.get(); }
  // the block's device, its claim on the slot, the slot's stream: what a worker does first
  hipError_t open() {
    const hipError_t e = hipSetDevice(dev);
    if (e != hipSuccess) return e;
    claim_slot_for_device(slot, dev);
    return stream.open(slot);
  }
  // device copies of rvec0 / rindex_vec0 (/ power) of rays [r0, r1), queued on the block's stream
  hipError_t upload(const RayInputs& host) {
    const size_t N = (size_t)n();
    const auto up = [&](const double* src, size_t per_ray, const double** out) {
      double* p = nullptr;
      hipError_t e = bufs.alloc(&p, per_ray * N);
      if (e == hipSuccess)
        e = hipMemcpyAsync(p, src + per_ray * (size_t)r0, sizeof(double) * per_ray * N, hipMemcpyHostToDevice, st());
      *out = p;
      return e;
    };
    hipError_t e = up(host.rvec0, 3, &in.rvec0);
    if (e == hipSuccess) e = up(host.rindex_vec0, 3, &in.rindex_vec0);
    if (e == hipSuccess && host.power) e = up(host.power, 1, &in.power);
    return e;
  }
  // the summaries' device-to-host copies into the caller's arrays at r0, queued on the block's stream; an array the
  // caller did not ask for (null) is skipped
  hipError_t download(const SummaryArrays& host, size_t nv) const {
    const size_t N = (size_t)n();
    const auto down = [&](auto* dst, const auto* src, size_t per_ray) {
      if (!dst) return hipSuccess;
      return hipMemcpyAsync(dst + per_ray * (size_t)r0, src, sizeof(*dst) * per_ray * N, hipMemcpyDeviceToHost, st());
    };
    hipError_t e = down(host.np, d.np, 1);
    if (e == hipSuccess) e = down(host.sc, d.sc, 1);
    if (e == hipSuccess) e = down(host.sv, d.sv, nv);
    if (e == hipSuccess) e = down(host.ev, d.ev, nv);
    if (e == hipSuccess) e = down(host.er, d.er, 1);
    return e == hipSuccess ? down(host.mr, d.mr, 1) : e;
  }
};

}  // namespace host
}  // namespace rays
