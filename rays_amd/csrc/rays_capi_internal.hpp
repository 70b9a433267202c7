// rays_capi_internal.hpp -- what an entry point of the C ABI that lives outside rays_capi.hip (rays_diag.hip) needs of
// that file's local state: the error text of rays_hip_last_error and the device copies of the tables.  Internal:
// rays_hip.map exports rays_hip_* only.
#pragma once

#include "rays_device.hpp"

namespace rays {

// set the calling thread's rays_hip_last_error text; return the ABI's error codes (1 = configuration, 2 = HIP)
int capi_fail(const char* msg);
int capi_hip_fail(hipError_t e, const char* what);

// rays_hip_check_params(p), then the kernels' parameter block for p on the CURRENT device: make_dev_params plus the
// device pointers of the Z-function table (with damping) and of the axisym_toroid tables (uploaded when stale).
// *unit_exponents: every profile exponent in use is 1 (the kernels' kEqUnitExp flag).  0, or an error code with the
// message set.
int capi_dev_params(const rays_params_t* p, DevParams* D, bool* unit_exponents);

// A device block of at least `bytes` for a post-processor's scratch on the current device: one block per (device,
// stream), grown on demand, kept between calls and released by rays_hip_finalize (launches on a stream run one after
// another, so they may share it).  0, or an error code with the message set.
int capi_stream_workspace(hipStream_t stream, size_t bytes, void** out);

}  // namespace rays
