// capi_device.h -- shared pieces of the device-pointer entry points (include/fsgm.h, "Device-pointer entry points"):
// pointer checks, the capture refusal, the event join with the caller's stream and the status word.
#pragma once
#include "capi_common.h"

namespace fsgm {

// FSGM_ERR_UNSUPPORTED when `s` is being captured into a graph (nothing may be queued then), FSGM_ERR_HIP when the
// runtime cannot tell
fsgm_status device_check_stream(hipStream_t s, const char* who);
// `p` (may be NULL when !required) must be device memory of `device`, aligned to `align`, with `bytes` bytes inside its
// allocation; a failed runtime query is cleared so that it does not surface in a later hipGetLastError
fsgm_status device_check_ptr(const void* p, size_t bytes, size_t align, int device, bool required, const char* who, const char* what);

// The two events of a plan's device calls: `in` recorded on the caller's stream and waited for by the plan's stream,
// `out` recorded on the plan's stream and waited for by the caller's.  Created on a plan's first device call.
struct DeviceJoin {
    hipEvent_t in = nullptr, out = nullptr;
    fsgm_status ensure();
    void destroy();
    fsgm_status enter(hipStream_t caller, hipStream_t plan);
    fsgm_status leave(hipStream_t plan, hipStream_t caller);
};

// One wave on `st`: *status = (flag && *flag) ? FSGM_ERR_HIP : 0, *flag cleared (either pointer may be NULL)
void launch_device_status(hipStream_t st, uint32_t* flag, int32_t* status);

// Swaps a plan's buffer pointer for the caller's for the length of one enqueue and puts it back on every exit.
template <class T>
struct Bind {
    T*& slot;
    T* saved;
    Bind(T*& s, T* v) : slot(s), saved(s) { if (v) slot = v; }
    ~Bind() { slot = saved; }
    Bind(const Bind&) = delete;
    Bind& operator=(const Bind&) = delete;
};

}  // namespace fsgm
