// capi_device.h -- shared pieces of the device-pointer entry points (include/fsgm.h, "Device-pointer entry points"):
// pointer checks, the capture refusal, the event join with the caller's stream and the status word.
#pragma once
#include "capi_common.h"
#include <initializer_list>

namespace fsgm {

// One row of an entry point's check table: `p` (may be NULL when !required) must be device memory of the call's device,
// aligned to `align`, with `bytes` bytes inside its allocation.  A pointer that the call reads only under a condition is
// passed as `cond ? ptr : nullptr`, one that is required only under a condition with `required = cond`.
struct DevicePtr {
    const void* p;
    size_t bytes, align;
    bool required;
    const char* what;
};
// The checks of every device entry point behind its own argument checks, in this order: `device` made current
// (use_device), the caller's stream `cs` refused while it is captured into a graph (FSGM_ERR_UNSUPPORTED: nothing may be
// queued then), each pointer checked in list order (FSGM_ERR_INVALID).  Entry points call it before they look up or build
// a plan: a call refused here has allocated nothing.  captured (non-null): a captured stream is let through and *captured says
// whether it is one -- for an entry point whose warm call only queues work (no allocation, no host wait) and joins the plan's
// stream to the caller's by events, which a capture records as a fork and a join.  Such an entry point refuses a captured call
// that its cached plan cannot serve as it stands, and pins the plan it records (PlanCache).
fsgm_status device_check_args(const char* who, int device, hipStream_t cs, std::initializer_list<DevicePtr> ptrs,
                              bool* captured = nullptr);

// The two events of a plan's device calls: `in` recorded on the caller's stream and waited for by the plan's stream,
// `out` recorded on the plan's stream and waited for by the caller's.  Created on a plan's first device call.
struct DeviceJoin {
    hipEvent_t in = nullptr, out = nullptr;
    fsgm_status ensure();
    void destroy();
    fsgm_status enter(hipStream_t caller, hipStream_t plan);
    fsgm_status leave(hipStream_t plan, hipStream_t caller);
};

// One device call on a plan: the plan's stream waits for the caller's, work() queues everything on the plan's stream (the
// status word last, and only when it succeeds), the caller's stream waits for the plan's -- on every exit once the join is
// entered, so whatever was queued stays ordered before the caller's later work.  Returns work's status, else a failed
// launch as FSGM_ERR_HIP, else the join's.
template <class Work>
fsgm_status device_call(DeviceJoin& j, hipStream_t caller, hipStream_t plan, Work&& work) {
    fsgm_status st;
    if ((st = j.ensure()) != FSGM_OK || (st = j.enter(caller, plan)) != FSGM_OK) return st;
    st = work();
    const hipError_t le = hipGetLastError();                     // (collected on every path: no later call inherits it)
    const fsgm_status js = j.leave(plan, caller);
    if (st != FSGM_OK) return st;
    if (le != hipSuccess) return fail(FSGM_ERR_HIP, "a launch of the device call failed: %s", hipGetErrorString(le));
    return js;
}

// One wave on `st`: *status = *hip_flag ? FSGM_ERR_HIP : *invalid_flag ? FSGM_ERR_INVALID : 0, both flags cleared (each
// pointer may be NULL; nothing is launched when all three are)
void launch_device_status(hipStream_t st, uint32_t* hip_flag, uint32_t* invalid_flag, int32_t* status);

// A plan's ingest flag -- the word an ingest kernel raises for a value outside the declared bound, launch_device_status's
// invalid_flag -- created cleared on `st` at its first use
inline fsgm_status ensure_ingest_flag(uint32_t** flag, hipStream_t st) {
    if (*flag) return FSGM_OK;
    FSGM_HIP(hipMalloc((void**)flag, sizeof(uint32_t)));
    FSGM_HIP(hipMemsetAsync(*flag, 0, sizeof(uint32_t), st));
    return FSGM_OK;
}

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
