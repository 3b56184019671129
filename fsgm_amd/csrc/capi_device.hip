// capi_device.hip -- shared pieces of the device-pointer entry points (capi_device.h): pointer checks, capture refusal,
// the event join with the caller's stream and the status kernel.
#include "capi_device.h"
#include <algorithm>

namespace fsgm {

static fsgm_status device_check_stream(hipStream_t s, const char* who, bool* captured) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(s, &cs);
    if (e == hipErrorStreamCaptureImplicit || (e == hipSuccess && cs != hipStreamCaptureStatusNone)) {
        (void)hipGetLastError();
        // (the legacy stream while another stream of the thread is captured cannot join a capture: refused for every entry)
        if (captured && e == hipSuccess && cs == hipStreamCaptureStatusActive) { *captured = true; return FSGM_OK; }
        return fail(FSGM_ERR_UNSUPPORTED, "%s: the stream is being captured into a graph (graph capture is not supported)", who);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FSGM_ERR_HIP, "%s: hipStreamIsCapturing failed: %s", who, hipGetErrorString(e));
    }
    return FSGM_OK;
}

// a failed runtime query is cleared so that it does not surface in a later hipGetLastError
static fsgm_status device_check_ptr(const void* p, size_t bytes, size_t align, int device, bool required, const char* who, const char* what) {
    if (!p) {
        if (required) return fail(FSGM_ERR_INVALID, "%s: %s is NULL", who, what);
        return FSGM_OK;
    }
    if ((uintptr_t)p % align != 0)
        return fail(FSGM_ERR_INVALID, "%s: %s (%p) is not aligned to %zu bytes", who, what, p, align);
    hipPointerAttribute_t a{};
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FSGM_ERR_INVALID, "%s: %s (%p) is not memory known to the HIP runtime (%s)", who, what, p, hipGetErrorString(e));
    }
    if (a.type != hipMemoryTypeDevice)
        return fail(FSGM_ERR_INVALID, "%s: %s (%p) is not device memory (memory type %d): pass HBM of device %d", who, what, p, (int)a.type, device);
    if (a.device != device)
        return fail(FSGM_ERR_INVALID, "%s: %s (%p) lives on device %d, the call runs on device %d", who, what, p, a.device, device);
    void* base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, const_cast<void*>(p));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FSGM_ERR_INVALID, "%s: %s (%p): no allocation found (%s)", who, what, p, hipGetErrorString(e));
    }
    const size_t used = (size_t)((const char*)p - (const char*)base);
    if (used > size || size - used < bytes)
        return fail(FSGM_ERR_INVALID, "%s: %s (%p) needs %zu bytes, its allocation holds %zu from there", who, what, p, bytes, size - std::min(used, size));
    return FSGM_OK;
}

fsgm_status device_check_args(const char* who, int device, hipStream_t cs, std::initializer_list<DevicePtr> ptrs, bool* captured) {
    if (captured) *captured = false;
    fsgm_status st = use_device(device);
    if (st != FSGM_OK || (st = device_check_stream(cs, who, captured)) != FSGM_OK) return st;
    for (const DevicePtr& d : ptrs)
        if ((st = device_check_ptr(d.p, d.bytes, d.align, device, d.required, who, d.what)) != FSGM_OK) return st;
    return FSGM_OK;
}

fsgm_status DeviceJoin::ensure() {
    if (!in) FSGM_HIP(hipEventCreateWithFlags(&in, hipEventDisableTiming));
    if (!out) FSGM_HIP(hipEventCreateWithFlags(&out, hipEventDisableTiming));
    return FSGM_OK;
}

void DeviceJoin::destroy() {
    if (in) (void)hipEventDestroy(in);
    if (out) (void)hipEventDestroy(out);
    in = out = nullptr;
}

fsgm_status DeviceJoin::enter(hipStream_t caller, hipStream_t plan) {
    FSGM_HIP(hipEventRecord(in, caller));
    FSGM_HIP(hipStreamWaitEvent(plan, in, 0));
    return FSGM_OK;
}

fsgm_status DeviceJoin::leave(hipStream_t plan, hipStream_t caller) {
    FSGM_HIP(hipEventRecord(out, plan));
    FSGM_HIP(hipStreamWaitEvent(caller, out, 0));
    return FSGM_OK;
}

__global__ __launch_bounds__(64) void device_status_kernel(uint32_t* __restrict__ hip_flag, uint32_t* __restrict__ invalid_flag,
                                                           int32_t* __restrict__ status) {
    if (threadIdx.x != 0) return;
    uint32_t h = 0, v = 0;
    if (hip_flag) { h = *hip_flag; *hip_flag = 0; }
    if (invalid_flag) { v = *invalid_flag; *invalid_flag = 0; }
    if (status) *status = h != 0 ? (int32_t)FSGM_ERR_HIP : v != 0 ? (int32_t)FSGM_ERR_INVALID : 0;
}

void launch_device_status(hipStream_t st, uint32_t* hip_flag, uint32_t* invalid_flag, int32_t* status) {
    if (!hip_flag && !invalid_flag && !status) return;
    hipLaunchKernelGGL(device_status_kernel, dim3(1), dim3(64), 0, st, hip_flag, invalid_flag, status);
}

}  // namespace fsgm
