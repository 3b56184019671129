// capi_runtime.hip -- the part of the C ABI that belongs to no plan: the thread's last error text, the device queries, the
// copy-bandwidth probe and fsgm_shutdown.  See include/fsgm.h.
#include "capi_common.h"
#include "epi_kernels.h"

namespace fsgm {
char* last_error_buf() {
    static thread_local char buf[512] = "";
    return buf;
}
}  // namespace fsgm

using namespace fsgm;

extern "C" {

const char* fsgm_last_error(void) { return last_error_buf(); }

int fsgm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

fsgm_status fsgm_device_arch(int device, char* buf, size_t buflen) {
    FSGM_REQUIRE(buf && buflen > 0, "fsgm_device_arch: null buffer");
    hipDeviceProp_t prop;
    FSGM_HIP(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buflen, "%s", prop.gcnArchName);
    return FSGM_OK;
}

// The achievable HBM rate of this device, measured the way the aggregation kernels move bytes: a grid-stride
// copy kernel, 16 B per lane per access (launch_copy16, epi_kernels.hip), device memory to device memory, read + written
// bytes counted.  mode 0: that kernel; mode 1: hipMemcpyAsync D2D (the runtime's blit kernel), for comparison.
fsgm_status fsgm_measure_copy_bandwidth2(int32_t device, size_t bytes, int32_t iters, int32_t mode, double* gbps) {
    FSGM_REQUIRE(gbps && bytes >= 4096 && iters > 0, "fsgm_measure_copy_bandwidth: bad argument");
    FSGM_REQUIRE(mode == 0 || mode == 1, "fsgm_measure_copy_bandwidth: mode must be 0 (copy kernel) or 1 (hipMemcpyAsync)");
    FSGM_HIP(hipSetDevice(device));
    bytes &= ~(size_t)4095;
    void *a = nullptr, *b = nullptr;
    hipEvent_t e0, e1;
    FSGM_HIP(hipMalloc(&a, bytes));
    if (hipMalloc(&b, bytes) != hipSuccess) { (void)hipFree(a); return fail(FSGM_ERR_NOMEM, "copy probe: out of memory"); }
    (void)hipMemset(a, 1, bytes);
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    auto once = [&]() {
        if (mode == 0) launch_copy16(0, b, a, bytes);
        else (void)hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, 0);
    };
    once();
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < iters; i++) once();
    (void)hipEventRecord(e1, 0);
    hipError_t e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(a); (void)hipFree(b);
    if (e != hipSuccess) return fail(FSGM_ERR_HIP, "copy probe: %s", hipGetErrorString(e));
    *gbps = 2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9;
    return FSGM_OK;
}

fsgm_status fsgm_measure_copy_bandwidth(int32_t device, size_t bytes, int32_t iters, double* gbps) {
    return fsgm_measure_copy_bandwidth2(device, bytes, iters, 0, gbps);
}

void fsgm_pyd_shutdown_internal(void);
void fsgm_pyramid_shutdown_internal(void);
void fsgm_post_shutdown_internal(void);
void fsgm_ng_shutdown_internal(void);
void fsgm_ng_pyramid_shutdown_internal(void);
void fsgm_flow_pp_shutdown_internal(void);
void fsgm_stereo_pp_shutdown_internal(void);
void fsgm_sgm2d_shutdown_internal(void);
__attribute__((visibility("hidden"))) void fsgm_epi_shutdown_internal(void);   // (capi_epi.hip; not among the library's dynamic symbols)

void fsgm_shutdown(void) {
    fsgm_sgm2d_shutdown_internal();
    fsgm_stereo_pp_shutdown_internal();
    fsgm_flow_pp_shutdown_internal();
    fsgm_ng_pyramid_shutdown_internal();
    fsgm_ng_shutdown_internal();
    fsgm_post_shutdown_internal();
    fsgm_pyramid_shutdown_internal();
    fsgm_pyd_shutdown_internal();
    fsgm_epi_shutdown_internal();
}

}  // extern "C"
