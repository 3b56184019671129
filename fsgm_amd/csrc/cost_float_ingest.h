// cost_float_ingest.h -- caller-supplied cost volumes of float32 / float16 / bfloat16, already in HBM, into a plan's u8 C: the
// float siblings of sgm_ingest.h and sgm2d_ingest.h.  Every voxel is quantised in registers by the rule of include/fsgm.h
// (fsgm_cost_format: one fp32 multiply, one fp32 add, round to nearest even, clamp to 0..cost_bound) as it arrives; from there
// on the tile, the byte transposition and the stores are the u8 kernels'.  A voxel that the clamp changed, or a NaN, raises the
// device flag that a byte above the bound raises there.  Kernels: cost_float_ingest.hip.
#pragma once
#include "capi_common.h"
#include "sgm2d_ingest.h"

namespace fsgm {

// a checked fsgm_cost_format
struct CostFormat {
    int dtype = -1;                      // FSGM_COST_F32 / _F16 / _BF16; -1: none (the volume is u8)
    float scale = 1.0f, offset = 0.0f;
};
inline size_t cost_elem_size(int dtype) { return dtype == FSGM_COST_F32 ? 4 : 2; }

// NULL, an unknown dtype, a non-finite or zero scale, a non-finite offset, non-zero reserved words: FSGM_ERR_INVALID
fsgm_status check_cost_format(const char* who, const fsgm_cost_format* fmt, CostFormat* out);

// n volumes from src (elements of fmt.dtype, aligned on their size and no further; layout FSGM_COST_LAYOUT_HWD or _DHW) into
// dst (u8 [n][H][W][D], 16-byte aligned); *flag = 1 (flag may be NULL) when some voxel was flagged.  bound 1..255.
void launch_sgm_ingest_float(hipStream_t st, const void* src, const CostFormat& fmt, uint8_t* dst, int n, int W, int H, int D, int layout,
                             int bound, uint32_t* flag);
// the same for the 2-D matcher's volumes: layout a FSGM_COST2D_LAYOUT_*, dst a fsgm_pyd_plan's padded C, the padding written as 0
void launch_sgm2d_ingest_float(hipStream_t st, const void* src, const CostFormat& fmt, uint8_t* dst, int n, int W, int H, int Sx, int Sy,
                               int layout, int bound, uint32_t* flag);

// The host float forms' way in: n volumes of `voxels` elements each from the host array C, staged one frame at a time in a
// device buffer that lives for this call; ingest(staged, f) queues frame f's quantising pass on `st`.  Then the stream is
// drained and the flag read and cleared: a raised flag is FSGM_ERR_INVALID, before the caller has queued anything else.
template <class Ingest>
fsgm_status stage_float_volumes(hipStream_t st, const void* C, const CostFormat& fmt, int n, size_t voxels, uint32_t* flag, const char* who,
                                Ingest&& ingest) {
    const size_t bytes = voxels * cost_elem_size(fmt.dtype);
    void* staged = nullptr;
    FSGM_HIP(hipMalloc(&staged, bytes));
    uint32_t raised = 0;
    hipError_t e = hipSuccess;
    for (int f = 0; f < n && e == hipSuccess; f++) {
        e = hipMemcpyAsync(staged, static_cast<const char*>(C) + (size_t)f * bytes, bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) ingest(staged, f);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&raised, flag, sizeof(raised), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(raised), st);
    const hipError_t se = hipStreamSynchronize(st);              // (on every path: the staging buffer is freed below)
    (void)hipFree(staged);
    if (e != hipSuccess || se != hipSuccess) return hip_status(e != hipSuccess ? e : se, who);
    if (raised) return fail(FSGM_ERR_INVALID, "%s: a cost quantises outside 0..cost_bound, or is NaN", who);
    return FSGM_OK;
}

}  // namespace fsgm
