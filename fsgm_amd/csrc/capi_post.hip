// capi_post.hip -- C ABI for the post-processing functions the reference chains after SGM
// (test.m:45-50): speckle_filter.m, calc_disp_from_first.m, forward_backward_check.m,
// scanline_in_fill.m, vzInd2Disp.m.  One entry point per MATLAB function (host pointers in / out), a
// device-resident plan that runs the whole chain without leaving HBM, and the chain on a batch of maps (host
// pointers, or device pointers ordered on the caller's stream).
#include "capi_common.h"
#include "capi_device.h"
#include "post_kernels.h"
#include "post_plan.h"
#include <math.h>
#include <mutex>

using namespace fsgm;

// A plan for `batch` maps of W x H.  The scratch set (dA, dB, dD2, dParent, dSize, dLeft) is always there; the staging
// maps of the host entry points (dIn, dOut, dDisp, dPd0, dNd, dO) come with the first host call (a plan of batch 1
// made by fsgm_post_plan_create has them from the start), the labels' buffers only with batch 1.
struct fsgm_post_plan {
    int W = 0, H = 0, batch = 1, device = 0;
    size_t NP = 0;                       // pixels of one map
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double *dIn = nullptr, *dA = nullptr, *dB = nullptr, *dD2 = nullptr, *dOut = nullptr, *dDisp = nullptr;
    double *dPd0 = nullptr, *dNd = nullptr, *dO = nullptr;
    int32_t *dParent = nullptr, *dSize = nullptr, *dScan = nullptr, *dLabels = nullptr, *dLeft = nullptr;
    uint32_t* dNeg = nullptr;            // device chain: some D1 value was negative (cleared by the status kernel)
    DeviceJoin join;                     // device-pointer entry points: the events that order the plan's stream with the caller's
};

namespace fsgm {

// test.m:45-50 on nf maps: D1 -> filterD1 (out), filterD2, disp (may be null).  Every stage is one launch for the batch.
// filterD1 must not be s.A; it may be s.B (the last read of B is before the fill writes it).
void post_enqueue_batch(hipStream_t st, const PostScratch& s, int nf, int W, int H, const double* D1, const double* Pd0,
                        const double* nd, const double* O, double vMax, double n, double dMax, double* filterD1,
                        double* filterD2, double* disp, uint32_t* neg) {
    const PostGeom g{Pd0, nd, O, vMax, n};
    launch_speckle_filter(st, D1, s.A, nullptr, s.parent, s.size, nullptr, W, H, 2.0, 100.0, nf, neg);               // :45
    launch_disp_from_first(st, s.A, filterD2, g, W, H, nf);                                                           // :46
    launch_fb_check(st, s.A, filterD2, s.B, g, W, H, nf);                                                             // :47
    launch_speckle_filter(st, s.B, s.A, nullptr, s.parent, s.size, nullptr, W, H, dMax,
                          (double)H * (double)W / 10.0, nf);                                                          // :48 rows*cols/10 of one map
    launch_scanline_in_fill(st, s.A, filterD1, s.left, W, H, nf);                                                     // :49
    if (disp) launch_vzind2disp(st, filterD1, O, disp, (size_t)W * H * nf, vMax, n);                                  // :50
}

PostScratch post_plan_scratch(fsgm_post_plan* p) { return PostScratch{p->dA, p->dB, p->dD2, p->dParent, p->dSize, p->dLeft}; }

}  // namespace fsgm

static fsgm_status ensure_staging(fsgm_post_plan* p) {
    const size_t np = p->NP * p->batch;
    hipError_t e = hipSuccess;
    auto alloc = [&](double** b, size_t bytes) { if (e == hipSuccess && !*b) e = hipMalloc((void**)b, bytes); };
    for (double** b : {&p->dIn, &p->dOut, &p->dDisp, &p->dO}) alloc(b, np * 8);
    alloc(&p->dPd0, np * 16);
    alloc(&p->dNd, np * 16);
    return hip_status(e, "post-processing plan");
}

extern "C" {

void fsgm_post_plan_destroy(fsgm_post_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);       // queued device-form work of an evicted plan (fsgm_epi_plan_destroy)
    void* bufs[] = {p->dIn, p->dA, p->dB, p->dD2, p->dOut, p->dDisp, p->dPd0, p->dNd, p->dO,
                    p->dParent, p->dSize, p->dScan, p->dLabels, p->dLeft, p->dNeg};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    p->join.destroy();
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

}  // extern "C"

fsgm_status fsgm::post_plan_create_batch(fsgm_post_plan** out, int32_t W, int32_t H, int32_t batch, int32_t device, bool staging) {
    FSGM_REQUIRE(out, "fsgm_post_plan_create: null plan pointer");
    *out = nullptr;
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    FSGM_REQUIRE(batch >= 1, "n_frames must be >= 1 (got %d)", batch);
    if ((double)W * H * batch >= 2147483648.0) return fail(FSGM_ERR_UNSUPPORTED, "n_frames * width * height reaches 2^31 pixels");
    fsgm_status st = use_device(device);
    if (st != FSGM_OK) return st;
    fsgm_post_plan* p = new fsgm_post_plan;
    p->W = W; p->H = H; p->batch = batch; p->device = device; p->NP = (size_t)W * H;
    const size_t np = p->NP * batch;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** ptr, size_t bytes) { if (e == hipSuccess) e = hipMalloc(ptr, bytes); };
    for (double** b : {&p->dA, &p->dB, &p->dD2}) alloc((void**)b, np * 8);
    for (int32_t** b : {&p->dParent, &p->dSize, &p->dLeft}) alloc((void**)b, np * 4);
    if (batch == 1) {
        alloc((void**)&p->dLabels, p->NP * 4);
        alloc((void**)&p->dScan, (p->NP / 1024 + 2) * 4);
    }
    alloc((void**)&p->dNeg, 4);
    if (e == hipSuccess) e = hipMemset(p->dNeg, 0, 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e != hipSuccess) {
        fsgm_post_plan_destroy(p);
        return hip_status(e, "fsgm_post_plan_create");
    }
    if (staging && (st = ensure_staging(p)) != FSGM_OK) {
        fsgm_post_plan_destroy(p);
        return st;
    }
    *out = p;
    return FSGM_OK;
}

extern "C" {

fsgm_status fsgm_post_plan_create(fsgm_post_plan** out, int32_t W, int32_t H, int32_t device) {
    return post_plan_create_batch(out, W, H, 1, device, true);
}

fsgm_status fsgm_post_plan_upload(fsgm_post_plan* p, const double* D1, const double* Pd0, const double* normDirect, const double* O) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_HIP(hipSetDevice(p->device));
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    if (D1) FSGM_HIP(hipMemcpyAsync(p->dIn, D1, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    if (Pd0) FSGM_HIP(hipMemcpyAsync(p->dPd0, Pd0, p->NP * 16, hipMemcpyHostToDevice, p->stream));
    if (normDirect) FSGM_HIP(hipMemcpyAsync(p->dNd, normDirect, p->NP * 16, hipMemcpyHostToDevice, p->stream));
    if (O) FSGM_HIP(hipMemcpyAsync(p->dO, O, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

// test.m:45-50 on the uploaded maps: dIn -> dOut (filterD1), dD2 (filterD2), dDisp
static fsgm_status post_enqueue(fsgm_post_plan* p, double vMax, double n, double dMax) {
    post_enqueue_batch(p->stream, post_plan_scratch(p), p->batch, p->W, p->H, p->dIn, p->dPd0, p->dNd, p->dO, vMax, n, dMax,
                       p->dOut, p->dD2, p->dDisp, nullptr);
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

fsgm_status fsgm_post_plan_run(fsgm_post_plan* p, double vMax, double n, double dMax) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_HIP(hipSetDevice(p->device));
    return post_enqueue(p, vMax, n, dMax);
}

fsgm_status fsgm_post_plan_download(fsgm_post_plan* p, double* filterD1, double* filterD2, double* disp) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_HIP(hipSetDevice(p->device));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    if (filterD1) FSGM_HIP(hipMemcpy(filterD1, p->dOut, p->NP * 8, hipMemcpyDeviceToHost));
    if (filterD2) FSGM_HIP(hipMemcpy(filterD2, p->dD2, p->NP * 8, hipMemcpyDeviceToHost));
    if (disp) FSGM_HIP(hipMemcpy(disp, p->dDisp, p->NP * 8, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_post_plan_time(fsgm_post_plan* p, double vMax, double n, double dMax, int32_t warmup, int32_t iters, float* ms_avg) {
    FSGM_REQUIRE(p && ms_avg && iters >= 1 && warmup >= 0, "fsgm_post_plan_time: bad argument");
    FSGM_HIP(hipSetDevice(p->device));
    return time_enqueues(p->stream, p->ev0, p->ev1, warmup, iters, [&] { return post_enqueue(p, vMax, n, dMax); }, ms_avg);
}

// ---- one host-pointer entry point per MATLAB function, on a cached plan ----
static PlanCache<fsgm_post_plan> g_post(4, fsgm_post_plan_destroy);   // cached plans per device, under that device's lock

void fsgm_post_shutdown_internal(void) { g_post.clear(); }

// The cached plan per (W, H, batch) for an entry point: `lk` holds its device's lock for the length of the call, the device is
// current.  staging: the host entry points' maps are wanted (added to a cached plan that lacks them)
static fsgm_status cached_plan(std::unique_lock<std::mutex>& lk, fsgm_post_plan** out, int W, int H, int device, int batch = 1,
                               bool staging = true) {
    FSGM_DEVICE_SLOT(device);
    lk = std::unique_lock<std::mutex>(g_post.mu(device));
    *out = g_post.find(device, [&](const fsgm_post_plan* q) { return q->W == W && q->H == H && q->batch == batch; });
    if (*out) {
        if (hipSetDevice(device) != hipSuccess) return fail(FSGM_ERR_HIP, "hipSetDevice failed");
        return staging ? ensure_staging(*out) : FSGM_OK;
    }
    const fsgm_status st = post_plan_create_batch(out, W, H, batch, device, staging);
    if (st == FSGM_OK) g_post.insert(device, *out);
    return st;
}

static fsgm_status require_non_negative(const double* D1, size_t n, const char* fn) {
    for (size_t i = 0; i < n; i++)
        if (D1[i] < 0.0) return fail(FSGM_ERR_INVALID, "%s: D1 must hold non-negative values or NaN (element %zu is %g)", fn, i, D1[i]);
    return FSGM_OK;
}

fsgm_status fsgm_speckle_filter_host(const double* image, int32_t W, int32_t H, double maxDiff, double maxSpeckleSize,
                                     double* imageFiltered, int32_t* labelImage, int32_t device) {
    FSGM_REQUIRE(image && imageFiltered, "fsgm_speckle_filter: null argument");
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    fsgm_status st = cached_plan(lk, &p, W, H, device);
    if (st != FSGM_OK) return st;
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dIn, image, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    launch_speckle_filter(p->stream, p->dIn, p->dOut, labelImage ? p->dLabels : nullptr, p->dParent, p->dSize, p->dScan,
                          W, H, maxDiff, maxSpeckleSize);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(imageFiltered, p->dOut, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    if (labelImage) FSGM_HIP(hipMemcpyAsync(labelImage, p->dLabels, p->NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_calc_disp_from_first_host(const double* D1, int32_t W, int32_t H, const double* Pd0, const double* normDirect,
                                           const double* O, double vMax, double n, double* D2, int32_t device) {
    FSGM_REQUIRE(D1 && Pd0 && normDirect && O && D2, "fsgm_calc_disp_from_first: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1");
    fsgm_status st = require_non_negative(D1, (size_t)W * H, "fsgm_calc_disp_from_first");
    if (st != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    if ((st = cached_plan(lk, &p, W, H, device)) != FSGM_OK) return st;
    if ((st = fsgm_post_plan_upload(p, D1, Pd0, normDirect, O)) != FSGM_OK) return st;
    launch_disp_from_first(p->stream, p->dIn, p->dD2, PostGeom{p->dPd0, p->dNd, p->dO, vMax, n}, W, H);
    FSGM_HIP(hipGetLastError());
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(D2, p->dD2, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_forward_backward_check_host(const double* D1, const double* D2, int32_t W, int32_t H, const double* Pd0,
                                             const double* normDirect, const double* O, double vMax, double n,
                                             double* D1checked, int32_t device) {
    FSGM_REQUIRE(D1 && D2 && Pd0 && normDirect && O && D1checked, "fsgm_forward_backward_check: null argument");
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    fsgm_status st = cached_plan(lk, &p, W, H, device);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_post_plan_upload(p, D1, Pd0, normDirect, O)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dD2, D2, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    launch_fb_check(p->stream, p->dIn, p->dD2, p->dOut, PostGeom{p->dPd0, p->dNd, p->dO, vMax, n}, W, H);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(D1checked, p->dOut, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_scanline_in_fill_host(const double* input, int32_t W, int32_t H, double* output, int32_t device) {
    FSGM_REQUIRE(input && output, "fsgm_scanline_in_fill: null argument");
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    fsgm_status st = cached_plan(lk, &p, W, H, device);
    if (st != FSGM_OK) return st;
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dIn, input, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    launch_scanline_in_fill(p->stream, p->dIn, p->dOut, p->dLeft, W, H);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(output, p->dOut, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_vzind2disp_host(const double* w, const double* O, int32_t W, int32_t H, double vMax, double n, double* D, int32_t device) {
    FSGM_REQUIRE(w && O && D, "fsgm_vzind2disp: null argument");
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    fsgm_status st = cached_plan(lk, &p, W, H, device);
    if (st != FSGM_OK) return st;
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dIn, w, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dO, O, p->NP * 8, hipMemcpyHostToDevice, p->stream));
    launch_vzind2disp(p->stream, p->dIn, p->dO, p->dDisp, p->NP, vMax, n);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(D, p->dDisp, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_vmf_host(const double* flow, int32_t W, int32_t H, int32_t channels, double* flowMed, int32_t device) {
    FSGM_REQUIRE(flow && flowMed, "fsgm_vmf: null argument");
    FSGM_REQUIRE(channels >= 1 && channels <= 3, "fsgm_vmf: 1..3 channels (got %d)", channels);
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    fsgm_status st = cached_plan(lk, &p, W, H, device);
    if (st != FSGM_OK) return st;
    double* src[3] = {p->dIn, p->dA, p->dB};                     // one plane per scratch map
    double* dst[3] = {p->dOut, p->dD2, p->dDisp};
    for (int c = 0; c < channels; c++) {
        StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
        FSGM_HIP(hipMemcpyAsync(src[c], flow + (size_t)c * p->NP, p->NP * 8, hipMemcpyHostToDevice, p->stream));
        launch_vmf(p->stream, src[c], dst[c], W, H, 1);
        FSGM_HIP(hipMemcpyAsync(flowMed + (size_t)c * p->NP, dst[c], p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    }
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipStreamSynchronize(p->stream));
    return FSGM_OK;
}

fsgm_status fsgm_epi_postprocess_host(const double* D1, int32_t W, int32_t H, const double* Pd0, const double* normDirect,
                                      const double* O, double vMax, double n, double dMax,
                                      double* filterD1, double* filterD2, double* disp, int32_t device) {
    FSGM_REQUIRE(D1 && Pd0 && normDirect && O && filterD1, "fsgm_epi_postprocess: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1");
    fsgm_status st = require_non_negative(D1, (size_t)W * H, "fsgm_epi_postprocess");
    if (st != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    if ((st = cached_plan(lk, &p, W, H, device)) != FSGM_OK) return st;
    if ((st = fsgm_post_plan_upload(p, D1, Pd0, normDirect, O)) != FSGM_OK) return st;
    if ((st = post_enqueue(p, vMax, n, dMax)) != FSGM_OK) return st;
    return fsgm_post_plan_download(p, filterD1, filterD2, disp);
}

// ---- the chain on a batch of maps ----
static fsgm_status batch_args(const char* who, int32_t n_frames, int32_t W, int32_t H, bool ok_ptrs, int32_t device) {
    FSGM_REQUIRE(n_frames >= 1, "%s: n_frames must be >= 1 (got %d)", who, n_frames);
    FSGM_REQUIRE(ok_ptrs, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    if ((double)n_frames * W * H >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who, (double)n_frames * W * H);
    FSGM_DEVICE_SLOT(device);
    return FSGM_OK;
}

fsgm_status fsgm_epi_postprocess_batch_host(int32_t n_frames, const double* D1, int32_t W, int32_t H, const double* Pd0,
                                            const double* normDirect, const double* O, double vMax, double n, double dMax,
                                            double* filterD1, double* filterD2, double* disp, int32_t device) {
    const char* who = "fsgm_epi_postprocess_batch";
    fsgm_status st = batch_args(who, n_frames, W, H, D1 && Pd0 && normDirect && O && filterD1, device);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n_frames * W * H;
    if ((st = require_non_negative(D1, np, who)) != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    if ((st = cached_plan(lk, &p, W, H, device, n_frames, true)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dIn, D1, np * 8, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dPd0, Pd0, np * 16, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dNd, normDirect, np * 16, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dO, O, np * 8, hipMemcpyHostToDevice, p->stream));
    if ((st = post_enqueue(p, vMax, n, dMax)) != FSGM_OK) return st;
    FSGM_HIP(hipMemcpyAsync(filterD1, p->dOut, np * 8, hipMemcpyDeviceToHost, p->stream));
    if (filterD2) FSGM_HIP(hipMemcpyAsync(filterD2, p->dD2, np * 8, hipMemcpyDeviceToHost, p->stream));
    if (disp) FSGM_HIP(hipMemcpyAsync(disp, p->dDisp, np * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_epi_postprocess_device(int32_t n_frames, const double* D1, int32_t W, int32_t H, const double* Pd0,
                                        const double* normDirect, const double* O, double vMax, double n, double dMax,
                                        double* filterD1, double* filterD2, double* disp, int32_t device, void* stream,
                                        int32_t* status) {
    const char* who = "fsgm_epi_postprocess_device";
    fsgm_status st = batch_args(who, n_frames, W, H, D1 && Pd0 && normDirect && O && filterD1, device);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n_frames * W * H;
    hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, device, cs, {{D1, np * 8, 8, true, "D1"},
                                                  {Pd0, np * 16, 8, true, "Pd0"},
                                                  {normDirect, np * 16, 8, true, "normDirect"},
                                                  {O, np * 8, 8, true, "O"},
                                                  {filterD1, np * 8, 8, true, "filterD1"},
                                                  {filterD2, np * 8, 8, false, "filterD2"},
                                                  {disp, np * 8, 8, false, "disp"},
                                                  {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_post_plan* p;
    if ((st = cached_plan(lk, &p, W, H, device, n_frames, false)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&] {
        post_enqueue_batch(p->stream, post_plan_scratch(p), n_frames, W, H, D1, Pd0, normDirect, O, vMax, n, dMax, filterD1,
                           filterD2 ? filterD2 : p->dD2, disp, status ? p->dNeg : nullptr);
        if (status) launch_device_status(p->stream, nullptr, p->dNeg, status);
        return FSGM_OK;
    });
}

fsgm_status fsgm_vmf_device(int32_t n_frames, const double* flow, int32_t W, int32_t H, int32_t channels, double* flowMed,
                            int32_t device, void* stream) {
    const char* who = "fsgm_vmf_device";
    fsgm_status st = batch_args(who, n_frames, W, H, flow && flowMed, device);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(channels >= 1 && channels <= 3, "%s: 1..3 channels (got %d)", who, channels);
    const size_t nv = (size_t)n_frames * channels * W * H;
    hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, device, cs, {{flow, nv * 8, 8, true, "flow"}, {flowMed, nv * 8, 8, true, "flowMed"}})) != FSGM_OK)
        return st;
    launch_vmf(cs, flow, flowMed, W, H, n_frames * channels);   // no scratch: queued on the caller's stream itself
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

}  // extern "C"
