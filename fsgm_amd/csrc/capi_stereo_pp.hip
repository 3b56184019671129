// capi_stereo_pp.hip -- C ABI of the checked, filtered and filled disparity map of rectified stereo (include/fsgm.h,
// "Rectified stereo: checked, filtered and filled disparity maps"): the chain of test.m:45-50 behind fsgm_stereo_sgm's
// matcher, with the second-view map and the check as one row kernel (stereo_pp_kernels.hip), and those two stages on their own.
// The matcher runs through its own device-pointer entry point (fsgm_stereo_sgm_device_range) on this plan's stream: nothing
// of the matcher's plan is touched here.
#include "capi_common.h"
#include "capi_device.h"
#include "post_kernels.h"
#include "post_plan.h"
#include "stereo_pp_kernels.h"
#include <math.h>
#include <mutex>
#include <vector>

using namespace fsgm;

// Scratch for n maps of W x H: the chain's maps and union-find arrays (post_plan.h), the index map W, the matcher's raw
// outputs when the caller wants none, the negative-input flag and the host forms' status word.  The host forms' image and
// output maps come with the first host call.  Every entry point queues on `stream`: the scratch is used in stream order.
struct fsgm_stereo_pp_plan {
    int W = 0, H = 0, n = 0, device = 0;
    size_t NP = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DeviceJoin join;
    fsgm_post_plan* post = nullptr;
    double* dW = nullptr;
    int32_t* dDisp = nullptr;
    uint32_t* dMinC = nullptr;
    uint32_t* dNeg = nullptr;
    int32_t* dStatus = nullptr;
    uint8_t *dI1 = nullptr, *dI2 = nullptr;                      // host forms
    double *dPP = nullptr, *dChecked = nullptr, *dDisp2 = nullptr;
};

static void stereo_pp_plan_destroy(fsgm_stereo_pp_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);       // queued device-form work of an evicted plan (fsgm_epi_plan_destroy)
    void* bufs[] = {p->dW, p->dDisp, p->dMinC, p->dNeg, p->dStatus, p->dI1, p->dI2, p->dPP, p->dChecked, p->dDisp2};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (p->post) fsgm_post_plan_destroy(p->post);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    p->join.destroy();
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

static PlanCache<fsgm_stereo_pp_plan> g_spp(4, stereo_pp_plan_destroy);   // cached plans per device, under that device's lock

extern "C" void fsgm_stereo_pp_shutdown_internal(void) { g_spp.clear(); }

// what every entry point refuses before a device is touched
static fsgm_status map_args(const char* who, int32_t n, int32_t W, int32_t H, bool ok_ptrs, int32_t d_min, int32_t direction, int32_t device) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(ok_ptrs, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    FSGM_REQUIRE(direction == -1 || direction == 1, "%s: direction must be -1 (match at x - d) or +1 (x + d), got %d", who, direction);
    FSGM_REQUIRE(d_min >= -FSGM_D_MIN_LIMIT && d_min <= FSGM_D_MIN_LIMIT, "%s: |d_min| must be <= %d (got %d)", who, FSGM_D_MIN_LIMIT, d_min);
    if (W > STEREO_PP_MAX_WIDTH)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: width %d exceeds %d (the row kernel's LDS row of 8 * width bytes must stay within 64 KiB)", who,
                    W, STEREO_PP_MAX_WIDTH);
    if ((double)n * W * H >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who, (double)n * W * H);
    FSGM_DEVICE_SLOT(device);
    return FSGM_OK;
}

static fsgm_status pp_params(const char* who, const fsgm_stereo_pp_params* pp, fsgm_stereo_pp_params* q) {
    *q = pp ? *pp : fsgm_stereo_pp_params_default();
    FSGM_REQUIRE(!isnan(q->speckle_max_diff) && !isnan(q->speckle_max_size), "%s: speckle_max_diff / speckle_max_size must be numbers", who);
    FSGM_REQUIRE(q->fb_threshold >= 0.0, "%s: fb_threshold must be >= 0 (got %g)", who, q->fb_threshold);
    FSGM_REQUIRE(q->island_fraction >= 0.0 && q->island_fraction <= 1.0, "%s: island_fraction must be in [0, 1] (got %g)", who, q->island_fraction);
    FSGM_REQUIRE(q->in_fill == 0 || q->in_fill == 1, "%s: in_fill must be 0 or 1 (got %d)", who, q->in_fill);
    for (int32_t r : q->reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_stereo_pp_params must be zero", who);
    return FSGM_OK;
}

// the arguments of both forms of the whole call
static fsgm_status call_args(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                             const fsgm_stereo_params* prm, int32_t d_min, const fsgm_stereo_pp_params* pp, const double* disp_pp,
                             fsgm_stereo_params* sp, fsgm_stereo_pp_params* q) {
    *sp = prm ? *prm : fsgm_stereo_params_default();
    fsgm_status st = map_args(who, n, W, H, I1 && I2 && disp_pp, d_min, sp->direction, sp->device);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(dMax >= 1, "%s: dMax must be >= 1 (got %d)", who, dMax);
    FSGM_REQUIRE(!sp->fb_check, "%s: fb_check must be 0 (the chain does its own forward-backward check)", who);
    return pp_params(who, pp, q);
}

// The cached plan of this shape (the caller has checked the device's slot): `lk` holds its device's lock for the length of
// the call, the device is current.
static fsgm_status plan_get(std::unique_lock<std::mutex>& lk, fsgm_stereo_pp_plan** out, int W, int H, int n, int device) {
    fsgm_status st = use_device(device);
    if (st != FSGM_OK) return st;
    lk = std::unique_lock<std::mutex>(g_spp.mu(device));
    if ((*out = g_spp.find(device, [&](const fsgm_stereo_pp_plan* q) { return q->W == W && q->H == H && q->n == n; }))) return FSGM_OK;
    fsgm_stereo_pp_plan* p = new fsgm_stereo_pp_plan;
    p->W = W; p->H = H; p->n = n; p->device = device; p->NP = (size_t)W * H;
    const size_t np = p->NP * n;
    if ((st = post_plan_create_batch(&p->post, W, H, n, device, false)) != FSGM_OK) {
        stereo_pp_plan_destroy(p);
        return st;
    }
    hipError_t e = hipMalloc((void**)&p->dW, np * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dDisp, np * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dMinC, np * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dNeg, 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dStatus, 4);
    if (e == hipSuccess) e = hipMemset(p->dNeg, 0, 4);
    if (e == hipSuccess) e = hipMemset(p->dStatus, 0, 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e != hipSuccess) {
        stereo_pp_plan_destroy(p);
        return hip_status(e, "stereo post-processing plan");
    }
    g_spp.insert(device, p);
    *out = p;
    return FSGM_OK;
}

// the host forms' image and output maps, on first use
static fsgm_status ensure_host(fsgm_stereo_pp_plan* p, bool images) {
    const size_t np = p->NP * p->n;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** b, size_t bytes) { if (e == hipSuccess && !*b) e = hipMalloc(b, bytes); };
    if (images) {
        alloc((void**)&p->dI1, np);
        alloc((void**)&p->dI2, np);
    }
    for (double** b : {&p->dPP, &p->dChecked, &p->dDisp2}) alloc((void**)b, np * 8);
    return hip_status(e, "stereo post-processing plan");
}

// test.m:45-50 on the matcher's int32 true disparities * 256, all on `st`; each output may be null
static void chain_enqueue(hipStream_t st, fsgm_stereo_pp_plan* p, const fsgm_stereo_pp_params& q, int dMax, int d_min, int direction,
                          const int32_t* disp, double* disp_pp, double* disp_checked, double* disp2) {
    const int W = p->W, H = p->H, n = p->n;
    const size_t np = p->NP * n;
    const PostScratch s = post_plan_scratch(p->post);
    launch_stereo_index(st, disp, p->dW, np, d_min);                                                                        // w = bestD / 256
    launch_speckle_filter(st, p->dW, s.A, nullptr, s.parent, s.size, nullptr, W, H, q.speckle_max_diff, q.speckle_max_size, n);   // :45
    launch_stereo_row(st, s.A, s.D2, s.B, W, H, n, (double)d_min, (double)direction, q.fb_threshold, nullptr);              // :46-47
    launch_speckle_filter(st, s.B, s.A, nullptr, s.parent, s.size, nullptr, W, H, (double)dMax,
                          (double)((long long)H * W) * q.island_fraction, n);                                               // :48
    const double* filled = s.A;
    if (q.in_fill) {
        launch_scanline_in_fill(st, s.A, s.B, s.left, W, H, n);                                                             // :49
        filled = s.B;
    }
    launch_stereo_pack(st, filled, s.A, s.D2, disp_pp, disp_checked, disp2, np, (double)d_min);
}

static fsgm_status require_non_negative(const double* D1, size_t n, const char* who) {
    for (size_t i = 0; i < n; i++)
        if (D1[i] < 0.0) return fail(FSGM_ERR_INVALID, "%s: D1 must hold non-negative values or NaN (element %zu is %g)", who, i, D1[i]);
    return FSGM_OK;
}

// ---- the two stages on their own.  D2in null: the second-view map is made from D1 (row kernel; D2out and out may each be
// null); D2in given: the check alone against that map ----
static void stage_enqueue(hipStream_t st, int n, int W, int H, const double* D1, const double* D2in, int d_min, int direction, double thr,
                          double* out, double* D2out, uint32_t* neg) {
    if (D2in) launch_stereo_fb_check(st, D1, D2in, out, W, H, n, (double)d_min, (double)direction, thr);
    else launch_stereo_row(st, D1, D2out, out, W, H, n, (double)d_min, (double)direction, thr, neg);
}

static fsgm_status stage_host(const char* who, int32_t n, const double* D1, const double* D2in, int32_t W, int32_t H, int32_t d_min,
                              int32_t direction, double thr, double* out, double* D2out, int32_t device) {
    fsgm_status st = map_args(who, n, W, H, D1 && (out || D2out) && !(D2in && (D2out || !out)), d_min, direction, device);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(thr >= 0.0, "%s: thr must be >= 0 (got %g)", who, thr);
    const size_t np = (size_t)n * W * H;
    if ((st = require_non_negative(D1, np, who)) != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n, device)) != FSGM_OK) return st;
    const PostScratch s = post_plan_scratch(p->post);
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dW, D1, np * 8, hipMemcpyHostToDevice, p->stream));
    if (D2in) FSGM_HIP(hipMemcpyAsync(s.A, D2in, np * 8, hipMemcpyHostToDevice, p->stream));
    stage_enqueue(p->stream, n, W, H, p->dW, D2in ? s.A : nullptr, d_min, direction, thr, out ? s.B : nullptr, D2out ? s.D2 : nullptr, nullptr);
    FSGM_HIP(hipGetLastError());
    if (out) FSGM_HIP(hipMemcpyAsync(out, s.B, np * 8, hipMemcpyDeviceToHost, p->stream));
    if (D2out) FSGM_HIP(hipMemcpyAsync(D2out, s.D2, np * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

static fsgm_status stage_device(const char* who, int32_t n, const double* D1, const double* D2in, int32_t W, int32_t H, int32_t d_min,
                                int32_t direction, double thr, double* out, double* D2out, int32_t device, void* stream, int32_t* status) {
    fsgm_status st = map_args(who, n, W, H, D1 && (out || D2out) && !(D2in && (D2out || !out)), d_min, direction, device);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(thr >= 0.0, "%s: thr must be >= 0 (got %g)", who, thr);
    const size_t bytes = (size_t)n * W * H * 8;
    hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, device, cs, {{D1, bytes, 8, true, "D1"},
                                                  {D2in, bytes, 8, false, "D2"},
                                                  {out, bytes, 8, false, "the checked map"},
                                                  {D2out, bytes, 8, false, "the second-view map"},
                                                  {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n, device)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&] {
        stage_enqueue(p->stream, n, W, H, D1, D2in, d_min, direction, thr, out, D2out, status && !D2in ? p->dNeg : nullptr);
        if (status) launch_device_status(p->stream, nullptr, p->dNeg, status);   // (the check alone raises no flag: 0)
        return FSGM_OK;
    });
}

// ---- the uniqueness filter: what both forms refuse before a device is touched ----
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
static fsgm_status uniqueness_args(const char* who, int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W,
                                   int32_t H, int32_t planes, int32_t ratio, const double* out, int32_t device) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(map && minC && minC2 && out, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    FSGM_REQUIRE(planes == 1 || planes == 2, "%s: planes must be 1 (a map) or 2 (a flow), got %d", who, planes);
    FSGM_REQUIRE(ratio >= 0 && ratio <= 100, "%s: ratio must be in [0, 100] (got %d)", who, ratio);
    if ((double)n * planes * W * H >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames * planes * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who,
                    (double)n * planes * W * H);
    const size_t np = (size_t)n * W * H, nm = np * planes;
    FSGM_REQUIRE((const void*)out == (const void*)map || !ranges_overlap(out, nm * 8, map, nm * 8),
                 "%s: out must be map itself or not overlap it", who);
    FSGM_REQUIRE(!ranges_overlap(out, nm * 8, minC, np * 4) && !ranges_overlap(out, nm * 8, minC2, np * 4),
                 "%s: out must not overlap minC or minC2", who);
    FSGM_DEVICE_SLOT(device);
    return FSGM_OK;
}

static void uniqueness_enqueue(hipStream_t st, const double* map, const uint32_t* minC, const uint32_t* minC2, double* out, size_t np,
                               size_t frame_px, int planes, int ratio) {
    if (planes == 2) launch_flow_uniqueness(st, map, minC, minC2, out, np, frame_px, ratio);
    else launch_stereo_uniqueness(st, map, minC, minC2, out, np, ratio);
}

// both host forms (the cached plan is that of n * planes maps: its map scratch holds every plane)
static fsgm_status uniqueness_host(const char* who, int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W,
                                   int32_t H, int32_t planes, int32_t ratio, double* out, int32_t device) {
    fsgm_status st = uniqueness_args(who, n, map, minC, minC2, W, H, planes, ratio, out, device);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H, nm = np * planes;
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n * planes, device)) != FSGM_OK) return st;
    uint32_t* c2 = (uint32_t*)p->dDisp;                          // (the chain's int32 disparity scratch: at least np words)
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dW, map, nm * 8, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dMinC, minC, np * 4, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(c2, minC2, np * 4, hipMemcpyHostToDevice, p->stream));
    uniqueness_enqueue(p->stream, p->dW, p->dMinC, c2, p->dW, np, (size_t)W * H, planes, ratio);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(out, p->dW, nm * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

static fsgm_status uniqueness_device(const char* who, int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W,
                                     int32_t H, int32_t planes, int32_t ratio, double* out, int32_t device, void* stream, int32_t* status) {
    fsgm_status st = uniqueness_args(who, n, map, minC, minC2, W, H, planes, ratio, out, device);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H, nm = np * planes;
    hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, device, cs, {{map, nm * 8, 8, true, "map"},
                                                  {minC, np * 4, 4, true, "minC"},
                                                  {minC2, np * 4, 4, true, "minC2"},
                                                  {out, nm * 8, 8, true, "out"},
                                                  {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n, device)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&] {
        uniqueness_enqueue(p->stream, map, minC, minC2, out, np, (size_t)W * H, planes, ratio);
        if (status) launch_device_status(p->stream, nullptr, p->dNeg, status);   // (no flag is ever raised here: 0)
        return FSGM_OK;
    });
}

extern "C" {

fsgm_status fsgm_uniqueness_filter_host(int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W, int32_t H,
                                        int32_t ratio, double* out, int32_t device) {
    return uniqueness_host("fsgm_uniqueness_filter", n, map, minC, minC2, W, H, 1, ratio, out, device);
}

fsgm_status fsgm_uniqueness_filter_device(int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W, int32_t H,
                                          int32_t ratio, double* out, int32_t device, void* stream, int32_t* status) {
    return uniqueness_device("fsgm_uniqueness_filter_device", n, map, minC, minC2, W, H, 1, ratio, out, device, stream, status);
}

fsgm_status fsgm_uniqueness_filter_planes_host(int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W,
                                               int32_t H, int32_t planes, int32_t ratio, double* out, int32_t device) {
    return uniqueness_host("fsgm_uniqueness_filter_planes", n, map, minC, minC2, W, H, planes, ratio, out, device);
}

fsgm_status fsgm_uniqueness_filter_planes_device(int32_t n, const double* map, const uint32_t* minC, const uint32_t* minC2, int32_t W,
                                                 int32_t H, int32_t planes, int32_t ratio, double* out, int32_t device, void* stream,
                                                 int32_t* status) {
    return uniqueness_device("fsgm_uniqueness_filter_planes_device", n, map, minC, minC2, W, H, planes, ratio, out, device, stream, status);
}

fsgm_stereo_pp_params fsgm_stereo_pp_params_default(void) {
    fsgm_stereo_pp_params p;
    p.speckle_max_diff = 2.0;          // test.m:45
    p.speckle_max_size = 100.0;
    p.fb_threshold = 2.0;              // forward_backward_check.m:6
    p.island_fraction = 0.1;           // test.m:48
    p.in_fill = 1;                     // test.m:49
    for (int32_t& r : p.reserved) r = 0;
    return p;
}

fsgm_status fsgm_stereo_pp_launch_lds(int32_t W, uint64_t* row_lds) {
    FSGM_REQUIRE(row_lds, "fsgm_stereo_pp_launch_lds: null argument");
    FSGM_REQUIRE(W >= 1, "fsgm_stereo_pp_launch_lds: width must be >= 1 (got %d)", W);
    if (W > STEREO_PP_MAX_WIDTH)
        return fail(FSGM_ERR_UNSUPPORTED, "fsgm_stereo_pp_launch_lds: width %d exceeds %d (8 * width bytes must stay within 64 KiB)", W,
                    STEREO_PP_MAX_WIDTH);
    *row_lds = stereo_row_lds(W);
    return FSGM_OK;
}

fsgm_status fsgm_stereo_disp_from_first_host(int32_t n, const double* D1, int32_t W, int32_t H, int32_t d_min, int32_t direction, double* D2,
                                             int32_t device) {
    return stage_host("fsgm_stereo_disp_from_first", n, D1, nullptr, W, H, d_min, direction, 0.0, nullptr, D2, device);
}
fsgm_status fsgm_stereo_disp_from_first_device(int32_t n, const double* D1, int32_t W, int32_t H, int32_t d_min, int32_t direction, double* D2,
                                               int32_t device, void* stream, int32_t* status) {
    return stage_device("fsgm_stereo_disp_from_first_device", n, D1, nullptr, W, H, d_min, direction, 0.0, nullptr, D2, device, stream, status);
}
fsgm_status fsgm_stereo_fb_check_host(int32_t n, const double* D1, const double* D2, int32_t W, int32_t H, int32_t d_min, int32_t direction,
                                      double thr, double* D1checked, double* D2out, int32_t device) {
    FSGM_REQUIRE(D1checked, "fsgm_stereo_fb_check: null argument");
    return stage_host("fsgm_stereo_fb_check", n, D1, D2, W, H, d_min, direction, thr, D1checked, D2out, device);
}
fsgm_status fsgm_stereo_fb_check_device(int32_t n, const double* D1, const double* D2, int32_t W, int32_t H, int32_t d_min, int32_t direction,
                                        double thr, double* D1checked, double* D2out, int32_t device, void* stream, int32_t* status) {
    FSGM_REQUIRE(D1checked, "fsgm_stereo_fb_check_device: null argument");
    return stage_device("fsgm_stereo_fb_check_device", n, D1, D2, W, H, d_min, direction, thr, D1checked, D2out, device, stream, status);
}

fsgm_status fsgm_stereo_sgm_pp_host(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                    int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                    const fsgm_stereo_pp_params* pp, double* disp_pp, double* disp_checked, int32_t* disp, uint32_t* minC,
                                    double* disp2) {
    const char* who = "fsgm_stereo_sgm_pp";
    fsgm_stereo_params sp;
    fsgm_stereo_pp_params q;
    fsgm_status st = call_args(who, n, I1, I2, W, H, dMax, prm, d_min, pp, disp_pp, &sp, &q);
    if (st != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n, sp.device)) != FSGM_OK) return st;
    if ((st = ensure_host(p, true)) != FSGM_OK) return st;
    const size_t np = p->NP * n;
    hipStream_t s = p->stream;
    StreamGuard guard(s);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(p->dI1, I1, np, hipMemcpyHostToDevice, s));
    FSGM_HIP(hipMemcpyAsync(p->dI2, I2, np, hipMemcpyHostToDevice, s));
    if ((st = fsgm_stereo_sgm_device_range(n, p->dI1, p->dI2, W, H, dMax, P1, P2, &sp, opt, d_min, p->dDisp, p->dMinC, nullptr, nullptr, s,
                                           p->dStatus)) != FSGM_OK)
        return st;
    chain_enqueue(s, p, q, dMax, d_min, sp.direction, p->dDisp, p->dPP, disp_checked ? p->dChecked : nullptr, disp2 ? p->dDisp2 : nullptr);
    FSGM_HIP(hipGetLastError());
    int32_t status = 0;
    FSGM_HIP(hipMemcpyAsync(disp_pp, p->dPP, np * 8, hipMemcpyDeviceToHost, s));
    if (disp_checked) FSGM_HIP(hipMemcpyAsync(disp_checked, p->dChecked, np * 8, hipMemcpyDeviceToHost, s));
    if (disp) FSGM_HIP(hipMemcpyAsync(disp, p->dDisp, np * 4, hipMemcpyDeviceToHost, s));
    if (minC) FSGM_HIP(hipMemcpyAsync(minC, p->dMinC, np * 4, hipMemcpyDeviceToHost, s));
    if (disp2) FSGM_HIP(hipMemcpyAsync(disp2, p->dDisp2, np * 8, hipMemcpyDeviceToHost, s));
    FSGM_HIP(hipMemcpyAsync(&status, p->dStatus, 4, hipMemcpyDeviceToHost, s));
    FSGM_HIP(hipStreamSynchronize(s));
    guard.dismiss();
    if (status != 0) return fail((fsgm_status)status, "%s: the matcher reported a failed run (an aggregation hand-off gave up)", who);
    return FSGM_OK;
}

fsgm_status fsgm_stereo_sgm_pp_device(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                      const fsgm_stereo_pp_params* pp, double* disp_pp, double* disp_checked, int32_t* disp, uint32_t* minC,
                                      double* disp2, void* stream, int32_t* status) {
    const char* who = "fsgm_stereo_sgm_pp_device";
    fsgm_stereo_params sp;
    fsgm_stereo_pp_params q;
    fsgm_status st = call_args(who, n, I1, I2, W, H, dMax, prm, d_min, pp, disp_pp, &sp, &q);
    if (st != FSGM_OK) return st;
    hipStream_t cs = (hipStream_t)stream;
    const size_t np = (size_t)W * H * n;
    if ((st = device_check_args(who, sp.device, cs, {{I1, np, 1, true, "I1"},
                                                     {I2, np, 1, true, "I2"},
                                                     {disp_pp, np * 8, 8, true, "disp_pp"},
                                                     {disp_checked, np * 8, 8, false, "disp_checked"},
                                                     {disp, np * 4, 4, false, "disp"},
                                                     {minC, np * 4, 4, false, "minC"},
                                                     {disp2, np * 8, 8, false, "disp2"},
                                                     {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n, sp.device)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        // the images are read where they lie, the matcher writes the caller's disp / minC (the plan's when it wants none); it
        // joins the plan's stream in its turn and queues the status word, which the chain behind it leaves alone
        int32_t* d = disp ? disp : p->dDisp;
        const fsgm_status ms = fsgm_stereo_sgm_device_range(n, I1, I2, W, H, dMax, P1, P2, &sp, opt, d_min, d, minC ? minC : p->dMinC, nullptr,
                                                            nullptr, p->stream, status);
        if (ms != FSGM_OK) return ms;
        chain_enqueue(p->stream, p, q, dMax, d_min, sp.direction, d, disp_pp, disp_checked, disp2);
        return FSGM_OK;
    });
}

// Average milliseconds, warm, HIP events on the plan's stream, for host images as fsgm_stereo_sgm_pp_host takes them: ms[0]
// the matcher alone, ms[1] the chain behind it, ms[2] the fused row kernel on the chain's speckle-filtered map, ms[3] the
// two generic kernels (calc_disp_from_first + forward_backward_check of the epipolar chain) on the same map with explicit
// rectified maps Pd0 = (x + 1, y + 1), direction (direction, 0), O = 1 -- their disparity function differs (vzInd2Disp), so
// ms[2] against ms[3] compares cost, not results.
fsgm_status fsgm_stereo_sgm_pp_time(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                    int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                    const fsgm_stereo_pp_params* pp, int32_t warmup, int32_t iters, float* ms) {
    const char* who = "fsgm_stereo_sgm_pp_time";
    fsgm_stereo_params sp;
    fsgm_stereo_pp_params q;
    fsgm_status st = call_args(who, n, I1, I2, W, H, dMax, prm, d_min, pp, (const double*)ms, &sp, &q);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(iters >= 1 && warmup >= 0, "%s: iters must be >= 1 and warmup >= 0", who);
    std::unique_lock<std::mutex> lk;
    fsgm_stereo_pp_plan* p;
    if ((st = plan_get(lk, &p, W, H, n, sp.device)) != FSGM_OK) return st;
    if ((st = ensure_host(p, true)) != FSGM_OK) return st;
    const size_t NP = p->NP, np = NP * n;
    hipStream_t s = p->stream;
    const PostScratch sc = post_plan_scratch(p->post);
    // the generic kernels' maps, for the length of this call
    std::vector<double> hPd0(2 * np), hNd(2 * np), hO(np, 1.0);
    for (int f = 0; f < n; f++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)f * 2 * NP + (size_t)y * W + x;
                hPd0[i] = x + 1.0; hPd0[i + NP] = y + 1.0;
                hNd[i] = (double)sp.direction; hNd[i + NP] = 0.0;
            }
    double *dPd0 = nullptr, *dNd = nullptr, *dO = nullptr;
    auto release = [&] { for (double* b : {dPd0, dNd, dO}) if (b) (void)hipFree(b); };
    hipError_t e = hipMalloc((void**)&dPd0, np * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&dNd, np * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&dO, np * 8);
    if (e != hipSuccess) { release(); return hip_status(e, who); }
    auto run = [&]() -> fsgm_status {
        StreamGuard guard(s);
        FSGM_HIP(hipMemcpyAsync(p->dI1, I1, np, hipMemcpyHostToDevice, s));
        FSGM_HIP(hipMemcpyAsync(p->dI2, I2, np, hipMemcpyHostToDevice, s));
        FSGM_HIP(hipMemcpyAsync(dPd0, hPd0.data(), np * 16, hipMemcpyHostToDevice, s));
        FSGM_HIP(hipMemcpyAsync(dNd, hNd.data(), np * 16, hipMemcpyHostToDevice, s));
        FSGM_HIP(hipMemcpyAsync(dO, hO.data(), np * 8, hipMemcpyHostToDevice, s));
        fsgm_status r;
        if ((r = time_enqueues(s, p->ev0, p->ev1, warmup, iters, [&] {
                 return fsgm_stereo_sgm_device_range(n, p->dI1, p->dI2, W, H, dMax, P1, P2, &sp, opt, d_min, p->dDisp, p->dMinC, nullptr, nullptr, s, nullptr);
             }, &ms[0])) != FSGM_OK) return r;
        if ((r = time_enqueues(s, p->ev0, p->ev1, warmup, iters, [&]() -> fsgm_status {
                 chain_enqueue(s, p, q, dMax, d_min, sp.direction, p->dDisp, p->dPP, p->dChecked, p->dDisp2);
                 FSGM_HIP(hipGetLastError());
                 return FSGM_OK;
             }, &ms[1])) != FSGM_OK) return r;
        launch_stereo_index(s, p->dDisp, p->dW, np, d_min);
        launch_speckle_filter(s, p->dW, sc.A, nullptr, sc.parent, sc.size, nullptr, W, H, q.speckle_max_diff, q.speckle_max_size, n);
        if ((r = time_enqueues(s, p->ev0, p->ev1, warmup, iters, [&]() -> fsgm_status {
                 launch_stereo_row(s, sc.A, sc.D2, sc.B, W, H, n, (double)d_min, (double)sp.direction, q.fb_threshold, nullptr);
                 FSGM_HIP(hipGetLastError());
                 return FSGM_OK;
             }, &ms[2])) != FSGM_OK) return r;
        const PostGeom g{dPd0, dNd, dO, 0.3, (double)dMax + 1.0};
        if ((r = time_enqueues(s, p->ev0, p->ev1, warmup, iters, [&]() -> fsgm_status {
                 launch_disp_from_first(s, sc.A, sc.D2, g, W, H, n);
                 launch_fb_check(s, sc.A, sc.D2, sc.B, g, W, H, n);
                 FSGM_HIP(hipGetLastError());
                 return FSGM_OK;
             }, &ms[3])) != FSGM_OK) return r;
        FSGM_HIP(hipStreamSynchronize(s));
        guard.dismiss();
        return FSGM_OK;
    };
    st = run();
    release();
    return st;
}

}  // extern "C"
