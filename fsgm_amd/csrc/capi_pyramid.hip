// capi_pyramid.hip -- C ABI for the pyramidal driver (include/fsgm.h): the level loop of pyramidal_sgm.m around one
// calc_pyd_cost_sgm plan per level (pyramid_driver.h holds the loop, the entry points and the plan cache).
#include "pyd_kernels.h"
#include "pyd_plan.h"
#include "pyramid_driver.h"
#include "flow_pp.h"

using namespace fsgm;

struct fsgm_pyramid_plan {
    using Params = fsgm_pyramid_params;
    static constexpr int max_batch = 4096;
    static constexpr const char *plan_name = "fsgm_pyramid_plan", *entry_name = "fsgm_pyramidal_sgm", *flow_name = "mv";
    PyramidCore core;
    Params prm{};
    std::vector<fsgm_pyd_plan*> lv;                  // one calc_pyd_cost_sgm plan per level: its dI1 / dI2 / dMinC are the level's

    static fsgm_status check(const Params&, int, int) { return FSGM_OK; }
    uint8_t*& gray(int img, int l) { return img ? lv[l]->dI2 : lv[l]->dI1; }
    uint32_t*& minC(int l) { return lv[l]->dMinC; }
    uint32_t*& minC2() { return lv[0]->dMinC2; }     // the last level's WTA takes it from its plan (PydWtaArgs::minC2)
    fsgm_status set_runner_up(int on) { return fsgm_pyd_plan_set_runner_up(lv[0], on); }

    fsgm_status create_levels() {
        const int n = prm.numPyd;
        lv.assign(n, nullptr);
        for (int l = 0; l < n; l++) {
            fsgm_status st = fsgm_pyd_plan_create(&lv[l], core.Ws[l], core.Hs[l], core.mvW[l], core.mvH[l], prm.horSearchHalfWinSize,
                                                  prm.verSearchHalfWinSize, prm.aggHalfWinSize, core.batch, prm.device);
            if (st != FSGM_OK) return st;
            fsgm_pyd_plan* q = lv[l];
            (void)hipStreamDestroy(q->stream);       // all levels run on the pyramid's stream, in order
            q->stream = core.stream; q->owns_stream = false;
            st = fsgm_pyd_plan_set_params(q, prm.P1, prm.P2, prm.enableDiagonal, prm.totalPass, prm.adaptiveP2, l == 0);   // :49
            if (st != FSGM_OK) return st;
        }
        return hip_status(hipMemset(lv[n - 1]->dMv, 0, (size_t)core.batch * 2 * lv[n - 1]->MV * sizeof(double)));     // :34
    }
    void destroy_levels() {
        for (fsgm_pyd_plan* q : lv) fsgm_pyd_plan_destroy(q);
    }

    fsgm_status enqueue_level(int l) {
        fsgm_pyd_plan* q = lv[l];
        fsgm_status st = pyd_enqueue(q, FSGM_STAGE_ALL, nullptr);                // :50
        if (st != FSGM_OK) return st;
        PyrFlowArgs a;
        a.bestD = q->dBestD; a.mvSub = q->dMvSub; a.mvPre = q->dMv; a.flow = core.dFlow[l];
        const bool median = l > 0 && core.level_median;                          // :70-71 live: the hints come from the filtered flow
        a.next = l > 0 && !median ? lv[l - 1]->dMv : nullptr;
        a.next_frame_stride = l > 0 ? 2 * lv[l - 1]->MV : 0;
        a.W = q->W; a.H = q->H; a.mvW = q->mvW; a.mvH = q->mvH;
        a.Sy = q->Sy; a.hor = prm.horSearchHalfWinSize; a.ver = prm.verSearchHalfWinSize;
        launch_pyr_flow(core.stream, a, core.batch);                              // :57-72
        if (median) launch_pyr_median_upsample2(core.stream, core.dFlow[l], lv[l - 1]->dMv, q->W, q->H, core.batch, 2 * lv[l - 1]->MV, core.level_median);
        return FSGM_OK;
    }
};

static PyramidCache<fsgm_pyramid_plan> g_pyr;

fsgm_status fsgm::pyd_pyramid_with_pair(int n, int W, int H, int channels, const fsgm_pyramid_params* prm, int ru, int lm, const PairBody& body) {
    return pyramid_with_pair(g_pyr, n, W, H, channels, prm, ru, lm, body);
}

extern "C" {

fsgm_pyramid_params fsgm_pyramid_params_default(void) {
    fsgm_pyramid_params p;
    p.numPyd = 5;                      // pyramidal_sgm.m:12
    p.P1 = 6; p.P2 = 32;               // :15-16
    p.aggHalfWinSize = 2;              // :17
    p.verSearchHalfWinSize = 5;        // :18
    p.horSearchHalfWinSize = 5;        // :19
    p.enableDiagonal = 1;              // :20
    p.totalPass = 2;                   // :21
    p.adaptiveP2 = 0;                  // :22
    p.device = 0;
    return p;
}

void fsgm_pyramid_plan_destroy(fsgm_pyramid_plan* p) { pyramid_destroy(p); }

fsgm_status fsgm_pyramid_plan_create(fsgm_pyramid_plan** out, int32_t W, int32_t H, int32_t channels,
                                     const fsgm_pyramid_params* prm) {
    return pyramid_create(out, W, H, channels, 1, prm);
}

// `batch` image pairs resident in one plan: every kernel of a level covers all of them (the level loop stays a
// sequence -- a level needs the level above -- but each of its launches has batch times the work)
fsgm_status fsgm_pyramid_plan_create_batch(fsgm_pyramid_plan** out, int32_t W, int32_t H, int32_t channels,
                                           const fsgm_pyramid_params* prm, int32_t batch) {
    return pyramid_create(out, W, H, channels, batch, prm);
}

fsgm_status fsgm_pyramid_plan_level_size(fsgm_pyramid_plan* p, int32_t level, int32_t* w, int32_t* h) {
    return pyramid_level_size(p, level, w, h);
}

fsgm_status fsgm_pyramid_plan_upload(fsgm_pyramid_plan* p, const uint8_t* I0, const uint8_t* I1) {
    return pyramid_upload_frame(p, 0, I0, I1);
}

fsgm_status fsgm_pyramid_plan_upload_frame(fsgm_pyramid_plan* p, int32_t frame, const uint8_t* I0, const uint8_t* I1) {
    return pyramid_upload_frame(p, frame, I0, I1);
}

fsgm_status fsgm_pyramid_plan_run(fsgm_pyramid_plan* p) { return pyramid_run(p); }

fsgm_status fsgm_pyramid_plan_sync(fsgm_pyramid_plan* p) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_HIP(hipSetDevice(p->prm.device));
    FSGM_HIP(hipStreamSynchronize(p->core.stream));
    return FSGM_OK;
}

fsgm_status fsgm_pyramid_plan_run_images(fsgm_pyramid_plan* p) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_HIP(hipSetDevice(p->prm.device));
    pyramid_enqueue_images(p);
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

fsgm_status fsgm_pyramid_plan_download(fsgm_pyramid_plan* p, int32_t level, double* mv, uint32_t* minC) {
    return pyramid_download_frame(p, 0, level, mv, minC);
}

fsgm_status fsgm_pyramid_plan_download_frame(fsgm_pyramid_plan* p, int32_t frame, int32_t level, double* mv, uint32_t* minC) {
    return pyramid_download_frame(p, frame, level, mv, minC);
}

fsgm_status fsgm_pyramid_plan_download_gray_frame(fsgm_pyramid_plan* p, int32_t frame, int32_t level, uint8_t* g0, uint8_t* g1) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(level >= 1 && level <= p->prm.numPyd, "level %d out of range 1..%d", level, p->prm.numPyd);
    FSGM_REQUIRE(frame >= 0 && frame < p->core.batch, "frame %d out of range (batch %d)", frame, p->core.batch);
    FSGM_HIP(hipSetDevice(p->prm.device));
    FSGM_HIP(hipStreamSynchronize(p->core.stream));
    const fsgm_pyd_plan* q = p->lv[level - 1];
    const size_t o = (size_t)frame * q->NP;
    if (g0) FSGM_HIP(hipMemcpy(g0, q->dI1 + o, q->NP, hipMemcpyDeviceToHost));
    if (g1) FSGM_HIP(hipMemcpy(g1, q->dI2 + o, q->NP, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

fsgm_status fsgm_pyramid_plan_download_gray(fsgm_pyramid_plan* p, int32_t level, uint8_t* g0, uint8_t* g1) {
    return fsgm_pyramid_plan_download_gray_frame(p, 0, level, g0, g1);
}

fsgm_status fsgm_pyramid_plan_time(fsgm_pyramid_plan* p, int32_t warmup, int32_t iters, float* ms_avg) {
    return pyramid_time(p, warmup, iters, ms_avg);
}

fsgm_status fsgm_pyramid_plan_set_runner_up(fsgm_pyramid_plan* p, int32_t on) { return pyramid_set_runner_up(p, on); }

fsgm_status fsgm_pyramid_plan_download_runner_up(fsgm_pyramid_plan* p, int32_t frame, uint32_t* minC2) {
    return pyramid_download_runner_up(p, frame, minC2);
}

fsgm_status fsgm_pyramid_plan_set_level_median(fsgm_pyramid_plan* p, int32_t size) { return pyramid_set_level_median(p, size); }

void fsgm_pyramid_shutdown_internal(void) { g_pyr.clear(); }

// one call = pyramidal_sgm(I0, I1, numPyd)
fsgm_status fsgm_pyramidal_sgm_host(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                    const fsgm_pyramid_params* prm, double* mv, uint32_t* minC, double* const* mvPyd) {
    return pyramid_host(g_pyr, I0, I1, width, height, channels, prm, mv, minC, mvPyd);
}

fsgm_status fsgm_pyramidal_sgm_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                      const fsgm_pyramid_params* prm, double* mv, uint32_t* minC, void* stream, int32_t* status) {
    return pyramid_device(g_pyr, n, I0, I1, width, height, channels, prm, mv, minC, stream, status);
}

fsgm_status fsgm_pyramidal_sgm_host_ru(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                       const fsgm_pyramid_params* prm, double* mv, uint32_t* minC, uint32_t* minC2, double* const* mvPyd) {
    return pyramid_host(g_pyr, I0, I1, width, height, channels, prm, mv, minC, mvPyd, minC2, true);
}

fsgm_status fsgm_pyramidal_sgm_device_ru(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                         const fsgm_pyramid_params* prm, double* mv, uint32_t* minC, uint32_t* minC2, void* stream,
                                         int32_t* status) {
    return pyramid_device(g_pyr, n, I0, I1, width, height, channels, prm, mv, minC, stream, status, minC2, true);
}

fsgm_status fsgm_pyramidal_sgm_host_lm(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                       const fsgm_pyramid_params* prm, int32_t level_median, double* mv, uint32_t* minC, uint32_t* minC2,
                                       double* const* mvPyd) {
    return pyramid_host(g_pyr, I0, I1, width, height, channels, prm, mv, minC, mvPyd, minC2, minC2 != nullptr, level_median, true);
}

fsgm_status fsgm_pyramidal_sgm_device_lm(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                         const fsgm_pyramid_params* prm, int32_t level_median, double* mv, uint32_t* minC, uint32_t* minC2,
                                         void* stream, int32_t* status) {
    return pyramid_device(g_pyr, n, I0, I1, width, height, channels, prm, mv, minC, stream, status, minC2, minC2 != nullptr,
                          level_median, true);
}

// ---- the level-hint kernel on its own: one entry point per MATLAB expression, like the post-processing layer ----
static fsgm_status hints_args(const char* who, int32_t n, const double* flow, int32_t W, int32_t H, int32_t size, double* next, int32_t device) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(flow && next, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    const fsgm_status st = level_median_check(who, size);
    if (st != FSGM_OK) return st;
    if (4.0 * n * W * H >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: 4 * n_frames * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who, 4.0 * n * W * H);
    FSGM_DEVICE_SLOT(device);
    return FSGM_OK;
}

static void hints_enqueue(hipStream_t st, int n, const double* flow, int W, int H, int size, double* next) {
    const size_t stride = 8 * (size_t)W * H;                 // `next` frames are contiguous: [2][2H][2W]
    if (size) launch_pyr_median_upsample2(st, flow, next, W, H, n, stride, size);
    else launch_pyr_upsample2(st, flow, next, W, H, n, stride);
}

fsgm_status fsgm_flow_level_hints_host(int32_t n, const double* flow, int32_t W, int32_t H, int32_t size, double* next, int32_t device) {
    fsgm_status st = hints_args("fsgm_flow_level_hints", n, flow, W, H, size, next, device);
    if (st != FSGM_OK || (st = use_device(device)) != FSGM_OK) return st;
    const size_t in_bytes = 2 * (size_t)n * W * H * sizeof(double);
    double* d = nullptr;                                     // the flows, then the hint maps (four times their size)
    FSGM_HIP(hipMalloc((void**)&d, 5 * in_bytes));
    hipError_t e = hipMemcpy(d, flow, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hints_enqueue(nullptr, n, d, W, H, size, d + in_bytes / sizeof(double));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(next, d + in_bytes / sizeof(double), 4 * in_bytes, hipMemcpyDeviceToHost);   // (waits for the kernel)
    (void)hipFree(d);
    return hip_status(e, "fsgm_flow_level_hints");
}

fsgm_status fsgm_flow_level_hints_device(int32_t n, const double* flow, int32_t W, int32_t H, int32_t size, double* next, int32_t device,
                                         void* stream) {
    const char* who = "fsgm_flow_level_hints_device";
    fsgm_status st = hints_args(who, n, flow, W, H, size, next, device);
    if (st != FSGM_OK) return st;
    const size_t nv = 2 * (size_t)n * W * H;
    hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, device, cs, {{flow, nv * 8, 8, true, "flow"}, {next, 4 * nv * 8, 8, true, "next"}})) != FSGM_OK) return st;
    hints_enqueue(cs, n, flow, W, H, size, next);            // no scratch: queued on the caller's stream itself
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

}  // extern "C"
