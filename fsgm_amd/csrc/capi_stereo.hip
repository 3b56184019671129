// capi_stereo.hip -- C ABI of rectified stereo on image pairs, in host memory or in HBM (include/fsgm.h: fsgm_stereo_sgm_host,
// fsgm_stereo_sgm_device, their _opts, _range and _ru forms and the second-view forms): n contiguous frames, images up, everything
// else as calc_cost_sgm, on a cached rectified plan (epi_plan.h).
#include "epi_plan.h"
#include "epi_kernels.h"
#include "epi_view2.h"

using namespace fsgm;

// the pipeline of this thread's last rectified-stereo one-shot call (fsgm_stereo_sgm_last_kernel), as fsgm_sgm_last_kernel's
static thread_local const char* g_stereo_kernel = "";

// the view-2 forms' own arguments (include/fsgm.h, "Second view"): disp2 required, minC_v2 and conf may be NULL
struct StereoView2 {
    int max_diff;
    uint32_t *disp2, *minC_v2;
    uint8_t* conf;
};
static fsgm_status stereo_view2_args(const char* who, const fsgm_stereo_params& sp, const StereoView2& v) {
    FSGM_REQUIRE(v.disp2, "%s: null disp2", who);
    FSGM_REQUIRE(v.max_diff >= 0, "%s: max_diff must be >= 0 (got %d)", who, v.max_diff);
    FSGM_REQUIRE(!sp.fb_check, "%s: fb_check = 1 is the forward-backward check of fsgm_stereo_sgm_host (the other door): not together with the second view", who);
    return FSGM_OK;
}
// the left-right check on a stereo call's outputs, int32 true disparities both
static void enqueue_stereo_view2_check(fsgm_epi_plan* p, int dir, int max_diff, int n, const uint32_t* disp, const uint32_t* disp2, uint8_t* conf) {
    View2CheckArgs k{};
    k.disp = disp; k.disp2 = disp2; k.conf = conf; k.W = p->W; k.H = p->H; k.dir = dir; k.max_diff = max_diff;
    k.add1 = k.add2 = 0; k.marker2 = 0x80000000u;
    if (!p->prm.subpixel) { k.pre1 = k.add1 = 256 * p->d_min; k.shift1 = 8; }   // (disp = 256 * d_min + the whole index, as the _range forms return it)
    launch_view2_check(p->stream, k, n);
}

// A checked call: the caller's parameters (never its NULL) and the key of the cached plan that serves it (key.prm: the plan's).
// The cached rectified plan is shared by every d_min (the key does not hold it): each stereo entry point sets the plan's shift
// under the plan's lock before it queues anything, the older ones to 0.
struct StereoCall {
    fsgm_stereo_params sp;
    EpiPlanKey key;
};
// the checks both forms share, none of which needs a device; v2: the view-2 forms' arguments, NULL in the others
static fsgm_status stereo_call(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                               const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min, const uint32_t* disp,
                               const uint32_t* minC, const uint32_t* minC2, const StereoView2* v2, StereoCall* c) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(I1 && I2 && disp && minC, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1 && dMax >= 1, "%s: width/height/dMax must be >= 1 (got %d x %d x %d)", who, W, H, dMax);
    const fsgm_stereo_params sp = c->sp = prm ? *prm : fsgm_stereo_params_default();
    FSGM_REQUIRE(sp.direction == -1 || sp.direction == 1, "%s: direction must be -1 (match at x - d) or +1 (x + d), got %d", who, sp.direction);
    fsgm_epi_options o;
    fsgm_status st = epi_read_options(who, opt, &o);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(d_min >= -FSGM_D_MIN_LIMIT && d_min <= FSGM_D_MIN_LIMIT, "%s: |d_min| must be <= %d (got %d)", who, FSGM_D_MIN_LIMIT, d_min);
    if (v2 && (st = stereo_view2_args(who, sp, *v2)) != FSGM_OK) return st;
    EpiPlanKey& k = c->key;
    k.W = W; k.H = H; k.D = dMax; k.batch = n;
    k.prm.paths = sp.paths; k.prm.subpixel = sp.subpixel; k.prm.fb_check = sp.fb_check; k.prm.device = sp.device; k.prm.vz_to_disp = 0;
    k.sampling = FSGM_SAMPLING_RECTIFIED; k.direction = sp.direction;
    k.adaptive = o.adaptive_p2; k.runner_up = minC2 != nullptr; k.view2_dir = v2 ? sp.direction : 0;
    return FSGM_OK;
}

// ranged: the _range forms, whose disp / disp2 leave as int32 true disparities
static fsgm_status stereo_host(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                               int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                               bool ranged, uint32_t* disp, uint32_t* minC, uint8_t* conf, uint32_t* disp2, uint32_t* minC2 = nullptr,
                               const StereoView2* v2 = nullptr) {
    StereoCall c;
    fsgm_status st = stereo_call(who, n, I1, I2, W, H, dMax, prm, opt, d_min, disp, minC, minC2, v2, &c);
    if (st != FSGM_OK) return st;
    const fsgm_stereo_params& sp = c.sp;
    const fsgm_epi_params& pr = c.key.prm;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    if ((st = cached_plan(lk, &p, c.key)) != FSGM_OK) return st;
    p->d_min = d_min;
    if ((st = fsgm_epi_plan_set_penalties(p, P1, P2, p->vMax)) != FSGM_OK) return st;
    if ((st = epi_ensure_cost_buffers(p)) != FSGM_OK) return st;
    if (v2 && v2->conf && (st = epi_ensure_view2_conf(p)) != FSGM_OK) return st;
    p->have_img.assign(n, 1);                                    // the pairs go up below, ahead of the kernels
    const size_t np = (size_t)n * p->NP;
    StreamGuard guard(p->stream);                                // every early exit drains the stream: the copies use caller memory
    FSGM_HIP(hipMemcpyAsync(p->dI1, I1, np, hipMemcpyHostToDevice, p->stream));
    FSGM_HIP(hipMemcpyAsync(p->dI2, I2, np, hipMemcpyHostToDevice, p->stream));
    if (v2) { View2Format fmt(p, d_min); st = epi_enqueue(p, FSGM_STAGE_ALL); }
    else st = epi_enqueue(p, FSGM_STAGE_ALL);
    if (st != FSGM_OK) return st;
    g_stereo_kernel = kPipelineName[p->pipe];
    if (ranged) {
        launch_stereo_range(p->stream, p->dBestD, pr.fb_check ? p->dD2 : nullptr, np, d_min);
        FSGM_HIP(hipGetLastError());
    }
    FSGM_HIP(hipMemcpyAsync(disp, p->dBestD, np * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(minC, p->dMinC, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (minC2) FSGM_HIP(hipMemcpyAsync(minC2, p->dMinC2, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (pr.fb_check && conf) FSGM_HIP(hipMemcpyAsync(conf, p->dConf, np, hipMemcpyDeviceToHost, p->stream));
    if (pr.fb_check && disp2) FSGM_HIP(hipMemcpyAsync(disp2, p->dD2, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (v2) {                                                    // (ranged: dBestD holds int32 true disparities by now)
        FSGM_HIP(hipMemcpyAsync(v2->disp2, p->dDisp2v, np * 4, hipMemcpyDeviceToHost, p->stream));
        if (v2->minC_v2) FSGM_HIP(hipMemcpyAsync(v2->minC_v2, p->dMinCv2, np * 4, hipMemcpyDeviceToHost, p->stream));
        if (v2->conf) {
            enqueue_stereo_view2_check(p, sp.direction, v2->max_diff, n, p->dBestD, p->dDisp2v, p->dConfV2);
            FSGM_HIP(hipGetLastError());
            FSGM_HIP(hipMemcpyAsync(v2->conf, p->dConfV2, np, hipMemcpyDeviceToHost, p->stream));
        }
    }
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return epi_check_handoff(p);
}

static fsgm_status stereo_device(const char* who, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax,
                                 int32_t P1, int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                 bool ranged, uint32_t* disp, uint32_t* minC, uint8_t* conf, uint32_t* disp2, void* stream,
                                 int32_t* status, uint32_t* minC2 = nullptr, const StereoView2* v2 = nullptr) {
    StereoCall c;
    fsgm_status st = stereo_call(who, n, I1, I2, W, H, dMax, prm, opt, d_min, disp, minC, minC2, v2, &c);
    if (st != FSGM_OK) return st;
    const fsgm_stereo_params& sp = c.sp;
    const fsgm_epi_params& pr = c.key.prm;
    const size_t np = (size_t)n * (size_t)W * (size_t)H;
    const bool fb = pr.fb_check != 0;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, pr.device, cs, {{I1, np, 1, true, "I1"},
                                                     {I2, np, 1, true, "I2"},
                                                     {disp, np * 4, 4, true, "disp"},
                                                     {minC, np * 4, 4, true, "minC"},
                                                     {minC2, np * 4, 4, false, "minC2"},
                                                     {fb ? conf : nullptr, np, 1, false, "conf"},
                                                     {fb ? disp2 : nullptr, np * 4, 4, false, "disp2"},
                                                     {v2 ? v2->disp2 : nullptr, np * 4, 4, v2 != nullptr, "disp2"},
                                                     // (the label carries the type for the reason given at fsgm_sgm_view2_dptr's table, capi_sgm.hip)
                                                     {v2 ? v2->minC_v2 : nullptr, np * 4, 4, false, "minC_v2 (u32)"},
                                                     {v2 ? v2->conf : nullptr, np, 1, false, "conf"},
                                                     {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    if ((st = cached_plan(lk, &p, c.key)) != FSGM_OK) return st;
    p->d_min = d_min;
    if ((st = epi_device_prepare(p, P1, P2, p->vMax)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        Bind<uint8_t> i1(p->dI1, const_cast<uint8_t*>(I1)), i2(p->dI2, const_cast<uint8_t*>(I2));
        Bind<uint32_t> bd(p->dBestD, disp), mc(p->dMinC, minC), d2(p->dD2, fb ? disp2 : nullptr), m2(p->dMinC2, minC2);
        Bind<uint8_t> cf(p->dConf, fb ? conf : nullptr);
        Bind<uint32_t> v2d(p->dDisp2v, v2 ? v2->disp2 : nullptr), v2m(p->dMinCv2, v2 ? v2->minC_v2 : nullptr);
        fsgm_status es;
        if (v2) { View2Format fmt(p, d_min); es = epi_enqueue(p, FSGM_STAGE_ALL); }
        else es = epi_enqueue(p, FSGM_STAGE_ALL);
        if (es != FSGM_OK) return es;
        g_stereo_kernel = kPipelineName[p->pipe];
        if (ranged) launch_stereo_range(p->stream, disp, fb ? disp2 : nullptr, np, d_min);
        if (v2 && v2->conf) enqueue_stereo_view2_check(p, sp.direction, v2->max_diff, n, disp, v2->disp2, v2->conf);
        launch_device_status(p->stream, p->dBandErr, nullptr, status);
        return FSGM_OK;
    });
}

extern "C" {

// ---- rectified stereo on host pointers: n contiguous frames, images up, everything else as calc_cost_sgm ----
fsgm_stereo_params fsgm_stereo_params_default(void) {
    fsgm_stereo_params p;
    p.paths = 4; p.subpixel = 1; p.fb_check = 0; p.direction = -1; p.device = 0;
    return p;
}

fsgm_status fsgm_stereo_sgm_host(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                 int32_t P2, const fsgm_stereo_params* prm, uint32_t* disp, uint32_t* minC, uint8_t* conf,
                                 uint32_t* disp2) {
    return fsgm_stereo_sgm_host_opts(n, I1, I2, W, H, dMax, P1, P2, prm, nullptr, disp, minC, conf, disp2);
}

fsgm_status fsgm_stereo_sgm_host_opts(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, uint32_t* disp,
                                      uint32_t* minC, uint8_t* conf, uint32_t* disp2) {
    return stereo_host("fsgm_stereo_sgm_host", n, I1, I2, W, H, dMax, P1, P2, prm, opt, 0, false, disp, minC, conf, disp2);
}

fsgm_status fsgm_stereo_sgm_host_range(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                       int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                       int32_t* disp, uint32_t* minC, uint8_t* conf, int32_t* disp2) {
    return stereo_host("fsgm_stereo_sgm_host_range", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                       (uint32_t*)disp2);
}

const char* fsgm_stereo_sgm_last_kernel(void) { return g_stereo_kernel; }

// the same through a cached plan with the runner-up switch on (never the plan of the call above: cached_plan's key)
fsgm_status fsgm_stereo_sgm_host_ru(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                    int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                    int32_t* disp, uint32_t* minC, uint32_t* minC2, uint8_t* conf, int32_t* disp2) {
    FSGM_REQUIRE(minC2, "fsgm_stereo_sgm_host_ru: null minC2");
    return stereo_host("fsgm_stereo_sgm_host_ru", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                       (uint32_t*)disp2, minC2);
}

// the second view from the same aggregated volume and the left-right check against it (include/fsgm.h, "Second view")
fsgm_status fsgm_stereo_sgm_view2_host(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                       int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                       int32_t max_diff, int32_t* disp, uint32_t* minC, uint32_t* minC2, int32_t* disp2,
                                       uint32_t* minC_v2, uint8_t* conf) {
    const StereoView2 v{max_diff, (uint32_t*)disp2, minC_v2, conf};
    return stereo_host("fsgm_stereo_sgm_view2_host", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, nullptr,
                       nullptr, minC2, &v);
}

fsgm_status fsgm_stereo_sgm_device(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                   int32_t P2, const fsgm_stereo_params* prm, uint32_t* disp, uint32_t* minC, uint8_t* conf,
                                   uint32_t* disp2, void* stream, int32_t* status) {
    return fsgm_stereo_sgm_device_opts(n, I1, I2, W, H, dMax, P1, P2, prm, nullptr, disp, minC, conf, disp2, stream, status);
}

fsgm_status fsgm_stereo_sgm_device_opts(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                        int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, uint32_t* disp,
                                        uint32_t* minC, uint8_t* conf, uint32_t* disp2, void* stream, int32_t* status) {
    return stereo_device("fsgm_stereo_sgm_device", n, I1, I2, W, H, dMax, P1, P2, prm, opt, 0, false, disp, minC, conf, disp2, stream, status);
}

fsgm_status fsgm_stereo_sgm_device_range(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                         int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                         int32_t* disp, uint32_t* minC, uint8_t* conf, int32_t* disp2, void* stream, int32_t* status) {
    return stereo_device("fsgm_stereo_sgm_device_range", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                         (uint32_t*)disp2, stream, status);
}

// fsgm_stereo_sgm_host_ru on device pointers: minC2 is written where it lies, by the WTA itself
fsgm_status fsgm_stereo_sgm_device_ru(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                      int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                      int32_t* disp, uint32_t* minC, uint32_t* minC2, uint8_t* conf, int32_t* disp2, void* stream,
                                      int32_t* status) {
    FSGM_REQUIRE(minC2, "fsgm_stereo_sgm_device_ru: null minC2");
    return stereo_device("fsgm_stereo_sgm_device_ru", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, conf,
                         (uint32_t*)disp2, stream, status, minC2);
}

// fsgm_stereo_sgm_view2_host on device pointers: disp2, minC_v2 and conf are written where they lie
fsgm_status fsgm_stereo_sgm_view2_dptr(int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t W, int32_t H, int32_t dMax, int32_t P1,
                                       int32_t P2, const fsgm_stereo_params* prm, const fsgm_epi_options* opt, int32_t d_min,
                                       int32_t max_diff, int32_t* disp, uint32_t* minC, uint32_t* minC2, int32_t* disp2,
                                       uint32_t* minC_v2, uint8_t* conf, void* stream, int32_t* status) {
    const StereoView2 v{max_diff, (uint32_t*)disp2, minC_v2, conf};
    return stereo_device("fsgm_stereo_sgm_view2_dptr", n, I1, I2, W, H, dMax, P1, P2, prm, opt, d_min, true, (uint32_t*)disp, minC, nullptr,
                         nullptr, stream, status, minC2, &v);
}

}  // extern "C"
