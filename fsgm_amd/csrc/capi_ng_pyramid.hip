// capi_ng_pyramid.hip -- C ABI for the pyramidal level loop around calc_pyd_cost_sgm_ng (include/fsgm.h).
// pyramidal_sgm.m:24-76 with the neighbour-guided MEX in place of calc_pyd_cost_sgm (pyramid_driver.h holds the loop, the
// entry points and the plan cache).  The level scratch (ng_level_bufs: candidate lists at 12 B per entry, the sum volume,
// ...) is shared by the levels -- they run in order on one stream -- and sized for the finest.
#include "ng_kernels.h"
#include "pyramid_driver.h"
#include "flow_pp.h"

using namespace fsgm;

struct fsgm_ng_pyramid_plan {
    using Params = fsgm_ng_pyramid_params;
    static constexpr int max_batch = 1024;
    static constexpr const char *plan_name = "fsgm_ng_pyramid_plan", *entry_name = "fsgm_pyramidal_sgm_ng", *flow_name = "flow";
    PyramidCore core;
    Params prm{};
    std::vector<uint8_t*> dG0, dG1;                  // gray pair per level
    std::vector<double*> dMv;                        // hint map per level: [2][mvH][mvW]
    std::vector<uint32_t*> dMinC;                    // [h][w]
    uint32_t* dMinC2 = nullptr;                      // level 1's runner-up cost [H][W], made by set_runner_up
    NgLevelBufs nb{};

    static fsgm_status check(const Params& prm, int W, int H) {
        FSGM_REQUIRE(prm.halfSearchWinSize >= 0 && prm.aggSize >= 0, "halfSearchWinSize and aggSize must be >= 0");
        const long long D = 9LL * (2 * prm.halfSearchWinSize + 1) * (2 * prm.halfSearchWinSize + 1);
        if (D > FSGM_NG_MAX_D) return fail(FSGM_ERR_UNSUPPORTED, "%lld candidates per pixel exceed %d", D, FSGM_NG_MAX_D);
        if ((double)W * H * D >= 2147483648.0) return fail(FSGM_ERR_UNSUPPORTED, "candidate volume exceeds 2^31 entries");
        return FSGM_OK;
    }
    uint8_t*& gray(int img, int l) { return (img ? dG1 : dG0)[l]; }
    uint32_t*& minC(int l) { return dMinC[l]; }
    uint32_t*& minC2() { return dMinC2; }
    fsgm_status set_runner_up(int on) {
        if (on && !dMinC2) {                         // all ones until a WTA has run: FSGM_NO_RUNNER_UP
            const size_t bytes = (size_t)core.batch * core.W * core.H * 4;
            uint32_t* m = nullptr;
            FSGM_HIP(hipMalloc((void**)&m, bytes));
            const hipError_t e = hipMemsetAsync(m, 0xFF, bytes, core.stream);
            if (e != hipSuccess) { (void)hipFree(m); return hip_status(e, "fsgm_ng_pyramid_plan_set_runner_up"); }
            dMinC2 = m;
        }
        return FSGM_OK;
    }

    fsgm_status create_levels() {
        const int n = prm.numPyd, D = 9 * (2 * prm.halfSearchWinSize + 1) * (2 * prm.halfSearchWinSize + 1);
        const size_t B = core.batch;
        dG0.assign(n, nullptr); dG1.assign(n, nullptr); dMv.assign(n, nullptr); dMinC.assign(n, nullptr);
        hipError_t e = hipSuccess;
        for (int l = 0; l < n && e == hipSuccess; l++) {
            const size_t np = (size_t)core.Ws[l] * core.Hs[l], mv = (size_t)core.mvW[l] * core.mvH[l];
            e = hipMalloc((void**)&dG0[l], B * np);
            if (e == hipSuccess) e = hipMalloc((void**)&dG1[l], B * np);
            if (e == hipSuccess) e = hipMalloc((void**)&dMv[l], B * 2 * mv * sizeof(double));
            if (e == hipSuccess) e = hipMalloc((void**)&dMinC[l], B * np * 4);
        }
        for (const NgBuf& b : ng_level_bufs(nb, core.W, core.H, D, core.batch))
            if (e == hipSuccess && b.bytes) e = hipMalloc(b.slot, b.bytes);
        if (e == hipSuccess) e = hipMemset(dMv[n - 1], 0, B * 2 * (size_t)core.mvW[n - 1] * core.mvH[n - 1] * sizeof(double));   // :34
        return hip_status(e);
    }
    void destroy_levels() {
        for (auto* v : {&dG0, &dG1})
            for (uint8_t* b : *v) if (b) (void)hipFree(b);
        for (double* b : dMv) if (b) (void)hipFree(b);
        for (uint32_t* b : dMinC) if (b) (void)hipFree(b);
        if (dMinC2) (void)hipFree(dMinC2);
        for (const NgBuf& b : ng_level_bufs(nb, 0, 0, 0, 0)) if (*b.slot) (void)hipFree(*b.slot);     // (the slots only)
    }

    fsgm_status enqueue_level(int l) {
        const int w = core.Ws[l], h = core.Hs[l];
        const NgLevel lv = {dG0[l], dG1[l], dMv[l], dMinC[l], core.dFlow[l], w, h, core.mvW[l], core.mvH[l],
                            prm.halfSearchWinSize, prm.aggSize / 2, prm.P1, prm.P2, prm.subPixelRefine,
                            l == 0 && core.runner_up ? dMinC2 : nullptr};
        FSGM_HIP(ng_level_enqueue(core.stream, nb, lv, core.batch));
        const size_t stride = l > 0 ? (size_t)2 * core.mvW[l - 1] * core.mvH[l - 1] : 0;
        if (l > 0 && core.level_median)                                          // pyramidal_sgm.m:70-72, :70-71 live
            launch_pyr_median_upsample2(core.stream, core.dFlow[l], dMv[l - 1], w, h, core.batch, stride, core.level_median);
        else if (l > 0)                                                          // pyramidal_sgm.m:72
            launch_pyr_upsample2(core.stream, core.dFlow[l], dMv[l - 1], w, h, core.batch, stride);
        return FSGM_OK;
    }
};

static PyramidCache<fsgm_ng_pyramid_plan> g_ngpyr;

fsgm_status fsgm::ng_pyramid_with_pair(int n, int W, int H, int channels, const fsgm_ng_pyramid_params* prm, int ru, int lm, const PairBody& body) {
    return pyramid_with_pair(g_ngpyr, n, W, H, channels, prm, ru, lm, body);
}

extern "C" {

fsgm_ng_pyramid_params fsgm_ng_pyramid_params_default(void) {
    fsgm_ng_pyramid_params p;
    p.numPyd = 3;                      // test_psgm.m:33
    p.P1 = 6; p.P2 = 32;               // ng_sgm.m:7-8
    p.halfSearchWinSize = 1;           // ng_sgm.m:20
    p.aggSize = 2;
    p.subPixelRefine = 0;
    p.device = 0;
    return p;
}

void fsgm_ng_pyramid_plan_destroy(fsgm_ng_pyramid_plan* p) { pyramid_destroy(p); }

fsgm_status fsgm_ng_pyramid_plan_create(fsgm_ng_pyramid_plan** out, int32_t W, int32_t H, int32_t channels,
                                        const fsgm_ng_pyramid_params* prm) {
    return pyramid_create(out, W, H, channels, 1, prm);
}

// `batch` image pairs resident at once: every buffer holds `batch` frames, frame-major
fsgm_status fsgm_ng_pyramid_plan_create_batch(fsgm_ng_pyramid_plan** out, int32_t W, int32_t H, int32_t channels, int32_t batch,
                                              const fsgm_ng_pyramid_params* prm) {
    return pyramid_create(out, W, H, channels, batch, prm);
}

fsgm_status fsgm_ng_pyramid_plan_level_size(fsgm_ng_pyramid_plan* p, int32_t level, int32_t* w, int32_t* h) {
    return pyramid_level_size(p, level, w, h);
}

fsgm_status fsgm_ng_pyramid_plan_upload_frame(fsgm_ng_pyramid_plan* p, int32_t frame, const uint8_t* I0, const uint8_t* I1) {
    return pyramid_upload_frame(p, frame, I0, I1);
}

fsgm_status fsgm_ng_pyramid_plan_upload(fsgm_ng_pyramid_plan* p, const uint8_t* I0, const uint8_t* I1) {
    return pyramid_upload_frame(p, 0, I0, I1);
}

fsgm_status fsgm_ng_pyramid_plan_run(fsgm_ng_pyramid_plan* p) { return pyramid_run(p); }

fsgm_status fsgm_ng_pyramid_plan_download_frame(fsgm_ng_pyramid_plan* p, int32_t frame, int32_t level, double* flow, uint32_t* minC) {
    return pyramid_download_frame(p, frame, level, flow, minC);
}

fsgm_status fsgm_ng_pyramid_plan_download(fsgm_ng_pyramid_plan* p, int32_t level, double* flow, uint32_t* minC) {
    return pyramid_download_frame(p, 0, level, flow, minC);
}

fsgm_status fsgm_ng_pyramid_plan_time(fsgm_ng_pyramid_plan* p, int32_t warmup, int32_t iters, float* ms_avg) {
    return pyramid_time(p, warmup, iters, ms_avg);
}

fsgm_status fsgm_ng_pyramid_plan_set_runner_up(fsgm_ng_pyramid_plan* p, int32_t on) { return pyramid_set_runner_up(p, on); }

fsgm_status fsgm_ng_pyramid_plan_download_runner_up(fsgm_ng_pyramid_plan* p, int32_t frame, uint32_t* minC2) {
    return pyramid_download_runner_up(p, frame, minC2);
}

fsgm_status fsgm_ng_pyramid_plan_set_level_median(fsgm_ng_pyramid_plan* p, int32_t size) { return pyramid_set_level_median(p, size); }

void fsgm_ng_pyramid_shutdown_internal(void) { g_ngpyr.clear(); }

// one call = the whole loop; plans are cached per shape like fsgm_pyramidal_sgm_host's
fsgm_status fsgm_pyramidal_sgm_ng_host(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                       const fsgm_ng_pyramid_params* prm, double* flow, uint32_t* minC, double* const* flowPyd) {
    return pyramid_host(g_ngpyr, I0, I1, width, height, channels, prm, flow, minC, flowPyd);
}

fsgm_status fsgm_pyramidal_sgm_ng_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                         const fsgm_ng_pyramid_params* prm, double* flow, uint32_t* minC, void* stream, int32_t* status) {
    return pyramid_device(g_ngpyr, n, I0, I1, width, height, channels, prm, flow, minC, stream, status);
}

fsgm_status fsgm_pyramidal_sgm_ng_host_ru(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                          const fsgm_ng_pyramid_params* prm, double* flow, uint32_t* minC, uint32_t* minC2,
                                          double* const* flowPyd) {
    return pyramid_host(g_ngpyr, I0, I1, width, height, channels, prm, flow, minC, flowPyd, minC2, true);
}

fsgm_status fsgm_pyramidal_sgm_ng_device_ru(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                            const fsgm_ng_pyramid_params* prm, double* flow, uint32_t* minC, uint32_t* minC2, void* stream,
                                            int32_t* status) {
    return pyramid_device(g_ngpyr, n, I0, I1, width, height, channels, prm, flow, minC, stream, status, minC2, true);
}

fsgm_status fsgm_pyramidal_sgm_ng_host_lm(const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                          const fsgm_ng_pyramid_params* prm, int32_t level_median, double* flow, uint32_t* minC,
                                          uint32_t* minC2, double* const* flowPyd) {
    return pyramid_host(g_ngpyr, I0, I1, width, height, channels, prm, flow, minC, flowPyd, minC2, minC2 != nullptr,
                        level_median, true);
}

fsgm_status fsgm_pyramidal_sgm_ng_device_lm(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t width, int32_t height, int32_t channels,
                                            const fsgm_ng_pyramid_params* prm, int32_t level_median, double* flow, uint32_t* minC,
                                            uint32_t* minC2, void* stream, int32_t* status) {
    return pyramid_device(g_ngpyr, n, I0, I1, width, height, channels, prm, flow, minC, stream, status, minC2, minC2 != nullptr,
                          level_median, true);
}

}  // extern "C"
