// capi_epi_driver.hip -- C ABI of what stands around the calc_cost_sgm matcher (include/fsgm.h): census alone, the coordinate maps
// of a geometry, and the epipolar drivers on host and device pointers -- epipolar_sgm_of and test.m's frame body -- all on cached
// plans (epi_plan.h).
#include "epi_plan.h"
#include "epi_kernels.h"
#include "geometry_kernels.h"
#include "post_kernels.h"
#include "post_plan.h"
#include "pyramid_kernels.h"

using namespace fsgm;

// ---- the dense half of the epipolar driver (dense part only) ----
static EpiGeomArgs geom_args(const fsgm_epi_geometry* g, int W, int H, double* Pd0, double* nd, double* off, double* rflow) {
    EpiGeomArgs a;
    for (int i = 0; i < 9; i++) { a.F[i] = g->F[i]; a.Hm[i] = g->H[i]; }
    a.ex = g->epipole[0]; a.ey = g->epipole[1]; a.direction = g->direction != 0;
    a.Pd0 = Pd0; a.nd = nd; a.off = off; a.rflow = rflow; a.W = W; a.H = H;
    return a;
}

// ---------------------------------------------------------------------------------------------
// The epipolar drivers: epipolar_sgm_of (the matcher, then the flow) and test.m's frame body (pp; :32-54), the geometry given:
// the matcher in vz-index mode, D1 = bestD/256, flow, the post-processing chain and flow2, all on the plan's stream
// ---------------------------------------------------------------------------------------------
// the arguments of both forms of test.m's frame body (pp: flow2 required) and of fsgm_epipolar_sgm_of_device
static fsgm_status driver_args(const char* who, bool pp, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H,
                               int32_t channels, const fsgm_epi_geometry* g, int32_t dMax, const fsgm_epi_params* prm, const double* flow,
                               const double* flow2, fsgm_epi_params* pr) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(I0 && I1 && g && flow && (flow2 || !pp), "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1 && dMax >= 1, "%s: width/height/dMax must be >= 1 (got %d x %d x %d)", who, W, H, dMax);
    FSGM_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 (gray) or 3 (RGB planes), got %d", who, channels);
    *pr = prm ? *prm : fsgm_epi_params_default();
    if (!pp) {
        FSGM_REQUIRE(pr->vz_to_disp && !pr->fb_check, "%s: the flow needs disparities (vz_to_disp = 1, fb_check = 0)", who);
    } else {
        FSGM_REQUIRE(!pr->fb_check, "%s: fb_check must be 0 (the chain does its own forward-backward check)", who);
        if ((double)n * W * H >= 2147483648.0)
            return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who, (double)n * W * H);
    }
    if (pp) pr->vz_to_disp = 0;                                                          // the chain works on vz indices
    return FSGM_OK;
}

// images in dI1 / dI2 and the maps in dPd0 / dNd / dOff / dRflow: the matcher (epipolar_sgm_of.m:45, test.m:36), then each
// frame's flow (epipolar_sgm_of.m:46-51) or (pp) test.m's flow (:38-42) and flow2 (:45-54); D1 [batch][H][W]
static fsgm_status enqueue_flow(fsgm_epi_plan* p, bool pp, int dMax, double vMax, double* flow, double* flow2, double* D1) {
    fsgm_status st = epi_enqueue(p, FSGM_STAGE_ALL);
    if (st != FSGM_OK) return st;
    const int W = p->W, H = p->H, nf = p->batch;
    const size_t NP = p->NP;
    if (!pp) {
        for (int f = 0; f < nf; f++)
            launch_epi_flow(p->stream, p->dBestD + f * NP, p->dNd + f * 2 * NP, p->dRflow + f * 2 * NP, flow + f * 3 * NP, W, H);
    } else {
        const double n = (double)dMax + 1.0;                                             // test.m:6
        const PostScratch s = post_plan_scratch(p->post);
        launch_vz_from_bestd(p->stream, p->dBestD, D1, (size_t)nf * NP);
        post_enqueue_batch(p->stream, s, nf, W, H, D1, p->dPd0, p->dNd, p->dOff, vMax, n, (double)dMax, s.B, s.D2, nullptr, nullptr);
        launch_epi_pp_flow(p->stream, D1, s.B, p->dOff, p->dNd, p->dRflow, flow, flow2, W, H, nf, vMax, n);
    }
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

// Host forms: on the plan's stream the n image pairs as gray (:35-38; RGB planes through one staging pair, reused in stream
// order) and each frame's coordinate maps (:24), the matcher (:45) and the flow (:46-51), the results down.
static fsgm_status host_drive(bool pp, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                              const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params& pr, double* flow,
                              double* flow2, double* D1, uint32_t* minC) {
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    EpiPlanKey key;
    key.W = W; key.H = H; key.D = dMax; key.batch = n; key.prm = pr;
    fsgm_status st = cached_plan(lk, &p, key);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_set_penalties(p, 6, 64, vMax)) != FSGM_OK) return st;       // epipolar_sgm_of.m:19, test.m:36
    if ((st = epi_ensure_driver_buffers(p, channels, pp, true)) != FSGM_OK) return st;
    const size_t NP = p->NP, np = (size_t)n * NP;
    StreamGuard guard(p->stream);
    if (channels == 1) {
        FSGM_HIP(hipMemcpyAsync(p->dI1, I0, np, hipMemcpyHostToDevice, p->stream));
        FSGM_HIP(hipMemcpyAsync(p->dI2, I1, np, hipMemcpyHostToDevice, p->stream));
    }
    for (int f = 0; f < n; f++) {
        if (channels == 3) {
            FSGM_HIP(hipMemcpyAsync(p->dRgb, I0 + f * 3 * NP, 3 * NP, hipMemcpyHostToDevice, p->stream));
            FSGM_HIP(hipMemcpyAsync(p->dRgb + 3 * NP, I1 + f * 3 * NP, 3 * NP, hipMemcpyHostToDevice, p->stream));
            launch_pyr_gray(p->stream, p->dRgb, p->dI1 + f * NP, W, H);
            launch_pyr_gray(p->stream, p->dRgb + 3 * NP, p->dI2 + f * NP, W, H);
        }
        launch_epi_maps(p->stream, geom_args(&g[f], W, H, p->dPd0 + f * 2 * NP, p->dNd + f * 2 * NP, p->dOff + f * NP, p->dRflow + f * 2 * NP));
    }
    if ((st = enqueue_flow(p, pp, dMax, vMax, p->dFlow, p->dFlow2, p->dD1)) != FSGM_OK) return st;
    FSGM_HIP(hipMemcpyAsync(flow, p->dFlow, np * 24, hipMemcpyDeviceToHost, p->stream));
    if (flow2) FSGM_HIP(hipMemcpyAsync(flow2, p->dFlow2, np * 24, hipMemcpyDeviceToHost, p->stream));
    if (D1) FSGM_HIP(hipMemcpyAsync(D1, p->dD1, np * 8, hipMemcpyDeviceToHost, p->stream));
    if (minC) FSGM_HIP(hipMemcpyAsync(minC, p->dMinC, np * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return epi_check_handoff(p);
}

// Device forms: the caller's arrays checked, the plan prepared before the join with the caller's stream, then on the plan's
// stream the caller's images as gray (:35-38, straight from its planes) and each frame's maps (:24, the geometry by value),
// with the caller's images and minC bound to the plan.
static fsgm_status device_drive(const char* who, bool pp, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H,
                                int32_t channels, const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                double* flow, double* flow2, double* D1, uint32_t* minC, void* stream, int32_t* status) {
    fsgm_epi_params pr;
    fsgm_status st = driver_args(who, pp, n, I0, I1, W, H, channels, g, dMax, prm, flow, flow2, &pr);
    if (st != FSGM_OK) return st;
    FSGM_DEVICE_SLOT(pr.device);
    if ((st = epi_plan_args(W, H, dMax, n, pr, FSGM_SAMPLING_VZ, 0)) != FSGM_OK) return st;
    const size_t NP = (size_t)W * H, np = (size_t)n * NP;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, pr.device, cs, {{I0, np * channels, 1, true, "I0"},
                                                     {I1, np * channels, 1, true, "I1"},
                                                     {flow, np * 24, 8, true, "flow"},
                                                     {pp ? flow2 : nullptr, np * 24, 8, pp, "flow2"},
                                                     {pp ? D1 : nullptr, np * 8, 8, false, "D1"},
                                                     {minC, np * 4, 4, false, "minC"},
                                                     {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    EpiPlanKey key;
    key.W = W; key.H = H; key.D = dMax; key.batch = n; key.prm = pr;
    if ((st = cached_plan(lk, &p, key)) != FSGM_OK) return st;
    if ((st = epi_ensure_driver_buffers(p, 1, pp)) != FSGM_OK) return st;
    if ((st = epi_device_prepare(p, 6, 64, vMax)) != FSGM_OK) return st;                 // epipolar_sgm_of.m:19, test.m:36
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        Bind<uint8_t> i1(p->dI1, channels == 1 ? const_cast<uint8_t*>(I0) : nullptr), i2(p->dI2, channels == 1 ? const_cast<uint8_t*>(I1) : nullptr);
        Bind<uint32_t> mc(p->dMinC, minC);
        if (channels == 3) {
            launch_pyr_gray(p->stream, I0, p->dI1, W, H, n);
            launch_pyr_gray(p->stream, I1, p->dI2, W, H, n);
        }
        for (int f = 0; f < n; f++)
            launch_epi_maps(p->stream, geom_args(&g[f], W, H, p->dPd0 + f * 2 * NP, p->dNd + f * 2 * NP, p->dOff + f * NP, p->dRflow + f * 2 * NP));
        const fsgm_status es = enqueue_flow(p, pp, dMax, vMax, flow, flow2, D1 ? D1 : p->dD1);
        if (es == FSGM_OK) launch_device_status(p->stream, p->dBandErr, nullptr, status);
        return es;
    });
}

extern "C" {

// census() of common.cpp:3-27 alone (the one function of the path that the reference's own sources pin here)
fsgm_status fsgm_census_host(const uint8_t* img, int32_t W, int32_t H, uint32_t* cen, int32_t device) {
    FSGM_REQUIRE(img && cen, "fsgm_census: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    EpiPlanKey key;
    key.W = W; key.H = H; key.D = 16; key.batch = 1;             // any dMax: only the image / census buffers are used
    key.prm.device = device;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, key);
    if (st != FSGM_OK) return st;
    if ((st = epi_ensure_cost_buffers(p)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);
    FSGM_HIP(hipMemcpyAsync(p->dI1, img, p->NP, hipMemcpyHostToDevice, p->stream));
    launch_census(p->stream, p->dI1, p->dCen1, W, H, 1);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(cen, p->dCen1, p->NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_epipolar_maps_host(const fsgm_epi_geometry* g, int32_t W, int32_t H, double* Pd0, double* normDirect,
                                    double* Offset, double* Rflow, int32_t device) {
    FSGM_REQUIRE(g && Pd0 && normDirect && Offset && Rflow, "fsgm_epipolar_maps: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    EpiPlanKey key;
    key.W = W; key.H = H; key.D = 16; key.batch = 1;             // any dMax: only the map buffers are used
    key.prm.device = device;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = cached_plan(lk, &p, key);
    if (st != FSGM_OK) return st;
    if ((st = epi_ensure_driver_buffers(p, 1)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);
    launch_epi_maps(p->stream, geom_args(g, W, H, p->dPd0, p->dNd, p->dOff, p->dRflow));
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(Pd0, p->dPd0, p->NP * 16, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(normDirect, p->dNd, p->NP * 16, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(Offset, p->dOff, p->NP * 8, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(Rflow, p->dRflow, p->NP * 16, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

fsgm_status fsgm_epipolar_sgm_of_host(const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                      const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                      double* flow, uint32_t* minC) {
    FSGM_REQUIRE(I0 && I1 && g && flow, "fsgm_epipolar_sgm_of: null argument");
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    FSGM_REQUIRE(channels == 1 || channels == 3, "channels must be 1 (gray) or 3 (RGB planes), got %d", channels);
    fsgm_epi_params pr = prm ? *prm : fsgm_epi_params_default();
    FSGM_REQUIRE(pr.vz_to_disp && !pr.fb_check, "fsgm_epipolar_sgm_of: the flow needs disparities (vz_to_disp = 1, fb_check = 0)");
    return host_drive(false, 1, I0, I1, W, H, channels, g, dMax, vMax, pr, flow, nullptr, nullptr, minC);
}

fsgm_status fsgm_epipolar_flow_pp_host(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                       const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                       double* flow, double* flow2, double* D1, uint32_t* minC) {
    fsgm_epi_params pr;
    fsgm_status st = driver_args("fsgm_epipolar_flow_pp_host", true, n, I0, I1, W, H, channels, g, dMax, prm, flow, flow2, &pr);
    if (st != FSGM_OK) return st;
    return host_drive(true, n, I0, I1, W, H, channels, g, dMax, vMax, pr, flow, flow2, D1, minC);
}

fsgm_status fsgm_epipolar_sgm_of_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                        const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                        double* flow, uint32_t* minC, void* stream, int32_t* status) {
    return device_drive("fsgm_epipolar_sgm_of_device", false, n, I0, I1, W, H, channels, g, dMax, vMax, prm, flow, nullptr, nullptr, minC,
                        stream, status);
}

fsgm_status fsgm_epipolar_flow_pp_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                         const fsgm_epi_geometry* g, int32_t dMax, double vMax, const fsgm_epi_params* prm,
                                         double* flow, double* flow2, double* D1, uint32_t* minC, void* stream, int32_t* status) {
    return device_drive("fsgm_epipolar_flow_pp_device", true, n, I0, I1, W, H, channels, g, dMax, vMax, prm, flow, flow2, D1, minC,
                        stream, status);
}

}  // extern "C"
