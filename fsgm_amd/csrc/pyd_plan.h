// pyd_plan.h -- the device-resident plan behind the calc_pyd_cost_sgm entry points, shared between
// capi_pyd.hip (one MEX call = one level), capi_pyramid.hip (the pyramidal_sgm.m level loop,
// which writes images and hint maps straight into the level plans' HBM buffers) and capi_sgm2d.hip
// (aggregation + WTA on caller-supplied volumes).
#pragma once
#include "capi_common.h"
#include "capi_device.h"
#include <vector>

struct fsgm_pyd_plan {
    int W = 0, H = 0, mvW = 0, mvH = 0, rX = 0, rY = 0, rAgg = 0, batch = 0, device = 0;
    int Sx = 0, Sy = 0, D = 0;
    int RS = 0, PS = 0;                  // volume layout in HBM (pyd_kernels.h): row stride, bytes per pixel
    int P1 = 6, P2 = 32, diagonal = 1, totalPass = 2, adaptive = 0, subpixel = 0;   // pyramidal_sgm.m:15-22
    int cmax = 24;                       // upper bound of the values in dC
    int flags = 0;                       // fsgm::PYD_PLAN_* it was created with
    size_t NP = 0, N = 0, MV = 0;        // N = bytes of one volume (NP * PS)
    hipStream_t stream = nullptr;
    bool owns_stream = true;             // false when a pyramid plan lends its stream (capi_pyramid.hip)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *dI1 = nullptr, *dI2 = nullptr, *dC = nullptr, *dL = nullptr;
    uint32_t *dCen1 = nullptr, *dCen2 = nullptr, *dBestD = nullptr, *dMinC = nullptr, *dS = nullptr, *dDesc = nullptr;
    std::vector<uint8_t> stage;          // host staging for layout conversion of debug volumes
    double *dMv = nullptr, *dMvSub = nullptr;
    // what the entry points on caller-supplied volumes add (capi_sgm2d.hip), each made on first use
    uint8_t* dIngest = nullptr;          // the caller's bytes as they came from the host, ahead of the ingest kernel
    uint32_t* dIngestFlag = nullptr;     // raised by the ingest kernel: some byte was above the declared bound
    double* dFlow = nullptr;             // hint + window offset + mvSub, f64 [batch][2][NP] (the host form's)
    // the runner-up cost (fsgm_pyd_plan_set_runner_up): with the switch on the WTA also writes dMinC2, u32 [batch][NP], made on
    // first use and all ones (FSGM_NO_RUNNER_UP) until a WTA has run; the cost and aggregation kernels do not depend on it
    int runner_up = 0;
    uint32_t* dMinC2 = nullptr;
    // exact path arithmetic (fsgm_pyd_plan_set_exact): the kernels of pyd_exact.hip, whose path volumes hold y = L - C.  agg_exact
    // is the switch as the last queued aggregation saw it, i.e. what dL holds: a WTA alone is refused while the two differ
    int exact = 0, agg_exact = 0;
    bool mv_zero = false;                // dMv holds zeros (aggregation-only plans: the hints of a call without preMv)
    fsgm::DeviceJoin join;               // the events of the plan's device calls
    const char* agg_name = "";           // the aggregation pyd_enqueue last queued: "rows", "rows/wide", "generic", "generic/wrap", "generic/exact"
};

namespace fsgm {
// enqueue the FSGM_STAGE_* stages of one level on the plan's stream (no synchronisation);
// dS (may be null): debug tap for the summed path costs, u32 [batch][NP][D]
fsgm_status pyd_enqueue(fsgm_pyd_plan* p, int stages, uint32_t* dS);

// The search windows the 2-D kernels accept, checked before a device is touched: the sides, then the candidate count
// (two steps, so that fsgm_pyd_plan_create keeps its order of checks: sides, batch, count).
fsgm_status pyd_check_sides(int32_t rX, int32_t rY, int32_t rAgg);
fsgm_status pyd_check_count(int32_t rX, int32_t rY);

// fsgm_pyd_plan_create with creation flags.  PYD_PLAN_AGG_ONLY: a plan that never runs the cost stage -- no second image, no
// census codes, a zeroed hint map, and the first image only with PYD_PLAN_GUIDE (adaptive P2 reads it).
constexpr int PYD_PLAN_AGG_ONLY = 1, PYD_PLAN_GUIDE = 2;
fsgm_status pyd_plan_create_flags(fsgm_pyd_plan** out, int32_t W, int32_t H, int32_t mvW, int32_t mvH, int32_t rX, int32_t rY,
                                  int32_t rAgg, int32_t batch, int32_t device, int flags);
}  // namespace fsgm
