// capi_sgm2d.hip -- C ABI of the 2-D matcher on batches of caller-supplied cost volumes, in host memory or in HBM
// (include/fsgm.h: fsgm_sgm2d_batch_host, fsgm_sgm2d_device, fsgm_pyd_plan_ingest_cost_device, and their float forms).  Everything that can be
// refused without a device is refused first; behind that both forms take one cached aggregation-only fsgm_pyd_plan, bring
// the volumes into its padded layout with the kernels of sgm2d_ingest.hip and run pyd_enqueue's aggregation and WTA on it.
#include "capi_common.h"
#include "capi_device.h"
#include "pyd_kernels.h"
#include "pyd_plan.h"
#include "pyramid_kernels.h"
#include "cost_float_ingest.h"
#include "sgm2d_ingest.h"
#include <algorithm>
#include <mutex>
#include <string.h>
#include <vector>

using namespace fsgm;

namespace {

// a checked call: prm never the caller's NULL, guide non-NULL exactly with adaptive_p2, mvW x mvH the hint map's size
// (the image's without preMv)
struct Sgm2dCall {
    int n, W, H, rX, rY, P1, P2, mvW, mvH;
    fsgm_sgm2d_params prm;
    const uint8_t* C;
    const double* preMv;
    const uint8_t* guide;
    uint32_t *bestD, *minC;
    double *mvSub, *flow;
    uint32_t* S;
    uint32_t* minC2;                     // the _ru forms' runner-up cost (never NULL there), NULL in the plain forms; _exact: as given
    bool exact;                          // the _exact forms: exact path arithmetic (fsgm_pyd_plan_set_exact)
    CostFormat fmt;                      // the float forms: C holds elements of fmt.dtype (-1 in the u8 forms), quantised by the ingest
};

bool layout_ok(int layout) {
    return layout == FSGM_COST2D_LAYOUT_HWD || layout == FSGM_COST2D_LAYOUT_DHW || layout == FSGM_COST2D_LAYOUT_DHW_YX;
}

// the checks both forms share, none of which needs a device
fsgm_status sgm2d_args(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                       const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide, uint32_t* bestD,
                       uint32_t* minC, double* mvSub, double* flow, uint32_t* S, uint32_t* minC2, bool ru, bool exact, Sgm2dCall* c) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    FSGM_REQUIRE(rX >= 0 && rY >= 0, "%s: halfX/halfY must be >= 0 (got %d, %d)", who, rX, rY);
    FSGM_REQUIRE(!exact || (P1 >= 0 && P1 <= 255), "%s: exact path arithmetic needs P1 in 0..255 (got %d)", who, P1);
    FSGM_REQUIRE(!exact || (P2 >= 0 && P2 <= 255), "%s: exact path arithmetic needs P2 in 0..255 (got %d)", who, P2);
    fsgm_status st = pyd_check_sides(rX, rY, 0);
    if (st == FSGM_OK) st = pyd_check_count(rX, rY);
    if (st != FSGM_OK) return st;
    const int D = (2 * rX + 1) * (2 * rY + 1);
    if ((double)W * H * D >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: cost volume %d x %d x %d exceeds 2^31 voxels per frame", who, W, H, D);
    // (the ingest, aggregation, WTA and flow kernels take the frame as blockIdx.y)
    if (n > 65535) return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames %d exceeds 65535 (the frame is a grid dimension)", who, n);
    const fsgm_sgm2d_params sp = prm ? *prm : fsgm_sgm2d_params_default();
    FSGM_REQUIRE(layout_ok(sp.layout), "%s: layout must be FSGM_COST2D_LAYOUT_HWD (0), _DHW (1) or _DHW_YX (2), got %d", who, sp.layout);
    FSGM_REQUIRE(sp.cost_bound >= 1 && sp.cost_bound <= 255, "%s: cost_bound must be 1..255 (got %d)", who, sp.cost_bound);
    FSGM_REQUIRE(sp.totalPass >= 1 && sp.totalPass <= 2, "%s: totalPass must be 1 or 2 (got %d)", who, sp.totalPass);
    FSGM_REQUIRE(sp.diagonal == 0 || sp.diagonal == 1, "%s: diagonal must be 0 or 1 (got %d)", who, sp.diagonal);
    FSGM_REQUIRE(sp.adaptive_p2 == 0 || sp.adaptive_p2 == 1, "%s: adaptive_p2 must be 0 or 1 (got %d)", who, sp.adaptive_p2);
    FSGM_REQUIRE(sp.subpixel == 0 || sp.subpixel == 1, "%s: subpixel must be 0 or 1 (got %d)", who, sp.subpixel);
    for (int r : sp.reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_sgm2d_params must be zero", who);
    FSGM_REQUIRE(sp.device >= 0 && sp.device < FSGM_MAX_DEVICES, "%s: device %d out of range", who, sp.device);
    FSGM_REQUIRE(C && bestD && minC && mvSub, "%s: null argument (C, bestD, minC and mvSub are required)", who);
    FSGM_REQUIRE(!ru || minC2, "%s: null argument (minC2 is required)", who);
    FSGM_REQUIRE(!preMv || (mvW >= W && mvH >= H), "%s: preMv (%d x %d) must be at least as large as the image (%d x %d): the "
                 "reference indexes it with image coordinates (calc_pyd_cost_sgm.cpp:388-389)", who, mvW, mvH, W, H);
    FSGM_REQUIRE(!sp.adaptive_p2 || guide, "%s: adaptive_p2 needs the guide image (guide is NULL)", who);
    *c = Sgm2dCall{n, W, H, rX, rY, P1, P2, preMv ? mvW : W, preMv ? mvH : H, sp, C, preMv, sp.adaptive_p2 ? guide : nullptr,
                   bestD, minC, mvSub, flow, S, ru ? minC2 : nullptr, exact};
    return FSGM_OK;
}

// Aggregation-only plans (pyd_plan.h), keyed by shape, window, hint-map size, batch, device, whether a guide is held and the
// runner-up switch (a call that asks for minC2 never takes the plan of one that does not) and the exact switch (an exact call and a
// plain one never share a plan: its path volumes hold y = L - C, theirs L).
// The host and the device form share them: a call holds its device's lock for its length and queues on the plan's stream.
PlanCache<fsgm_pyd_plan> g_sgm2d(6, fsgm_pyd_plan_destroy);
thread_local const char* g_sgm2d_kernel = "";

// the cached plan of a checked call, with the call's parameters and `cmax` set; the device's lock is the caller's
fsgm_status sgm2d_plan(fsgm_pyd_plan** out, const Sgm2dCall& c, int cmax) {
    const int dev = c.prm.device, flags = PYD_PLAN_AGG_ONLY | (c.guide ? PYD_PLAN_GUIDE : 0), ru = c.minC2 != nullptr;
    fsgm_pyd_plan* p = g_sgm2d.find(dev, [&](const fsgm_pyd_plan* q) {
        return q->W == c.W && q->H == c.H && q->mvW == c.mvW && q->mvH == c.mvH && q->rX == c.rX && q->rY == c.rY && q->batch == c.n &&
               q->flags == flags && q->runner_up == ru && q->exact == (int)c.exact;
    });
    fsgm_status st;
    if (!p) {
        if ((st = pyd_plan_create_flags(&p, c.W, c.H, c.mvW, c.mvH, c.rX, c.rY, 0, c.n, dev, flags)) != FSGM_OK) return st;
        if (ru && (st = fsgm_pyd_plan_set_runner_up(p, 1)) != FSGM_OK) { fsgm_pyd_plan_destroy(p); return st; }
        if (c.exact && (st = fsgm_pyd_plan_set_exact(p, 1)) != FSGM_OK) { fsgm_pyd_plan_destroy(p); return st; }
        g_sgm2d.insert(dev, p);
    } else if ((st = use_device(dev)) != FSGM_OK) {
        return st;
    }
    if ((st = fsgm_pyd_plan_set_params(p, c.P1, c.P2, c.prm.diagonal, c.prm.totalPass, c.prm.adaptive_p2, c.prm.subpixel)) != FSGM_OK) return st;
    p->cmax = cmax;
    *out = p;
    return FSGM_OK;
}

// the scalar checks of both plan-level ingest entries, behind their null and format checks
fsgm_status pyd_ingest_args(const char* who, const fsgm_pyd_plan* p, int32_t n, int32_t layout, int32_t cost_bound) {
    FSGM_REQUIRE(n == p->batch, "%s: n_frames %d differs from the plan's batch %d", who, n, p->batch);
    FSGM_REQUIRE(layout_ok(layout), "%s: layout must be FSGM_COST2D_LAYOUT_HWD (0), _DHW (1) or _DHW_YX (2), got %d", who, layout);
    FSGM_REQUIRE(cost_bound >= 1 && cost_bound <= 255, "%s: cost_bound must be 1..255 (got %d)", who, cost_bound);
    return FSGM_OK;
}

// zero hints for a call without preMv: the plan's own map, cleared when an earlier host call left its hints there
fsgm_status zero_hints(fsgm_pyd_plan* p) {
    if (p->mv_zero) return FSGM_OK;
    FSGM_HIP(hipMemsetAsync(p->dMv, 0, (size_t)p->batch * p->MV * 16, p->stream));
    p->mv_zero = true;
    return FSGM_OK;
}

// aggregation + WTA on the plan's volume, then hint + window offset + mvSub (pyramidal_sgm.m:57-64) when a flow is wanted;
// dS, dFlow may be NULL.  The plan's slots hold whatever the caller bound.
fsgm_status sgm2d_enqueue(fsgm_pyd_plan* p, uint32_t* dS, double* dFlow) {
    const fsgm_status st = pyd_enqueue(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA, dS);
    if (st != FSGM_OK) return st;
    g_sgm2d_kernel = p->agg_name;
    if (dFlow) {
        PyrFlowArgs a;
        a.bestD = p->dBestD; a.mvSub = p->dMvSub; a.mvPre = p->dMv; a.flow = dFlow; a.next = nullptr;
        a.W = p->W; a.H = p->H; a.mvW = p->mvW; a.mvH = p->mvH; a.Sy = p->Sy; a.hor = p->rX; a.ver = p->rY; a.next_frame_stride = 0;
        launch_pyr_flow(p->stream, a, p->batch);
        FSGM_HIP(hipGetLastError());
    }
    return FSGM_OK;
}

// the host forms; ru: minC2 is wanted (the _ru form, where it is required, or an _exact call that passed one)
fsgm_status sgm2d_host(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                       const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide, uint32_t* bestD,
                       uint32_t* minC, uint32_t* minC2, bool ru, bool exact, double* mvSub, double* flow, uint32_t* S,
                       const CostFormat& fmt = CostFormat()) {
    Sgm2dCall c;
    fsgm_status st = sgm2d_args(who, n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, mvSub, flow, S, minC2, ru, exact, &c);
    if (st != FSGM_OK) return st;
    c.fmt = fmt;
    const bool is_float = fmt.dtype >= 0;
    // the true maximum of the batch (every layout holds the same bytes), as fsgm_pyd_plan_upload_cost takes it; a float volume
    // is not scanned: its declared bound selects the aggregation, as in the device forms
    const size_t NP = (size_t)W * H, ND = NP * (2 * rX + 1) * (2 * rY + 1);
    int cmax = c.prm.cost_bound;
    if (!is_float) {
        std::vector<int> fmax(n, 0);
        if ((st = frame_cost_maxima(who, C, n, ND, c.prm.cost_bound, fmax.data())) != FSGM_OK) return st;
        cmax = *std::max_element(fmax.begin(), fmax.end());
    }
    std::lock_guard<std::mutex> lk(g_sgm2d.mu(c.prm.device));
    fsgm_pyd_plan* p = nullptr;
    if ((st = sgm2d_plan(&p, c, cmax)) != FSGM_OK) return st;
    const size_t B = n;
    if (!is_float && !p->dIngest) FSGM_HIP(hipMalloc((void**)&p->dIngest, B * ND));
    if (is_float && (st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    if (S && !p->dS) FSGM_HIP(hipMalloc((void**)&p->dS, B * ND * 4));
    if (flow && !p->dFlow) FSGM_HIP(hipMalloc((void**)&p->dFlow, B * NP * 16));
    StreamGuard guard(p->stream);                                // every early exit drains the stream: the copies use caller memory
    // staged as it came, brought into the plan's layout by the kernel the device form runs (the scan above has checked the bound)
    if (is_float) {
        // staged frame by frame, quantised by the kernel the device form runs; the flag is read before any output is written
        const fsgm_status fs = stage_float_volumes(p->stream, C, fmt, n, ND, p->dIngestFlag, who, [&](const void* d, int f) {
            launch_sgm2d_ingest_float(p->stream, d, fmt, p->dC + (size_t)f * p->N, 1, W, H, p->Sx, p->Sy, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        });
        if (fs != FSGM_OK) return fs;
    } else {
        FSGM_HIP(hipMemcpyAsync(p->dIngest, C, B * ND, hipMemcpyHostToDevice, p->stream));
        launch_sgm2d_ingest(p->stream, p->dIngest, p->dC, n, W, H, p->Sx, p->Sy, c.prm.layout, 255, nullptr);
    }
    if (preMv) {
        FSGM_HIP(hipMemcpyAsync(p->dMv, preMv, B * p->MV * 16, hipMemcpyHostToDevice, p->stream));
        p->mv_zero = false;
    } else if ((st = zero_hints(p)) != FSGM_OK) {
        return st;
    }
    if (c.guide) FSGM_HIP(hipMemcpyAsync(p->dI1, c.guide, B * NP, hipMemcpyHostToDevice, p->stream));
    if ((st = sgm2d_enqueue(p, S ? p->dS : nullptr, flow ? p->dFlow : nullptr)) != FSGM_OK) return st;
    FSGM_HIP(hipMemcpyAsync(bestD, p->dBestD, B * NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(minC, p->dMinC, B * NP * 4, hipMemcpyDeviceToHost, p->stream));
    if (c.minC2) FSGM_HIP(hipMemcpyAsync(c.minC2, p->dMinC2, B * NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(mvSub, p->dMvSub, B * NP * 16, hipMemcpyDeviceToHost, p->stream));
    if (flow) FSGM_HIP(hipMemcpyAsync(flow, p->dFlow, B * NP * 16, hipMemcpyDeviceToHost, p->stream));
    if (S) FSGM_HIP(hipMemcpyAsync(S, p->dS, B * ND * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

// the device forms; ru as above: minC2 is written where it lies by the WTA itself
fsgm_status sgm2d_device(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                         const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide, uint32_t* bestD,
                         uint32_t* minC, uint32_t* minC2, bool ru, bool exact, double* mvSub, double* flow, uint32_t* S, void* stream, int32_t* status,
                         const CostFormat& fmt = CostFormat()) {
    Sgm2dCall c;
    fsgm_status st = sgm2d_args(who, n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, mvSub, flow, S, minC2, ru, exact, &c);
    if (st != FSGM_OK) return st;
    c.fmt = fmt;
    const size_t np = (size_t)n * W * H, nv = np * (2 * rX + 1) * (2 * rY + 1), nmv = (size_t)n * c.mvW * c.mvH;
    const size_t es = fmt.dtype >= 0 ? cost_elem_size(fmt.dtype) : 1;    // the volume's element size: its alignment
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, c.prm.device, cs, {{C, nv * es, es, true, "C"},
                                                        {preMv, nmv * 16, 8, false, "preMv"},
                                                        {c.guide, np, 1, false, "guide"},
                                                        {bestD, np * 4, 4, true, "bestD"},
                                                        {minC, np * 4, 4, true, "minC"},
                                                        {c.minC2, np * 4, 4, ru, "minC2"},
                                                        {mvSub, np * 16, 8, true, "mvSub"},
                                                        {flow, np * 16, 8, false, "flow"},
                                                        {S, nv * 4, 4, false, "S"},
                                                        {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::lock_guard<std::mutex> lk(g_sgm2d.mu(c.prm.device));
    fsgm_pyd_plan* p = nullptr;
    // The device cannot be asked for the true maximum without a wait: the declared bound selects the aggregation, the ingest
    // kernel saturates at it.  What a warm call must not do (allocate) happens before the join with the caller's stream.
    if ((st = sgm2d_plan(&p, c, c.prm.cost_bound)) != FSGM_OK) return st;
    if ((st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        if (fmt.dtype >= 0) launch_sgm2d_ingest_float(p->stream, C, fmt, p->dC, n, W, H, p->Sx, p->Sy, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        else launch_sgm2d_ingest(p->stream, C, p->dC, n, W, H, p->Sx, p->Sy, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        if (!preMv) {
            const fsgm_status zs = zero_hints(p);
            if (zs != FSGM_OK) return zs;
        }
        // the caller's arrays stand in the plan's slots for the length of the enqueue
        Bind<double> mv(p->dMv, const_cast<double*>(preMv)), ms(p->dMvSub, mvSub);
        Bind<uint8_t> i1(p->dI1, const_cast<uint8_t*>(c.guide));
        Bind<uint32_t> bd(p->dBestD, bestD), mc(p->dMinC, minC), m2(p->dMinC2, c.minC2);
        const fsgm_status es = sgm2d_enqueue(p, S, flow);
        if (es != FSGM_OK) return es;
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

}  // namespace

extern "C" {

void fsgm_sgm2d_shutdown_internal(void) { g_sgm2d.clear(); }

fsgm_sgm2d_params fsgm_sgm2d_params_default(void) {
    fsgm_sgm2d_params p;
    memset(&p, 0, sizeof(p));
    p.diagonal = 1;                      // pyramidal_sgm.m:15-22
    p.totalPass = 2;
    p.subpixel = 1;
    p.layout = FSGM_COST2D_LAYOUT_HWD;
    p.cost_bound = 255;
    return p;
}

const char* fsgm_sgm2d_last_kernel(void) { return g_sgm2d_kernel; }

fsgm_status fsgm_sgm2d_batch_host(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                                  const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide,
                                  uint32_t* bestD, uint32_t* minC, double* mvSub, double* flow, uint32_t* S) {
    return sgm2d_host("fsgm_sgm2d_batch_host", n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, nullptr, false, false, mvSub,
                      flow, S);
}

fsgm_status fsgm_sgm2d_batch_host_ru(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                                     const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide,
                                     uint32_t* bestD, uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow, uint32_t* S) {
    return sgm2d_host("fsgm_sgm2d_batch_host_ru", n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, minC2, true, false, mvSub,
                      flow, S);
}

fsgm_status fsgm_sgm2d_device(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                              const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide,
                              uint32_t* bestD, uint32_t* minC, double* mvSub, double* flow, uint32_t* S, void* stream, int32_t* status) {
    return sgm2d_device("fsgm_sgm2d_device", n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, nullptr, false, false, mvSub,
                        flow, S, stream, status);
}

fsgm_status fsgm_sgm2d_device_ru(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                                 const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide,
                                 uint32_t* bestD, uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow, uint32_t* S, void* stream,
                                 int32_t* status) {
    return sgm2d_device("fsgm_sgm2d_device_ru", n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, minC2, true, false, mvSub,
                        flow, S, stream, status);
}

// exact path arithmetic: minC2 may be NULL (not wanted); one pair of entries with and without the runner-up cost
fsgm_status fsgm_sgm2d_batch_host_exact(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                                        const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide,
                                        uint32_t* bestD, uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow, uint32_t* S) {
    return sgm2d_host("fsgm_sgm2d_batch_host_exact", n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, minC2,
                      minC2 != nullptr, true, mvSub, flow, S);
}

fsgm_status fsgm_sgm2d_device_exact(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t rX, int32_t rY, int32_t P1, int32_t P2,
                                    const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH, const uint8_t* guide,
                                    uint32_t* bestD, uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow, uint32_t* S,
                                    void* stream, int32_t* status) {
    return sgm2d_device("fsgm_sgm2d_device_exact", n, C, W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, minC2,
                        minC2 != nullptr, true, mvSub, flow, S, stream, status);
}

// The float forms (include/fsgm.h, "Float cost volumes"): the format is checked first, then the u8 forms' bodies run with it;
// minC2 is wanted when given, exact is a switch.
fsgm_status fsgm_sgm2d_float_batch_host(int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t W, int32_t H, int32_t rX, int32_t rY,
                                        int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH,
                                        const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow,
                                        uint32_t* S, int32_t exact) {
    const char* who = "fsgm_sgm2d_float_batch_host";
    FSGM_REQUIRE(exact == 0 || exact == 1, "%s: exact must be 0 or 1 (got %d)", who, exact);
    CostFormat cf;
    const fsgm_status st = check_cost_format(who, fmt, &cf);
    if (st != FSGM_OK) return st;
    return sgm2d_host(who, n, static_cast<const uint8_t*>(C), W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, minC2,
                      minC2 != nullptr, exact != 0, mvSub, flow, S, cf);
}

fsgm_status fsgm_sgm2d_float_dptr(int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t W, int32_t H, int32_t rX, int32_t rY,
                                  int32_t P1, int32_t P2, const fsgm_sgm2d_params* prm, const double* preMv, int32_t mvW, int32_t mvH,
                                  const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2, double* mvSub, double* flow,
                                  uint32_t* S, int32_t exact, void* stream, int32_t* status) {
    const char* who = "fsgm_sgm2d_float_dptr";
    FSGM_REQUIRE(exact == 0 || exact == 1, "%s: exact must be 0 or 1 (got %d)", who, exact);
    CostFormat cf;
    const fsgm_status st = check_cost_format(who, fmt, &cf);
    if (st != FSGM_OK) return st;
    return sgm2d_device(who, n, static_cast<const uint8_t*>(C), W, H, rX, rY, P1, P2, prm, preMv, mvW, mvH, guide, bestD, minC, minC2,
                        minC2 != nullptr, exact != 0, mvSub, flow, S, stream, status, cf);
}

fsgm_status fsgm_pyd_plan_ingest_float_dptr(fsgm_pyd_plan* p, int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t layout,
                                            int32_t cost_bound, void* stream, int32_t* status) {
    const char* who = "fsgm_pyd_plan_ingest_float_dptr";
    FSGM_REQUIRE(p && C, "%s: null argument", who);
    CostFormat cf;
    fsgm_status st = check_cost_format(who, fmt, &cf);
    if (st != FSGM_OK || (st = pyd_ingest_args(who, p, n, layout, cost_bound)) != FSGM_OK) return st;
    const hipStream_t cs = (hipStream_t)stream;
    const size_t es = cost_elem_size(cf.dtype);
    if ((st = device_check_args(who, p->device, cs, {{C, (size_t)n * p->NP * p->D * es, es, true, "C"}, {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    if ((st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    p->cmax = cost_bound;
    return device_call(p->join, cs, p->stream, [&] {
        launch_sgm2d_ingest_float(p->stream, C, cf, p->dC, n, p->W, p->H, p->Sx, p->Sy, layout, cost_bound, p->dIngestFlag);
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

fsgm_status fsgm_pyd_plan_ingest_cost_device(fsgm_pyd_plan* p, int32_t n, const uint8_t* C, int32_t layout, int32_t cost_bound,
                                             void* stream, int32_t* status) {
    const char* who = "fsgm_pyd_plan_ingest_cost_device";
    FSGM_REQUIRE(p && C, "%s: null argument", who);
    fsgm_status st = pyd_ingest_args(who, p, n, layout, cost_bound);
    if (st != FSGM_OK) return st;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, p->device, cs, {{C, (size_t)n * p->NP * p->D, 1, true, "C"}, {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    if ((st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    p->cmax = cost_bound;
    return device_call(p->join, cs, p->stream, [&] {
        launch_sgm2d_ingest(p->stream, C, p->dC, n, p->W, p->H, p->Sx, p->Sy, layout, cost_bound, p->dIngestFlag);
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

}  // extern "C"
