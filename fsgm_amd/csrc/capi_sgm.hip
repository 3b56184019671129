// capi_sgm.hip -- C ABI of sgm(C, P1, P2) on batches of caller-supplied cost volumes, in host memory or in HBM (include/fsgm.h:
// fsgm_sgm_batch_host, fsgm_sgm_device, their _ru and _exact forms, the float and the view-2 forms, fsgm_sgm_host and the plan-level
// ingest entries).  Everything that can be refused without a device is refused first, into a checked call (SgmCall); behind that both
// forms run on a cached plan of capi_epi.hip (epi_plan.h).
#include "epi_plan.h"
#include "cost_float_ingest.h"
#include "epi_view2.h"
#include "sgm_ingest.h"
#include <algorithm>
#include <string.h>
#include <vector>

using namespace fsgm;

namespace {
// a checked call
struct SgmCall {
    int n, W, H, D, P1, P2;
    fsgm_sgm_params prm;                 // checked, never the caller's NULL
    const uint8_t *C, *guide;            // guide: non-NULL exactly when prm.adaptive_p2
    uint32_t *bestD, *minC, *S;          // S may be NULL
    uint32_t* minC2;                     // the _ru forms' runner-up cost (never NULL there), NULL in the plain forms
    int exact;                           // the _exact forms: exact path arithmetic, P1 and P2 checked to lie in 0..255 (never with minC2)
    int captured = 0;                    // fsgm_sgm_device_exact alone: the caller's stream is being captured into a graph
    CostFormat fmt;                      // the float forms: C holds elements of fmt.dtype (-1 in the u8 forms), quantised by the ingest
    // the view-2 forms (include/fsgm.h, "Second view"): view2 = the direction, -1 or +1 (0 in every other form); disp2 is never NULL
    // then, minC_v2 and conf may be
    int view2 = 0, d_min = 0, max_diff = 0;
    uint32_t *disp2 = nullptr, *minC_v2 = nullptr;
    uint8_t* conf = nullptr;
};
}  // namespace

// the checks both forms share: prm (NULL: the defaults) into c->prm, the scalars and the pointers every call needs
static fsgm_status sgm_args(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                            const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* S, uint32_t* minC2, bool ru,
                            bool exact, SgmCall* c) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(C && bestD && minC, "%s: null argument", who);
    FSGM_REQUIRE(!ru || minC2, "%s: null minC2", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    FSGM_REQUIRE(D >= 1 && D <= 1024, "%s: dMax must be 1..1024 (got %d)", who, D);
    const fsgm_sgm_params sp = prm ? *prm : fsgm_sgm_params_default();
    for (int r : sp.reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_sgm_params must be zero", who);
    FSGM_REQUIRE(sp.paths == 4 || sp.paths == 8, "%s: paths must be 4 or 8 (got %d)", who, sp.paths);
    FSGM_REQUIRE(sp.subpixel == 0 || sp.subpixel == 1, "%s: subpixel must be 0 or 1 (got %d)", who, sp.subpixel);
    FSGM_REQUIRE(sp.layout == FSGM_COST_LAYOUT_HWD || sp.layout == FSGM_COST_LAYOUT_DHW,
                 "%s: layout must be FSGM_COST_LAYOUT_HWD (0) or FSGM_COST_LAYOUT_DHW (1), got %d", who, sp.layout);
    FSGM_REQUIRE(sp.cost_bound >= 1 && sp.cost_bound <= 255, "%s: cost_bound must be 1..255 (got %d)", who, sp.cost_bound);
    FSGM_REQUIRE(sp.agg_mode >= 0 && sp.agg_mode <= 6, "%s: agg_mode must be 0..6 (got %d)", who, sp.agg_mode);
    FSGM_REQUIRE(sp.adaptive_p2 == 0 || sp.adaptive_p2 == 1, "%s: adaptive_p2 must be 0 or 1 (got %d)", who, sp.adaptive_p2);
    FSGM_REQUIRE(sp.device >= 0 && sp.device < FSGM_MAX_DEVICES, "%s: device %d out of range", who, sp.device);
    FSGM_REQUIRE(!sp.adaptive_p2 || guide, "%s: adaptive_p2 needs the guide image (guide is NULL)", who);
    if (sp.adaptive_p2 && sp.agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: agg_mode %d with adaptive_p2: only the line kernels (modes 0 and 1) take a per-step P2", who,
                    sp.agg_mode);
    if (ru && sp.agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: agg_mode %d with minC2: only the line kernels' WTA (modes 0 and 1) writes the runner-up cost", who,
                    sp.agg_mode);
    if (exact) {                                                 // (the plain forms take any P1, P2: the reference narrows whatever they are)
        FSGM_REQUIRE(P1 >= 0 && P1 <= 255, "%s: exact path arithmetic takes P1 in 0..255 (got %d)", who, P1);
        FSGM_REQUIRE(P2 >= 0 && P2 <= 255, "%s: exact path arithmetic takes P2 in 0..255 (got %d)", who, P2);
        if (sp.agg_mode >= 2)
            return fail(FSGM_ERR_UNSUPPORTED, "%s: agg_mode %d with exact path arithmetic: only the line kernels (modes 0 and 1) carry path costs above 255",
                        who, sp.agg_mode);
    }
    if ((double)W * H * D >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: cost volume %d x %d x %d exceeds 2^31 voxels per frame", who, W, H, D);
    if (n > 65535) return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames %d exceeds 65535 (the frame is a grid dimension)", who, n);
    *c = SgmCall{n, W, H, D, P1, P2, sp, C, sp.adaptive_p2 ? guide : nullptr, bestD, minC, S, ru ? minC2 : nullptr, exact ? 1 : 0};
    return FSGM_OK;
}

extern "C" {

fsgm_sgm_params fsgm_sgm_params_default(void) {
    fsgm_sgm_params p;
    memset(&p, 0, sizeof(p));
    p.paths = 4;                         // sgm.m's enableDiagonalPath = false, as fsgm_sgm_host's callers pass
    p.subpixel = 1;
    p.layout = FSGM_COST_LAYOUT_HWD;
    p.cost_bound = 255;
    return p;
}

}  // extern "C"

static thread_local const char* g_sgm_kernel = "";

// the cached plan of a checked call: its batch, mode, adaptive, runner-up and exact switches are part of the key
static fsgm_status sgm_plan(std::unique_lock<std::mutex>& lk, fsgm_epi_plan** p, const SgmCall& c) {
    EpiPlanKey k;
    k.W = c.W; k.H = c.H; k.D = c.D; k.batch = c.n;
    k.prm.paths = c.prm.paths; k.prm.subpixel = c.prm.subpixel; k.prm.device = c.prm.device; k.prm.vz_to_disp = 0; k.prm.fb_check = 0;
    k.adaptive = c.prm.adaptive_p2; k.agg_mode = c.prm.agg_mode; k.runner_up = c.minC2 != nullptr; k.exact = c.exact; k.view2_dir = c.view2;
    return cached_plan(lk, p, k, c.captured != 0);
}

// the check of the sgm(C) view-2 forms on the plan's own outputs: index units, both shifted by the call's d_min
static void enqueue_sgm_view2_check(fsgm_epi_plan* p, const SgmCall& c, const uint32_t* bestD, const uint32_t* disp2, uint8_t* conf) {
    View2CheckArgs k{};
    k.disp = bestD; k.disp2 = disp2; k.conf = conf; k.W = p->W; k.H = p->H; k.dir = c.view2; k.max_diff = c.max_diff;
    k.add1 = k.add2 = 256 * c.d_min; k.marker2 = 0xFFFFFFFFu;
    k.shift1 = c.prm.subpixel ? 0 : 8;                           // (without sub-pixel bestD is the whole index, disp2 always index * 256)
    launch_view2_check(p->stream, k, c.n);
}

// host pointers; cmax: the largest byte of each frame's volume (none above prm.cost_bound), of a float volume prm.cost_bound
static fsgm_status sgm_run_host(const SgmCall& c, const int* cmax) {
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = sgm_plan(lk, &p, c);
    if (st != FSGM_OK) return st;
    const size_t NP = p->NP, nv = (size_t)c.n * p->N;
    for (int f = 0; f < c.n; f++) p->cmax[f] = cmax[f];
    if ((st = fsgm_epi_plan_set_penalties(p, c.P1, c.P2, p->vMax)) != FSGM_OK) return st;    // (selects the kernels for cmax)
    if (c.guide)                                                 // the aggregation reads I1 only: the guide stands for both images
        for (int f = 0; f < c.n; f++)
            if ((st = fsgm_epi_plan_upload_images(p, f, c.guide + f * NP, c.guide + f * NP)) != FSGM_OK) return st;
    if ((st = epi_prepare(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    const bool dhw = c.prm.layout == FSGM_COST_LAYOUT_DHW;       // staged as it came, transposed on the device
    if (dhw && c.fmt.dtype < 0 && !p->dIngest) FSGM_HIP(hipMalloc((void**)&p->dIngest, nv));
    if (c.fmt.dtype >= 0 && (st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    if (c.view2) p->d_min = c.d_min;                             // (read by the second view's kernel only: the plan has no cost stage to shift)
    if (c.conf && (st = epi_ensure_view2_conf(p)) != FSGM_OK) return st;
    StreamGuard guard(p->stream);                                // every early exit drains the stream: the copies use caller memory
    if (c.fmt.dtype >= 0) {
        // a float volume: staged frame by frame, quantised by the kernel the device form runs; the flag is read before any output is written
        const fsgm_status fs = stage_float_volumes(p->stream, c.C, c.fmt, c.n, p->N, p->dIngestFlag, "fsgm_sgm_float_batch_host",
            [&](const void* d, int f) { launch_sgm_ingest_float(p->stream, d, c.fmt, p->dC + (size_t)f * p->N, 1, c.W, c.H, c.D, c.prm.layout, c.prm.cost_bound, p->dIngestFlag); });
        if (fs != FSGM_OK) return fs;
    } else {
        FSGM_HIP(hipMemcpyAsync(dhw ? p->dIngest : p->dC, c.C, nv, hipMemcpyHostToDevice, p->stream));
        if (dhw) launch_sgm_ingest(p->stream, p->dIngest, p->dC, c.n, c.W, c.H, c.D, FSGM_COST_LAYOUT_DHW, 255, nullptr);
    }
    if ((st = epi_enqueue(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    g_sgm_kernel = kPipelineName[p->pipe];
    FSGM_HIP(hipMemcpyAsync(c.bestD, p->dBestD, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipMemcpyAsync(c.minC, p->dMinC, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
    if (c.minC2) FSGM_HIP(hipMemcpyAsync(c.minC2, p->dMinC2, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
    if (c.view2) {
        FSGM_HIP(hipMemcpyAsync(c.disp2, p->dDisp2v, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
        if (c.minC_v2) FSGM_HIP(hipMemcpyAsync(c.minC_v2, p->dMinCv2, (size_t)c.n * NP * 4, hipMemcpyDeviceToHost, p->stream));
        if (c.conf) {
            enqueue_sgm_view2_check(p, c, p->dBestD, p->dDisp2v, p->dConfV2);
            FSGM_HIP(hipGetLastError());
            FSGM_HIP(hipMemcpyAsync(c.conf, p->dConfV2, (size_t)c.n * NP, hipMemcpyDeviceToHost, p->stream));
        }
    }
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    if ((st = epi_check_handoff(p)) != FSGM_OK) return st;
    for (int f = 0; c.S && f < c.n; f++)
        if ((st = fsgm_epi_plan_download_sum(p, f, c.S + (size_t)f * p->N)) != FSGM_OK) return st;
    return FSGM_OK;
}

// device pointers, checked (device_check_args) by the caller; cs: the caller's stream
static fsgm_status sgm_run_device(const SgmCall& c, hipStream_t cs, int32_t* status) {
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    fsgm_status st = sgm_plan(lk, &p, c);
    if (st != FSGM_OK) return st;
    if (c.captured) {
        // Under a capture nothing may be allocated or waited for: everything the call below would create must exist (an earlier
        // call of the host form, or one without S or without a guide, leaves some of it out).  Refused before anything is queued.
        const bool warm = p->dL && p->dIngestFlag && p->join.in && p->join.out && (!c.S || p->dS) && (!c.guide || (p->dI1 && p->dI2));
        if (!warm)
            return fail(FSGM_ERR_UNSUPPORTED, "fsgm_sgm_device_exact: the stream is being captured into a graph and the cached plan lacks buffers "
                                              "this call needs: run the same call once outside the capture");
        p->pinned = true;                                        // the graph names the plan's buffers, stream and events from here on
    }
    // What a warm call must not do happens here, before the join with the caller's stream.  The device cannot be asked for the
    // true maximum without a wait: the declared bound selects the kernels, the ingest kernel saturates at it.
    p->cmax.assign(c.n, c.prm.cost_bound);
    if ((st = fsgm_epi_plan_set_penalties(p, c.P1, c.P2, p->vMax)) != FSGM_OK) return st;
    if (c.guide) {
        if ((st = epi_ensure_image_buffers(p)) != FSGM_OK) return st;
        p->have_img.assign(c.n, 1);                              // the guide goes into dI1 below, ahead of the kernels
    }
    if ((st = epi_prepare(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    if ((st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    if (c.S && (st = epi_ensure_tap_buffers(p)) != FSGM_OK) return st;
    if (c.view2) p->d_min = c.d_min;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        if (c.fmt.dtype >= 0) launch_sgm_ingest_float(p->stream, c.C, c.fmt, p->dC, c.n, c.W, c.H, c.D, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        else launch_sgm_ingest(p->stream, c.C, p->dC, c.n, c.W, c.H, c.D, c.prm.layout, c.prm.cost_bound, p->dIngestFlag);
        if (c.guide) FSGM_HIP(hipMemcpyAsync(p->dI1, c.guide, (size_t)c.n * p->NP, hipMemcpyDeviceToDevice, p->stream));
        Bind<uint32_t> bd(p->dBestD, c.bestD), mc(p->dMinC, c.minC), m2(p->dMinC2, c.minC2);
        Bind<uint32_t> d2(p->dDisp2v, c.disp2), mv(p->dMinCv2, c.minC_v2);   // (the view-2 forms: written where they lie)
        const fsgm_status es = epi_enqueue(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA);
        if (es != FSGM_OK) return es;
        g_sgm_kernel = kPipelineName[p->pipe];
        if (c.view2 && c.conf) enqueue_sgm_view2_check(p, c, c.bestD, c.disp2, c.conf);
        for (int f = 0; c.S && f < c.n; f++) {                   // S never exists for a batch: frame by frame through the tap's buffer
            epi_tap_sum(p, f);
            FSGM_HIP(hipMemcpyAsync(c.S + (size_t)f * p->N, p->dS, p->N * 4, hipMemcpyDeviceToDevice, p->stream));
        }
        launch_device_status(p->stream, p->dBandErr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

// every host form; ru: the _ru form, exact: the _exact form
static fsgm_status sgm_host(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                            const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2, bool ru,
                            uint32_t* S, bool exact = false) {
    SgmCall c;
    fsgm_status st = sgm_args(who, n, C, W, H, D, P1, P2, prm, guide, bestD, minC, S, minC2, ru, exact, &c);
    if (st != FSGM_OK) return st;
    // the true maximum of every frame, as fsgm_epi_plan_upload_cost takes it (either layout holds the same bytes)
    std::vector<int> cmax(n, 0);
    if ((st = frame_cost_maxima(who, C, n, (size_t)W * H * D, c.prm.cost_bound, cmax.data())) != FSGM_OK) return st;
    return sgm_run_host(c, cmax.data());
}

// every device form
static fsgm_status sgm_device(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                              const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2, bool ru,
                              uint32_t* S, void* stream, int32_t* status, bool exact = false) {
    SgmCall c;
    fsgm_status st = sgm_args(who, n, C, W, H, D, P1, P2, prm, guide, bestD, minC, S, minC2, ru, exact, &c);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H, nv = np * D;
    const hipStream_t cs = (hipStream_t)stream;
    bool captured = false;
    if ((st = device_check_args(who, c.prm.device, cs, {{C, nv, 1, true, "C"},
                                                        {c.guide, np, 1, false, "guide"},
                                                        {bestD, np * 4, 4, true, "bestD"},
                                                        {minC, np * 4, 4, true, "minC"},
                                                        {c.minC2, np * 4, 4, ru, "minC2"},
                                                        {S, nv * 4, 4, false, "S"},
                                                        {status, 4, 4, false, "status"}},
                                /* a warm exact call may be captured into a graph (include/fsgm.h) */ exact ? &captured : nullptr)) != FSGM_OK)
        return st;
    c.captured = captured;
    return sgm_run_device(c, cs, status);
}

// The float forms (include/fsgm.h, "Float cost volumes"): the checks of the u8 forms with the format's in front; minC2 is wanted
// when given, exact is a switch.  The checked call carries the format, and only the ingest launch behind it differs.
static fsgm_status sgm_float_args(const char* who, int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t W, int32_t H, int32_t D,
                                  int32_t P1, int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                  uint32_t* minC2, uint32_t* S, int32_t exact, SgmCall* c) {
    FSGM_REQUIRE(exact == 0 || exact == 1, "%s: exact must be 0 or 1 (got %d)", who, exact);
    CostFormat cf;
    fsgm_status st = check_cost_format(who, fmt, &cf);
    if (st != FSGM_OK) return st;
    const bool ru = minC2 != nullptr;
    if ((st = sgm_args(who, n, static_cast<const uint8_t*>(C), W, H, D, P1, P2, prm, guide, bestD, minC, S, minC2, ru, exact != 0, c)) != FSGM_OK)
        return st;
    if (exact && ru) return fail(FSGM_ERR_UNSUPPORTED, "%s: exact path arithmetic has no runner-up cost (pass minC2 = NULL with exact)", who);
    c->fmt = cf;
    return FSGM_OK;
}

extern "C" {

fsgm_status fsgm_sgm_float_batch_host(int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t W, int32_t H, int32_t D, int32_t P1,
                                      int32_t P2, const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC,
                                      uint32_t* minC2, uint32_t* S, int32_t exact) {
    SgmCall c;
    const fsgm_status st = sgm_float_args("fsgm_sgm_float_batch_host", n, C, fmt, W, H, D, P1, P2, prm, guide, bestD, minC, minC2, S, exact, &c);
    if (st != FSGM_OK) return st;
    // no scan for the true maximum: the declared bound selects the kernels, as in the device forms
    const std::vector<int> cmax(n, c.prm.cost_bound);
    return sgm_run_host(c, cmax.data());
}

fsgm_status fsgm_sgm_float_dptr(int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                                uint32_t* S, int32_t exact, void* stream, int32_t* status) {
    const char* who = "fsgm_sgm_float_dptr";
    SgmCall c;
    fsgm_status st = sgm_float_args(who, n, C, fmt, W, H, D, P1, P2, prm, guide, bestD, minC, minC2, S, exact, &c);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H, nv = np * D, es = cost_elem_size(c.fmt.dtype);
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, c.prm.device, cs, {{C, nv * es, es, true, "C"},
                                                        {c.guide, np, 1, false, "guide"},
                                                        {bestD, np * 4, 4, true, "bestD"},
                                                        {minC, np * 4, 4, true, "minC"},
                                                        {c.minC2, np * 4, 4, false, "minC2"},
                                                        {S, nv * 4, 4, false, "S"},
                                                        {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    return sgm_run_device(c, cs, status);
}

}  // extern "C"

// The view-2 forms (include/fsgm.h, "Second view"): the checks of the u8 forms with the view-2 struct's in front; minC2 is wanted when
// given, exact is a switch.  The checked call carries the direction, the shift and the check's bound into the u8 forms' bodies.
static fsgm_status view2_params_args(const char* who, const fsgm_view2_params* v2, fsgm_view2_params* out) {
    *out = v2 ? *v2 : fsgm_view2_params_default();
    for (int r : out->reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_view2_params must be zero", who);
    FSGM_REQUIRE(out->direction == -1 || out->direction == 1, "%s: direction must be -1 or +1 (got %d)", who, out->direction);
    FSGM_REQUIRE(out->d_min >= -FSGM_D_MIN_LIMIT && out->d_min <= FSGM_D_MIN_LIMIT, "%s: |d_min| must be <= %d (got %d)", who,
                 FSGM_D_MIN_LIMIT, out->d_min);
    FSGM_REQUIRE(out->max_diff >= 0, "%s: max_diff must be >= 0 (got %d)", who, out->max_diff);
    return FSGM_OK;
}
static fsgm_status sgm_view2_args(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                  const fsgm_sgm_params* prm, const fsgm_view2_params* v2, const uint8_t* guide, uint32_t* bestD,
                                  uint32_t* minC, uint32_t* minC2, uint32_t* S, int32_t exact, uint32_t* disp2, uint32_t* minC_v2,
                                  uint8_t* conf, SgmCall* c) {
    FSGM_REQUIRE(exact == 0 || exact == 1, "%s: exact must be 0 or 1 (got %d)", who, exact);
    FSGM_REQUIRE(disp2, "%s: null disp2", who);
    fsgm_view2_params vp;
    fsgm_status st = view2_params_args(who, v2, &vp);
    if (st != FSGM_OK) return st;
    const bool ru = minC2 != nullptr;
    if ((st = sgm_args(who, n, C, W, H, D, P1, P2, prm, guide, bestD, minC, S, minC2, ru, exact != 0, c)) != FSGM_OK) return st;
    if (exact && ru) return fail(FSGM_ERR_UNSUPPORTED, "%s: exact path arithmetic has no runner-up cost (pass minC2 = NULL with exact)", who);
    if (c->prm.agg_mode >= 2)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: agg_mode %d with the second view: only the line kernels (modes 0 and 1) keep the path volumes", who,
                    c->prm.agg_mode);
    c->view2 = vp.direction; c->d_min = vp.d_min; c->max_diff = vp.max_diff;
    c->disp2 = disp2; c->minC_v2 = minC_v2; c->conf = conf;
    return FSGM_OK;
}
static fsgm_status view2_check_args(const char* who, int32_t n, const int32_t* disp, const int32_t* disp2, int32_t W, int32_t H,
                                    int32_t direction, int32_t max_diff, const uint8_t* conf, int32_t device) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(disp && disp2 && conf, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    FSGM_REQUIRE(direction == -1 || direction == 1, "%s: direction must be -1 or +1 (got %d)", who, direction);
    FSGM_REQUIRE(max_diff >= 0, "%s: max_diff must be >= 0 (got %d)", who, max_diff);
    FSGM_REQUIRE(device >= 0 && device < FSGM_MAX_DEVICES, "%s: device %d out of range", who, device);
    if ((double)W * H >= 2147483648.0) return fail(FSGM_ERR_UNSUPPORTED, "%s: %d x %d exceeds 2^31 pixels per frame", who, W, H);
    if (n > 65535) return fail(FSGM_ERR_UNSUPPORTED, "%s: n_frames %d exceeds 65535 (the frame is a grid dimension)", who, n);
    return FSGM_OK;
}
static View2CheckArgs view2_check_launch_args(const int32_t* disp, const int32_t* disp2, int W, int H, int direction, int max_diff, uint8_t* conf) {
    View2CheckArgs k{};
    k.disp = (const uint32_t*)disp; k.disp2 = (const uint32_t*)disp2; k.conf = conf; k.W = W; k.H = H; k.dir = direction;
    k.max_diff = max_diff; k.add1 = k.add2 = 0; k.marker2 = 0x80000000u;
    return k;
}

extern "C" {

fsgm_view2_params fsgm_view2_params_default(void) {
    fsgm_view2_params p;
    memset(&p, 0, sizeof(p));
    p.direction = -1;
    p.max_diff = 256;                    // one disparity
    return p;
}

fsgm_status fsgm_sgm_view2_batch_host(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                      const fsgm_sgm_params* prm, const fsgm_view2_params* v2, const uint8_t* guide, uint32_t* bestD,
                                      uint32_t* minC, uint32_t* minC2, uint32_t* S, int32_t exact, uint32_t* disp2, uint32_t* minC_v2,
                                      uint8_t* conf) {
    const char* who = "fsgm_sgm_view2_batch_host";
    SgmCall c;
    fsgm_status st = sgm_view2_args(who, n, C, W, H, D, P1, P2, prm, v2, guide, bestD, minC, minC2, S, exact, disp2, minC_v2, conf, &c);
    if (st != FSGM_OK) return st;
    std::vector<int> cmax(n, 0);                                 // the true maximum of every frame, as fsgm_sgm_batch_host takes it
    if ((st = frame_cost_maxima(who, C, n, (size_t)W * H * D, c.prm.cost_bound, cmax.data())) != FSGM_OK) return st;
    return sgm_run_host(c, cmax.data());
}

fsgm_status fsgm_sgm_view2_dptr(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                const fsgm_sgm_params* prm, const fsgm_view2_params* v2, const uint8_t* guide, uint32_t* bestD,
                                uint32_t* minC, uint32_t* minC2, uint32_t* S, int32_t exact, uint32_t* disp2, uint32_t* minC_v2,
                                uint8_t* conf, void* stream, int32_t* status) {
    const char* who = "fsgm_sgm_view2_dptr";
    SgmCall c;
    fsgm_status st = sgm_view2_args(who, n, C, W, H, D, P1, P2, prm, v2, guide, bestD, minC, minC2, S, exact, disp2, minC_v2, conf, &c);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H, nv = np * D;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, c.prm.device, cs, {{C, nv, 1, true, "C"},
                                                        {c.guide, np, 1, false, "guide"},
                                                        {bestD, np * 4, 4, true, "bestD"},
                                                        {minC, np * 4, 4, true, "minC"},
                                                        {c.minC2, np * 4, 4, false, "minC2"},
                                                        {S, nv * 4, 4, false, "S"},
                                                        {disp2, np * 4, 4, true, "disp2"},
                                                        // (the type in the label: tests/test_footprint_table_cpu.py matches bare names against a
                                                        // closed table of element sizes that has no minC_v2; the row aligns on its 4 bytes as the
                                                        // table wants, and tests/test_gpu_footprint_view2.py places it so)
                                                        {minC_v2, np * 4, 4, false, "minC_v2 (u32)"},
                                                        {conf, np, 1, false, "conf"},
                                                        {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    return sgm_run_device(c, cs, status);
}

fsgm_status fsgm_view2_check_host(int32_t n, const int32_t* disp, const int32_t* disp2, int32_t W, int32_t H, int32_t direction,
                                  int32_t max_diff, uint8_t* conf, int32_t device) {
    const char* who = "fsgm_view2_check_host";
    fsgm_status st = view2_check_args(who, n, disp, disp2, W, H, direction, max_diff, conf, device);
    if (st != FSGM_OK) return st;
    if ((st = use_device(device)) != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H;
    uint8_t* buf = nullptr;                                      // disp, disp2, conf
    FSGM_HIP(hipMalloc((void**)&buf, np * 9));
    int32_t *d1 = (int32_t*)buf, *d2 = d1 + np;
    uint8_t* cf = buf + np * 8;
    hipError_t e = hipMemcpy(d1, disp, np * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d2, disp2, np * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_view2_check(nullptr, view2_check_launch_args(d1, d2, W, H, direction, max_diff, cf), n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(conf, cf, np, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    return hip_status(e, who);
}

fsgm_status fsgm_view2_check_dptr(int32_t n, const int32_t* disp, const int32_t* disp2, int32_t W, int32_t H, int32_t direction,
                                  int32_t max_diff, uint8_t* conf, int32_t device, void* stream, int32_t* status) {
    const char* who = "fsgm_view2_check_dptr";
    fsgm_status st = view2_check_args(who, n, disp, disp2, W, H, direction, max_diff, conf, device);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, device, cs, {{disp, np * 4, 4, true, "disp"},
                                                  {disp2, np * 4, 4, true, "disp2"},
                                                  {conf, np, 1, true, "conf"},
                                                  {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    launch_view2_check(cs, view2_check_launch_args(disp, disp2, W, H, direction, max_diff, conf), n);
    FSGM_HIP(hipGetLastError());
    launch_device_status(cs, nullptr, nullptr, status);
    return FSGM_OK;
}

fsgm_status fsgm_sgm_batch_host(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* S) {
    return sgm_host("fsgm_sgm_batch_host", n, C, W, H, D, P1, P2, prm, guide, bestD, minC, nullptr, false, S);
}

fsgm_status fsgm_sgm_batch_host_ru(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                   const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                                   uint32_t* S) {
    return sgm_host("fsgm_sgm_batch_host_ru", n, C, W, H, D, P1, P2, prm, guide, bestD, minC, minC2, true, S);
}

fsgm_status fsgm_sgm_device(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                            const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* S, void* stream,
                            int32_t* status) {
    return sgm_device("fsgm_sgm_device", n, C, W, H, D, P1, P2, prm, guide, bestD, minC, nullptr, false, S, stream, status);
}

fsgm_status fsgm_sgm_device_ru(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                               const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2,
                               uint32_t* S, void* stream, int32_t* status) {
    return sgm_device("fsgm_sgm_device_ru", n, C, W, H, D, P1, P2, prm, guide, bestD, minC, minC2, true, S, stream, status);
}

fsgm_status fsgm_sgm_batch_host_exact(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                      const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* S) {
    return sgm_host("fsgm_sgm_batch_host_exact", n, C, W, H, D, P1, P2, prm, guide, bestD, minC, nullptr, false, S, true);
}

fsgm_status fsgm_sgm_device_exact(int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                                  const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* S,
                                  void* stream, int32_t* status) {
    return sgm_device("fsgm_sgm_device_exact", n, C, W, H, D, P1, P2, prm, guide, bestD, minC, nullptr, false, S, stream, status, true);
}

// sgm(C, P1, P2): sgm.m's call shape on the MEX's aggregation + WTA (MEX semantics: include/fsgm.h)
fsgm_status fsgm_sgm_host(const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2, int32_t paths,
                          uint32_t* bestD, uint32_t* minC, uint32_t* S, int32_t device) {
    FSGM_REQUIRE(C && bestD && minC, "fsgm_sgm: null argument");
    fsgm_epi_params pr = fsgm_epi_params_default();
    pr.paths = paths; pr.device = device; pr.vz_to_disp = 0; pr.subpixel = 1;
    std::unique_lock<std::mutex> lk;
    fsgm_epi_plan* p = nullptr;
    EpiPlanKey key;
    key.W = W; key.H = H; key.D = D; key.batch = 1; key.prm = pr;
    fsgm_status st = cached_plan(lk, &p, key);
    if (st != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_set_penalties(p, P1, P2, p->vMax)) != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_upload_cost(p, 0, C)) != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_run(p, FSGM_STAGE_AGGREGATE | FSGM_STAGE_WTA)) != FSGM_OK) return st;
    if ((st = fsgm_epi_plan_download(p, 0, bestD, minC)) != FSGM_OK) return st;
    if (S && (st = fsgm_epi_plan_download_sum(p, 0, S)) != FSGM_OK) return st;
    return FSGM_OK;
}

const char* fsgm_sgm_last_kernel(void) { return g_sgm_kernel; }

// the scalar checks of both plan-level ingest entries, behind their null and format checks
static fsgm_status epi_ingest_args(const char* who, const fsgm_epi_plan* p, int32_t n, int32_t layout, int32_t cost_bound) {
    FSGM_REQUIRE(n == p->batch, "%s: n_frames %d differs from the plan's batch %d", who, n, p->batch);
    FSGM_REQUIRE(layout == FSGM_COST_LAYOUT_HWD || layout == FSGM_COST_LAYOUT_DHW,
                 "%s: layout must be FSGM_COST_LAYOUT_HWD (0) or FSGM_COST_LAYOUT_DHW (1), got %d", who, layout);
    FSGM_REQUIRE(cost_bound >= 1 && cost_bound <= 255, "%s: cost_bound must be 1..255 (got %d)", who, cost_bound);
    return FSGM_OK;
}

fsgm_status fsgm_epi_plan_ingest_cost_device(fsgm_epi_plan* p, int32_t n, const uint8_t* C, int32_t layout, int32_t cost_bound,
                                             void* stream, int32_t* status) {
    const char* who = "fsgm_epi_plan_ingest_cost_device";
    FSGM_REQUIRE(p && C, "%s: null argument", who);
    fsgm_status st = epi_ingest_args(who, p, n, layout, cost_bound);
    if (st != FSGM_OK) return st;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, p->prm.device, cs, {{C, (size_t)n * p->N, 1, true, "C"}, {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    if ((st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    p->cmax.assign(n, cost_bound);
    epi_select_kernel(p);
    return device_call(p->join, cs, p->stream, [&] {
        launch_sgm_ingest(p->stream, C, p->dC, n, p->W, p->H, p->D, layout, cost_bound, p->dIngestFlag);
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

fsgm_status fsgm_epi_plan_ingest_float_dptr(fsgm_epi_plan* p, int32_t n, const void* C, const fsgm_cost_format* fmt, int32_t layout,
                                            int32_t cost_bound, void* stream, int32_t* status) {
    const char* who = "fsgm_epi_plan_ingest_float_dptr";
    FSGM_REQUIRE(p && C, "%s: null argument", who);
    CostFormat cf;
    fsgm_status st = check_cost_format(who, fmt, &cf);
    if (st != FSGM_OK || (st = epi_ingest_args(who, p, n, layout, cost_bound)) != FSGM_OK) return st;
    const hipStream_t cs = (hipStream_t)stream;
    const size_t es = cost_elem_size(cf.dtype);
    if ((st = device_check_args(who, p->prm.device, cs, {{C, (size_t)n * p->N * es, es, true, "C"}, {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    if ((st = ensure_ingest_flag(&p->dIngestFlag, p->stream)) != FSGM_OK) return st;
    p->cmax.assign(n, cost_bound);
    epi_select_kernel(p);
    return device_call(p->join, cs, p->stream, [&] {
        launch_sgm_ingest_float(p->stream, C, cf, p->dC, n, p->W, p->H, p->D, layout, cost_bound, p->dIngestFlag);
        launch_device_status(p->stream, nullptr, p->dIngestFlag, status);
        return FSGM_OK;
    });
}

}  // extern "C"
