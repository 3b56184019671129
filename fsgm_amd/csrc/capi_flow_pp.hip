// capi_flow_pp.hip -- C ABI of the filtered flow for the pyramidal matchers (include/fsgm.h, "Consistency-checked, filtered
// flow"): the chain of test.m:45-49 on two-channel flows (post_kernels.hip), its stages on their own, and the pipeline
// behind a batch-2n run of either pyramidal driver (flow_pp.h).
#include "capi_common.h"
#include "capi_device.h"
#include "flow_pp.h"
#include "post_kernels.h"
#include "stereo_pp_kernels.h"
#include <math.h>
#include <mutex>

using namespace fsgm;

// Scratch for n flows of W x H.  S holds 4n planes (the speckle-filtered forward and backward flows; later the checked and
// the filled flow), C 2n planes (the forward-backward result; later the median), parent / size 2n maps, left n maps.
// The stages' device forms run on `stream`, the pipeline on its pyramid plan's stream: `busy` is recorded behind the last
// user of the scratch and waited for by the next, whichever stream that is.
struct fsgm_flow_pp_plan {
    int W = 0, H = 0, n = 0, device = 0;
    size_t NP = 0;
    hipStream_t stream = nullptr;
    hipEvent_t busy = nullptr;
    DeviceJoin join;
    double *dS = nullptr, *dC = nullptr, *dPP = nullptr;         // dPP: flow_pp of the host form, 3n planes, on first use
    int32_t *dParent = nullptr, *dSize = nullptr, *dLeft = nullptr;
};

static void flow_plan_destroy(fsgm_flow_pp_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);       // queued device-form work of an evicted plan (fsgm_epi_plan_destroy)
    if (p->busy) (void)hipEventSynchronize(p->busy);             // the pipeline forms use the scratch on their pyramid plan's stream
    void* bufs[] = {p->dS, p->dC, p->dPP, p->dParent, p->dSize, p->dLeft};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (p->busy) (void)hipEventDestroy(p->busy);
    p->join.destroy();
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

static PlanCache<fsgm_flow_pp_plan> g_flow(4, flow_plan_destroy);   // cached plans per device, under that device's lock

extern "C" void fsgm_flow_pp_shutdown_internal(void) { g_flow.clear(); }

static fsgm_status flow_args(const char* who, int32_t n, int32_t W, int32_t H, bool ok_ptrs, int32_t device) {
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(ok_ptrs, "%s: null argument", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    if (2.0 * n * W * H >= 2147483648.0)
        return fail(FSGM_ERR_UNSUPPORTED, "%s: 2 * n_frames * width * height = %.0f reaches 2^31 (32-bit pixel indices)", who, 2.0 * n * W * H);
    FSGM_DEVICE_SLOT(device);
    return FSGM_OK;
}

// The cached plan of this shape for an entry point (flow_args has checked the device's slot): `lk` holds its device's lock
// for the length of the call, the device is current.
static fsgm_status flow_plan_get(std::unique_lock<std::mutex>& lk, fsgm_flow_pp_plan** out, int W, int H, int n, int device) {
    const fsgm_status st = use_device(device);
    if (st != FSGM_OK) return st;
    lk = std::unique_lock<std::mutex>(g_flow.mu(device));
    if ((*out = g_flow.find(device, [&](const fsgm_flow_pp_plan* q) { return q->W == W && q->H == H && q->n == n; }))) return FSGM_OK;
    fsgm_flow_pp_plan* p = new fsgm_flow_pp_plan;
    p->W = W; p->H = H; p->n = n; p->device = device; p->NP = (size_t)W * H;
    const size_t np = p->NP * n;
    hipError_t e = hipMalloc((void**)&p->dS, 4 * np * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dC, 2 * np * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dParent, 2 * np * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dSize, 2 * np * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&p->dLeft, np * 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->busy, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(p->busy, p->stream);
    if (e != hipSuccess) {
        flow_plan_destroy(p);
        return hip_status(e, "filtered-flow plan");
    }
    g_flow.insert(device, p);
    *out = p;
    return FSGM_OK;
}

// flow_pp of the host forms, 3n planes, on first use
static fsgm_status ensure_pp(fsgm_flow_pp_plan* p, const char* who) {
    return p->dPP ? FSGM_OK : hip_status(hipMalloc((void**)&p->dPP, 3 * p->NP * p->n * 8), who);
}

// ---- the stages on their own ----
enum FlowStage { STAGE_SPECKLE, STAGE_FB, STAGE_FILL };
struct StageArgs {
    const double *in, *b;            // b: fb_check only
    double* out;
    double p0, p1;                   // speckle: maxDiff, maxSpeckleSize; fb_check: thr
};

static void stage_enqueue(hipStream_t st, fsgm_flow_pp_plan* p, FlowStage stage, const StageArgs& a) {
    switch (stage) {
    case STAGE_SPECKLE: launch_flow_speckle_filter(st, a.in, a.out, p->dParent, p->dSize, p->W, p->H, a.p0, a.p1, p->n); break;
    case STAGE_FB: launch_flow_fb_check(st, a.in, a.b, a.out, p->W, p->H, a.p0, p->n); break;
    case STAGE_FILL: launch_flow_in_fill(st, a.in, a.out, p->dLeft, p->W, p->H, p->n); break;
    }
}

static fsgm_status stage_check(const char* who, FlowStage stage, const StageArgs& a) {
    if (stage == STAGE_FB) FSGM_REQUIRE(a.p0 >= 0.0, "%s: thr must be >= 0 (got %g)", who, a.p0);
    if (stage == STAGE_SPECKLE) FSGM_REQUIRE(!isnan(a.p0) && !isnan(a.p1), "%s: maxDiff / maxSpeckleSize must be numbers", who);
    return FSGM_OK;
}

static fsgm_status stage_host(const char* who, FlowStage stage, int32_t n, int32_t W, int32_t H, StageArgs a, int32_t device) {
    fsgm_status st = flow_args(who, n, W, H, a.in && a.out && (stage != STAGE_FB || a.b), device);
    if (st != FSGM_OK || (st = stage_check(who, stage, a)) != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_flow_pp_plan* p;
    if ((st = flow_plan_get(lk, &p, W, H, n, device)) != FSGM_OK) return st;
    const size_t bytes = 2 * p->NP * n * 8;
    double *dIn = p->dS, *dB = p->dS + 2 * p->NP * n;
    StreamGuard guard(p->stream);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipStreamWaitEvent(p->stream, p->busy, 0));
    FSGM_HIP(hipMemcpyAsync(dIn, a.in, bytes, hipMemcpyHostToDevice, p->stream));
    if (stage == STAGE_FB) FSGM_HIP(hipMemcpyAsync(dB, a.b, bytes, hipMemcpyHostToDevice, p->stream));
    double* host_out = a.out;
    a.in = dIn; a.b = dB; a.out = p->dC;
    stage_enqueue(p->stream, p, stage, a);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipMemcpyAsync(host_out, p->dC, bytes, hipMemcpyDeviceToHost, p->stream));
    FSGM_HIP(hipEventRecord(p->busy, p->stream));
    FSGM_HIP(hipStreamSynchronize(p->stream));
    guard.dismiss();
    return FSGM_OK;
}

static fsgm_status stage_device(const char* who, FlowStage stage, int32_t n, int32_t W, int32_t H, const StageArgs& a, int32_t device,
                                void* stream) {
    fsgm_status st = flow_args(who, n, W, H, a.in && a.out && (stage != STAGE_FB || a.b), device);
    if (st != FSGM_OK || (st = stage_check(who, stage, a)) != FSGM_OK) return st;
    hipStream_t cs = (hipStream_t)stream;
    const size_t bytes = 2 * (size_t)W * H * n * 8;
    if ((st = device_check_args(who, device, cs, {{a.in, bytes, 8, true, stage == STAGE_FB ? "f" : "flow"},
                                                  {a.b, bytes, 8, stage == STAGE_FB, "b"},
                                                  {a.out, bytes, 8, true, "the output flow"}})) != FSGM_OK)
        return st;
    if (stage == STAGE_FB) {                                     // no scratch: on the caller's stream itself
        launch_flow_fb_check(cs, a.in, a.b, a.out, W, H, a.p0, n);
        FSGM_HIP(hipGetLastError());
        return FSGM_OK;
    }
    std::unique_lock<std::mutex> lk;
    fsgm_flow_pp_plan* p;
    if ((st = flow_plan_get(lk, &p, W, H, n, device)) != FSGM_OK) return st;
    return device_call(p->join, cs, p->stream, [&]() -> fsgm_status {
        FSGM_HIP(hipStreamWaitEvent(p->stream, p->busy, 0));
        stage_enqueue(p->stream, p, stage, a);
        FSGM_HIP(hipEventRecord(p->busy, p->stream));
        return FSGM_OK;
    });
}

// ---- the pipeline ----
struct FlowOutputs {
    double *flow_pp, *flow_checked, *flow_fwd, *flow_bwd;
    uint32_t* minC;
};

static fsgm_status params_check(const char* who, const fsgm_flow_pp_params* prm) {
    FSGM_REQUIRE(prm, "%s: null parameters", who);
    FSGM_REQUIRE(prm->matcher == FSGM_MATCHER_PYD || prm->matcher == FSGM_MATCHER_NG, "%s: matcher must be FSGM_MATCHER_PYD or FSGM_MATCHER_NG (got %d)", who, prm->matcher);
    FSGM_REQUIRE(prm->fb_thr >= 0.0, "%s: fb_thr must be >= 0 (got %g)", who, prm->fb_thr);
    FSGM_REQUIRE(prm->island_fraction >= 0.0 && prm->island_fraction <= 1.0, "%s: island_fraction must be in [0, 1] (got %g)", who, prm->island_fraction);
    FSGM_REQUIRE(!isnan(prm->speckle_max_diff) && !isnan(prm->speckle_max_size), "%s: speckle_max_diff / speckle_max_size must be numbers", who);
    FSGM_REQUIRE(prm->median == 0 || prm->median == 1, "%s: median must be 0 or 1 (got %d)", who, prm->median);
    return FSGM_OK;
}

// the chain on the pair's stream: pair.flow (f then b) -> flow_pp and checked (the plan's when the caller wants none)
static void chain_enqueue(hipStream_t st, fsgm_flow_pp_plan* p, const fsgm_flow_pp_params& prm, const double* flows, double* flow_pp,
                          double* checked) {
    const int W = p->W, H = p->H, n = p->n;
    const size_t half = 2 * p->NP * n;
    double *sf = p->dS, *sb = p->dS + half;
    launch_flow_speckle_filter(st, flows, sf, p->dParent, p->dSize, W, H, prm.speckle_max_diff, prm.speckle_max_size, 2 * n);   // test.m:45, f and b
    launch_flow_fb_check(st, sf, sb, p->dC, W, H, prm.fb_thr, n);                                                             // :47
    double* c = checked ? checked : sf;
    launch_flow_speckle_filter(st, p->dC, c, p->dParent, p->dSize, W, H, INFINITY, (double)((long long)H * W) * prm.island_fraction, n);   // :48
    launch_flow_in_fill(st, c, sb, p->dLeft, W, H, n);                                                                        // :49
    const double* g = sb;
    if (prm.median) {
        launch_vmf(st, sb, p->dC, W, H, 2 * n);                                                                               // vmf.m
        g = p->dC;
    }
    launch_flow_pack(st, g, c, flow_pp, W, H, n);                                                                             // :53
}

// frames n..2n-1 of the plan's inputs are frames 0..n-1 with the images swapped (first-half sources: the plan's own or the caller's)
static fsgm_status swap_enqueue(const PyramidPair& pr, const uint8_t* I0, const uint8_t* I1, size_t bytes) {
    FSGM_HIP(hipMemcpyAsync(pr.in0 + bytes, I1, bytes, hipMemcpyDeviceToDevice, pr.stream));
    FSGM_HIP(hipMemcpyAsync(pr.in1 + bytes, I0, bytes, hipMemcpyDeviceToDevice, pr.stream));
    return FSGM_OK;
}

static fsgm_status with_pair(int n, int W, int H, int channels, const fsgm_flow_pp_params& prm, int ru, int lm, const PairBody& body) {
    if (prm.matcher == FSGM_MATCHER_NG) {
        fsgm_ng_pyramid_params q = prm.ng;
        q.device = prm.device;
        return ng_pyramid_with_pair(n, W, H, channels, &q, ru, lm, body);
    }
    fsgm_pyramid_params q = prm.pyd;
    q.device = prm.device;
    return pyd_pyramid_with_pair(n, W, H, channels, &q, ru, lm, body);
}

// The _u forms' extra arguments (on: the call is one of them).  The plan of 2n pairs runs with the runner-up switch on, and the
// uniqueness test of include/fsgm.h blanks the ambiguous pixels of the forward and of the backward flow, each by its own minC
// and minC2, ahead of the chain: one launch over the 2n flows, in place in the plan's level-1 flow -- behind the copies that hand
// out the raw flows, which every form queues anyway, so no flow is copied for the filter's sake.  The level loop writes every
// pixel of that buffer again on its next run.  Ratio 0 rejects nothing: no launch.
struct Uniqueness {
    bool on;
    int32_t ratio;
    uint32_t* minC2;
};

static fsgm_status uniqueness_check(const char* who, const Uniqueness& u) {
    if (!u.on) return FSGM_OK;
    FSGM_REQUIRE(u.ratio >= 0 && u.ratio <= 100, "%s: uniqueness_ratio must be in [0, 100] (got %d)", who, u.ratio);
    FSGM_REQUIRE(u.minC2, "%s: null argument (minC2 is required)", who);
    return FSGM_OK;
}

// The _lm forms: the _u forms' arguments with the level median of the 2n-pair plan (both directions run with it).  minC2 may be
// NULL exactly when the ratio is 0; the plan then runs without the runner-up switch
static fsgm_status level_median_args(const char* who, int32_t ratio, const uint32_t* minC2, int32_t lm) {
    FSGM_REQUIRE(ratio >= 0 && ratio <= 100, "%s: uniqueness_ratio must be in [0, 100] (got %d)", who, ratio);
    FSGM_REQUIRE(minC2 || ratio == 0, "%s: null argument (minC2 is required with a non-zero uniqueness_ratio)", who);
    return level_median_check(who, lm);
}

static void uniqueness_enqueue(hipStream_t st, const PyramidPair& pr, const Uniqueness& u, size_t np, size_t frame_px) {
    if (u.on && u.ratio > 0) launch_flow_uniqueness(st, pr.flow, pr.minC, pr.minC2, const_cast<double*>(pr.flow), 2 * np, frame_px, u.ratio);
}

static fsgm_status flow_pp_host(const char* who, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                const fsgm_flow_pp_params* prm, const Uniqueness& u, const FlowOutputs& o, int lm = 0) {
    fsgm_status st = params_check(who, prm);
    if (st != FSGM_OK || (st = uniqueness_check(who, u)) != FSGM_OK) return st;
    if ((st = flow_args(who, n, W, H, I0 && I1 && o.flow_pp, prm->device)) != FSGM_OK) return st;
    std::unique_lock<std::mutex> lk;
    fsgm_flow_pp_plan* p;
    if ((st = flow_plan_get(lk, &p, W, H, n, prm->device)) != FSGM_OK) return st;
    const size_t np = p->NP * n;
    if ((st = ensure_pp(p, who)) != FSGM_OK) return st;
    return with_pair(n, W, H, channels, *prm, u.on, lm, [&](const PyramidPair& pr) -> fsgm_status {
        hipStream_t s = pr.stream;
        const size_t img = np * channels;
        StreamGuard guard(s);   // an early exit drains the stream: queued copies use the caller's memory
        FSGM_HIP(hipMemcpyAsync(pr.in0, I0, img, hipMemcpyHostToDevice, s));
        FSGM_HIP(hipMemcpyAsync(pr.in1, I1, img, hipMemcpyHostToDevice, s));
        fsgm_status r = swap_enqueue(pr, pr.in0, pr.in1, img);
        if (r != FSGM_OK || (r = pr.run(pr.plan)) != FSGM_OK) return r;
        FSGM_HIP(hipStreamWaitEvent(s, p->busy, 0));
        if (u.on) {                                              // the raw flows leave ahead of the filter
            if (o.flow_fwd) FSGM_HIP(hipMemcpyAsync(o.flow_fwd, pr.flow, 2 * np * 8, hipMemcpyDeviceToHost, s));
            if (o.flow_bwd) FSGM_HIP(hipMemcpyAsync(o.flow_bwd, pr.flow + 2 * np, 2 * np * 8, hipMemcpyDeviceToHost, s));
            uniqueness_enqueue(s, pr, u, np, p->NP);
        }
        chain_enqueue(s, p, *prm, pr.flow, p->dPP, nullptr);
        FSGM_HIP(hipGetLastError());
        FSGM_HIP(hipMemcpyAsync(o.flow_pp, p->dPP, 3 * np * 8, hipMemcpyDeviceToHost, s));
        if (o.flow_checked) FSGM_HIP(hipMemcpyAsync(o.flow_checked, p->dS, 2 * np * 8, hipMemcpyDeviceToHost, s));
        if (!u.on) {
            if (o.flow_fwd) FSGM_HIP(hipMemcpyAsync(o.flow_fwd, pr.flow, 2 * np * 8, hipMemcpyDeviceToHost, s));
            if (o.flow_bwd) FSGM_HIP(hipMemcpyAsync(o.flow_bwd, pr.flow + 2 * np, 2 * np * 8, hipMemcpyDeviceToHost, s));
        }
        if (o.minC) FSGM_HIP(hipMemcpyAsync(o.minC, pr.minC, np * 4, hipMemcpyDeviceToHost, s));
        if (u.on) FSGM_HIP(hipMemcpyAsync(u.minC2, pr.minC2, np * 4, hipMemcpyDeviceToHost, s));
        FSGM_HIP(hipEventRecord(p->busy, s));
        FSGM_HIP(hipStreamSynchronize(s));
        guard.dismiss();
        return FSGM_OK;
    });
}

static fsgm_status flow_pp_device(const char* who, int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                  const fsgm_flow_pp_params* prm, const Uniqueness& u, const FlowOutputs& o, void* stream, int32_t* status,
                                  int lm = 0) {
    fsgm_status st = params_check(who, prm);
    if (st != FSGM_OK || (st = uniqueness_check(who, u)) != FSGM_OK) return st;
    if ((st = flow_args(who, n, W, H, I0 && I1 && o.flow_pp, prm->device)) != FSGM_OK) return st;
    FSGM_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 (gray) or 3 (RGB planes), got %d", who, channels);
    hipStream_t cs = (hipStream_t)stream;
    const size_t np = (size_t)W * H * n, img = np * channels;
    if ((st = device_check_args(who, prm->device, cs, {{I0, img, 1, true, "I0"},
                                                       {I1, img, 1, true, "I1"},
                                                       {o.flow_pp, 3 * np * 8, 8, true, "flow_pp"},
                                                       {o.flow_checked, 2 * np * 8, 8, false, "flow_checked"},
                                                       {o.flow_fwd, 2 * np * 8, 8, false, "flow_fwd"},
                                                       {o.flow_bwd, 2 * np * 8, 8, false, "flow_bwd"},
                                                       {o.minC, np * 4, 4, false, "minC"},
                                                       {u.on ? u.minC2 : nullptr, np * 4, 4, u.on, "minC2"},
                                                       {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::unique_lock<std::mutex> lk;
    fsgm_flow_pp_plan* p;
    if ((st = flow_plan_get(lk, &p, W, H, n, prm->device)) != FSGM_OK) return st;
    return with_pair(n, W, H, channels, *prm, u.on, lm, [&](const PyramidPair& pr) -> fsgm_status {
        hipStream_t s = pr.stream;
        return device_call(*pr.join, cs, s, [&]() -> fsgm_status {
            FSGM_HIP(hipMemcpyAsync(pr.in0, I0, img, hipMemcpyDeviceToDevice, s));
            FSGM_HIP(hipMemcpyAsync(pr.in1, I1, img, hipMemcpyDeviceToDevice, s));
            fsgm_status w = swap_enqueue(pr, I0, I1, img);
            if (w != FSGM_OK || (w = pr.run(pr.plan)) != FSGM_OK) return w;
            FSGM_HIP(hipStreamWaitEvent(s, p->busy, 0));
            if (u.on) {                                          // the raw flows leave ahead of the filter
                if (o.flow_fwd) FSGM_HIP(hipMemcpyAsync(o.flow_fwd, pr.flow, 2 * np * 8, hipMemcpyDeviceToDevice, s));
                if (o.flow_bwd) FSGM_HIP(hipMemcpyAsync(o.flow_bwd, pr.flow + 2 * np, 2 * np * 8, hipMemcpyDeviceToDevice, s));
                uniqueness_enqueue(s, pr, u, np, (size_t)W * H);
            }
            chain_enqueue(s, p, *prm, pr.flow, o.flow_pp, o.flow_checked);
            FSGM_HIP(hipGetLastError());
            if (!u.on) {
                if (o.flow_fwd) FSGM_HIP(hipMemcpyAsync(o.flow_fwd, pr.flow, 2 * np * 8, hipMemcpyDeviceToDevice, s));
                if (o.flow_bwd) FSGM_HIP(hipMemcpyAsync(o.flow_bwd, pr.flow + 2 * np, 2 * np * 8, hipMemcpyDeviceToDevice, s));
            }
            if (o.minC) FSGM_HIP(hipMemcpyAsync(o.minC, pr.minC, np * 4, hipMemcpyDeviceToDevice, s));
            if (u.on) FSGM_HIP(hipMemcpyAsync(u.minC2, pr.minC2, np * 4, hipMemcpyDeviceToDevice, s));
            FSGM_HIP(hipEventRecord(p->busy, s));
            launch_device_status(s, nullptr, nullptr, status);
            return FSGM_OK;
        });
    });
}

extern "C" {

fsgm_flow_pp_params fsgm_flow_pp_params_default(int32_t matcher) {
    fsgm_flow_pp_params p;
    p.matcher = matcher;
    p.pyd = fsgm_pyramid_params_default();
    p.ng = fsgm_ng_pyramid_params_default();
    p.speckle_max_diff = 2.0;          // test.m:45
    p.speckle_max_size = 100.0;
    p.fb_thr = 2.0;                    // forward_backward_check.m:6
    p.island_fraction = 0.1;           // test.m:48
    p.median = 0;
    p.device = 0;
    return p;
}

fsgm_status fsgm_flow_speckle_filter_host(int32_t n, const double* flow, int32_t W, int32_t H, double maxDiff, double maxSpeckleSize,
                                          double* out, int32_t device) {
    return stage_host("fsgm_flow_speckle_filter", STAGE_SPECKLE, n, W, H, StageArgs{flow, nullptr, out, maxDiff, maxSpeckleSize}, device);
}
fsgm_status fsgm_flow_speckle_filter_device(int32_t n, const double* flow, int32_t W, int32_t H, double maxDiff, double maxSpeckleSize,
                                            double* out, int32_t device, void* stream) {
    return stage_device("fsgm_flow_speckle_filter_device", STAGE_SPECKLE, n, W, H, StageArgs{flow, nullptr, out, maxDiff, maxSpeckleSize}, device, stream);
}
fsgm_status fsgm_flow_fb_check_host(int32_t n, const double* f, const double* b, int32_t W, int32_t H, double thr, double* out, int32_t device) {
    return stage_host("fsgm_flow_fb_check", STAGE_FB, n, W, H, StageArgs{f, b, out, thr, 0.0}, device);
}
fsgm_status fsgm_flow_fb_check_device(int32_t n, const double* f, const double* b, int32_t W, int32_t H, double thr, double* out,
                                      int32_t device, void* stream) {
    return stage_device("fsgm_flow_fb_check_device", STAGE_FB, n, W, H, StageArgs{f, b, out, thr, 0.0}, device, stream);
}
fsgm_status fsgm_flow_in_fill_host(int32_t n, const double* flow, int32_t W, int32_t H, double* out, int32_t device) {
    return stage_host("fsgm_flow_in_fill", STAGE_FILL, n, W, H, StageArgs{flow, nullptr, out, 0.0, 0.0}, device);
}
fsgm_status fsgm_flow_in_fill_device(int32_t n, const double* flow, int32_t W, int32_t H, double* out, int32_t device, void* stream) {
    return stage_device("fsgm_flow_in_fill_device", STAGE_FILL, n, W, H, StageArgs{flow, nullptr, out, 0.0, 0.0}, device, stream);
}

fsgm_status fsgm_pyramidal_flow_pp_host(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                        const fsgm_flow_pp_params* prm, double* flow_pp, double* flow_checked, double* flow_fwd,
                                        double* flow_bwd, uint32_t* minC) {
    return flow_pp_host("fsgm_pyramidal_flow_pp", n, I0, I1, W, H, channels, prm, Uniqueness{false, 0, nullptr},
                        FlowOutputs{flow_pp, flow_checked, flow_fwd, flow_bwd, minC});
}

fsgm_status fsgm_pyramidal_flow_pp_device(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                          const fsgm_flow_pp_params* prm, double* flow_pp, double* flow_checked, double* flow_fwd,
                                          double* flow_bwd, uint32_t* minC, void* stream, int32_t* status) {
    return flow_pp_device("fsgm_pyramidal_flow_pp_device", n, I0, I1, W, H, channels, prm, Uniqueness{false, 0, nullptr},
                          FlowOutputs{flow_pp, flow_checked, flow_fwd, flow_bwd, minC}, stream, status);
}

fsgm_status fsgm_pyramidal_flow_pp_host_u(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                          const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio, double* flow_pp, double* flow_checked,
                                          double* flow_fwd, double* flow_bwd, uint32_t* minC, uint32_t* minC2) {
    return flow_pp_host("fsgm_pyramidal_flow_pp_host_u", n, I0, I1, W, H, channels, prm, Uniqueness{true, uniqueness_ratio, minC2},
                        FlowOutputs{flow_pp, flow_checked, flow_fwd, flow_bwd, minC});
}

fsgm_status fsgm_pyramidal_flow_pp_device_u(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                            const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio, double* flow_pp, double* flow_checked,
                                            double* flow_fwd, double* flow_bwd, uint32_t* minC, uint32_t* minC2, void* stream,
                                            int32_t* status) {
    return flow_pp_device("fsgm_pyramidal_flow_pp_device_u", n, I0, I1, W, H, channels, prm, Uniqueness{true, uniqueness_ratio, minC2},
                          FlowOutputs{flow_pp, flow_checked, flow_fwd, flow_bwd, minC}, stream, status);
}

fsgm_status fsgm_pyramidal_flow_pp_host_lm(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                           const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio, int32_t level_median, double* flow_pp,
                                           double* flow_checked, double* flow_fwd, double* flow_bwd, uint32_t* minC, uint32_t* minC2) {
    const char* who = "fsgm_pyramidal_flow_pp_host_lm";
    const fsgm_status st = level_median_args(who, uniqueness_ratio, minC2, level_median);
    if (st != FSGM_OK) return st;
    return flow_pp_host(who, n, I0, I1, W, H, channels, prm, Uniqueness{minC2 != nullptr, uniqueness_ratio, minC2},
                        FlowOutputs{flow_pp, flow_checked, flow_fwd, flow_bwd, minC}, level_median);
}

fsgm_status fsgm_pyramidal_flow_pp_device_lm(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                             const fsgm_flow_pp_params* prm, int32_t uniqueness_ratio, int32_t level_median, double* flow_pp,
                                             double* flow_checked, double* flow_fwd, double* flow_bwd, uint32_t* minC, uint32_t* minC2,
                                             void* stream, int32_t* status) {
    const char* who = "fsgm_pyramidal_flow_pp_device_lm";
    const fsgm_status st = level_median_args(who, uniqueness_ratio, minC2, level_median);
    if (st != FSGM_OK) return st;
    return flow_pp_device(who, n, I0, I1, W, H, channels, prm, Uniqueness{minC2 != nullptr, uniqueness_ratio, minC2},
                          FlowOutputs{flow_pp, flow_checked, flow_fwd, flow_bwd, minC}, stream, status, level_median);
}

fsgm_status fsgm_pyramidal_flow_pp_time(int32_t n, const uint8_t* I0, const uint8_t* I1, int32_t W, int32_t H, int32_t channels,
                                        const fsgm_flow_pp_params* prm, int32_t warmup, int32_t iters, float* ms) {
    const char* who = "fsgm_pyramidal_flow_pp_time";
    fsgm_status st = params_check(who, prm);
    if (st != FSGM_OK || (st = flow_args(who, n, W, H, I0 && I1 && ms, prm->device)) != FSGM_OK) return st;
    FSGM_REQUIRE(iters >= 1 && warmup >= 0, "%s: iters must be >= 1 and warmup >= 0", who);
    std::unique_lock<std::mutex> lk;
    fsgm_flow_pp_plan* p;
    if ((st = flow_plan_get(lk, &p, W, H, n, prm->device)) != FSGM_OK) return st;
    const size_t np = p->NP * n;
    if ((st = ensure_pp(p, who)) != FSGM_OK) return st;
    return with_pair(n, W, H, channels, *prm, 0, 0, [&](const PyramidPair& pr) -> fsgm_status {
        hipStream_t s = pr.stream;
        const size_t img = np * channels;
        StreamGuard guard(s);
        FSGM_HIP(hipMemcpyAsync(pr.in0, I0, img, hipMemcpyHostToDevice, s));
        FSGM_HIP(hipMemcpyAsync(pr.in1, I1, img, hipMemcpyHostToDevice, s));
        fsgm_status r = swap_enqueue(pr, pr.in0, pr.in1, img);
        if (r != FSGM_OK) return r;
        FSGM_HIP(hipStreamWaitEvent(s, p->busy, 0));
        // ms[0]: the level loop, ms[1]: the chain on its flows
        if ((r = time_enqueues(s, pr.ev0, pr.ev1, warmup, iters, [&] { return pr.run(pr.plan); }, &ms[0])) != FSGM_OK) return r;
        r = time_enqueues(s, pr.ev0, pr.ev1, warmup, iters, [&]() -> fsgm_status {
            chain_enqueue(s, p, *prm, pr.flow, p->dPP, nullptr);
            FSGM_HIP(hipGetLastError());
            return FSGM_OK;
        }, &ms[1]);
        if (r != FSGM_OK) return r;
        FSGM_HIP(hipEventRecord(p->busy, s));
        guard.dismiss();
        return FSGM_OK;
    });
}

}  // extern "C"
