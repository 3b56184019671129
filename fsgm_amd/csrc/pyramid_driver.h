// pyramid_driver.h -- the level loop of pyramidal_sgm.m (:24-76) shared by the two pyramidal drivers of include/fsgm.h:
// capi_pyramid.hip runs calc_pyd_cost_sgm at every level, capi_ng_pyramid.hip the neighbour-guided matcher.  Every level's
// images, hint maps and flows stay in HBM; one host call uploads the image pair and downloads the flows (the reference's
// loop does one MEX call, i.e. one round trip, per level: pyramidal_sgm.m:37-75).
//
// A plan type P (the opaque plan struct of include/fsgm.h) holds `PyramidCore core` and `Params prm` and supplies what
// depends on its matcher:
//   using Params; static constexpr int max_batch;                      its parameter struct (numPyd, device) and batch limit
//   static constexpr const char *plan_name, *entry_name, *flow_name;   names in error messages
//   static fsgm_status check(const Params&, int W, int H);              parameter checks beyond the shared ones
//   fsgm_status create_levels(); void destroy_levels();                its own per-level state (core is set up before, released after)
//   uint8_t*& gray(int img, int l); uint32_t*& minC(int l);            the slots of level l's gray images (img 0 / 1) and minC
//   fsgm_status enqueue_level(int l);                                  level l on core.stream, the hint map of level l - 1 included
//   fsgm_status set_runner_up(int on); uint32_t*& minC2();              the runner-up cost of level 1 (include/fsgm.h): with core.runner_up
//                                                                      set, level 1's WTA also writes the slot's buffer, made on first use
// With core.level_median = 3 or 5, enqueue_level makes the hint map of level l - 1 from the median-filtered flow of level l
// (launch_pyr_median_upsample2: pyramidal_sgm.m:70-71 live); core.dFlow[l] stays the unfiltered flow (:66).
// The entry points reach the gray images and minC through those slots, so that Bind<> in the device entry point swaps what
// the kernels read and write.
#pragma once
#include "capi_common.h"
#include "capi_device.h"
#include "pyramid_kernels.h"
#include <mutex>
#include <string.h>
#include <vector>

namespace fsgm {

struct PyramidCore {
    int W = 0, H = 0, channels = 1, batch = 1;   // batch: image pairs resident at once, every buffer holds `batch` frames, frame-major
    std::vector<int> Ws, Hs;                     // level l (0-based) size
    std::vector<int> mvW, mvH;                   // level l's hint map
    std::vector<uint8_t*> dP0, dP1;              // colour pyramids [3][h][w] (channels == 3 only)
    std::vector<double*> dFlow;                  // flow of level l (mvPyd{l}): [2][h][w]
    hipStream_t stream = nullptr;                // every level runs on it, in order
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DeviceJoin join;                             // device-pointer entry point: ordering with the caller's stream
    int runner_up = 0;                           // level 1's WTA also writes minC2 (pyramid_set_runner_up); part of the cached plans' key
    int level_median = 0;                        // 0, 3 or 5: medfilt2 window of the flow that becomes the next level's hints; part of the key too
};

template <class P>
void pyramid_destroy(P* p) {
    if (!p) return;
    PyramidCore& c = p->core;
    (void)hipSetDevice(p->prm.device);
    if (c.stream) (void)hipStreamSynchronize(c.stream);         // queued device-form work of an evicted plan (fsgm_epi_plan_destroy)
    p->destroy_levels();
    for (auto* v : {&c.dP0, &c.dP1})
        for (uint8_t* b : *v) if (b) (void)hipFree(b);
    for (double* b : c.dFlow) if (b) (void)hipFree(b);
    if (c.ev0) (void)hipEventDestroy(c.ev0);
    if (c.ev1) (void)hipEventDestroy(c.ev1);
    c.join.destroy();
    if (c.stream) (void)hipStreamDestroy(c.stream);
    delete p;
}

// what a plan can be refused for without a GPU: asked by plan creation and, before it touches a device, by pyramid_device
template <class P>
fsgm_status pyramid_args(int W, int H, int channels, int batch, const typename P::Params* prm) {
    FSGM_REQUIRE(batch >= 1 && batch <= P::max_batch, "batch must be in 1..%d (got %d)", P::max_batch, batch);
    FSGM_REQUIRE(prm, "%s_create: null parameters", P::plan_name);
    FSGM_REQUIRE(W >= 1 && H >= 1, "width/height must be >= 1 (got %d x %d)", W, H);
    FSGM_REQUIRE(channels == 1 || channels == 3, "channels must be 1 (gray) or 3 (RGB planes), got %d", channels);
    FSGM_REQUIRE(prm->numPyd >= 1 && prm->numPyd <= 16, "numPyd must be in 1..16 (got %d)", prm->numPyd);
    return P::check(*prm, W, H);
}

template <class P>
fsgm_status pyramid_create(P** out, int W, int H, int channels, int batch, const typename P::Params* prm) {
    FSGM_REQUIRE(out, "%s_create: null plan pointer", P::plan_name);
    *out = nullptr;
    fsgm_status st = pyramid_args<P>(W, H, channels, batch, prm);
    if (st != FSGM_OK) return st;
    if ((st = use_device(prm->device)) != FSGM_OK) return st;
    P* p = new P;
    p->prm = *prm;
    PyramidCore& c = p->core;
    c.W = W; c.H = H; c.channels = channels; c.batch = batch;
    const int n = prm->numPyd;
    c.Ws.assign(n, W); c.Hs.assign(n, H); c.mvW.resize(n); c.mvH.resize(n);
    for (int l = 1; l < n; l++) { c.Ws[l] = (c.Ws[l - 1] + 1) / 2; c.Hs[l] = (c.Hs[l - 1] + 1) / 2; }   // impyramid: ceil(size/2)
    for (int l = 0; l < n; l++) {
        // the coarsest level starts from a zero map of its own size (:34); every other level gets
        // 2*imresize(flow, 2, 'nearest') of the level above, twice that level's size (:72)
        c.mvW[l] = l == n - 1 ? c.Ws[l] : 2 * c.Ws[l + 1];
        c.mvH[l] = l == n - 1 ? c.Hs[l] : 2 * c.Hs[l + 1];
    }
    c.dP0.assign(n, nullptr); c.dP1.assign(n, nullptr); c.dFlow.assign(n, nullptr);
    hipError_t e = hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c.ev0);
    if (e == hipSuccess) e = hipEventCreate(&c.ev1);
    for (int l = 0; l < n && e == hipSuccess; l++) {
        const size_t np = (size_t)batch * c.Ws[l] * c.Hs[l];
        if (channels == 3) {
            e = hipMalloc((void**)&c.dP0[l], 3 * np);
            if (e == hipSuccess) e = hipMalloc((void**)&c.dP1[l], 3 * np);
        }
        if (e == hipSuccess) e = hipMalloc((void**)&c.dFlow[l], 2 * np * sizeof(double));
    }
    st = e == hipSuccess ? p->create_levels() : hip_status(e);
    if (st != FSGM_OK) {
        char msg[512];
        snprintf(msg, sizeof msg, "%s", fsgm_last_error());
        pyramid_destroy(p);
        return fail(st, "%s_create: %s", P::plan_name, msg);
    }
    *out = p;
    return FSGM_OK;
}

// the slot that image `img` of level 1 is uploaded to: its colour pyramid, or for gray input the matcher's gray image
template <class P>
uint8_t*& pyramid_input(P* p, int img) {
    return p->core.channels == 3 ? (img ? p->core.dP1 : p->core.dP0)[0] : p->gray(img, 0);
}

template <class P>
fsgm_status pyramid_level_size(P* p, int level, int32_t* w, int32_t* h) {
    FSGM_REQUIRE(p && w && h, "%s_level_size: null argument", P::plan_name);
    FSGM_REQUIRE(level >= 1 && level <= p->prm.numPyd, "level %d out of range 1..%d", level, p->prm.numPyd);
    *w = p->core.Ws[level - 1]; *h = p->core.Hs[level - 1];
    return FSGM_OK;
}

template <class P>
fsgm_status pyramid_upload_frame(P* p, int frame, const uint8_t* I0, const uint8_t* I1) {
    FSGM_REQUIRE(p && I0 && I1, "%s_upload: null argument", P::plan_name);
    FSGM_REQUIRE(frame >= 0 && frame < p->core.batch, "frame %d out of range (batch %d)", frame, p->core.batch);
    FSGM_HIP(hipSetDevice(p->prm.device));
    const size_t n = (size_t)p->core.channels * p->core.W * p->core.H;
    hipStream_t s = p->core.stream;
    StreamGuard guard(s);   // an early exit drains the stream: queued copies use the caller's memory
    FSGM_HIP(hipMemcpyAsync(pyramid_input(p, 0) + frame * n, I0, n, hipMemcpyHostToDevice, s));
    FSGM_HIP(hipMemcpyAsync(pyramid_input(p, 1) + frame * n, I1, n, hipMemcpyHostToDevice, s));
    FSGM_HIP(hipStreamSynchronize(s));
    guard.dismiss();
    return FSGM_OK;
}

template <class P>
fsgm_status pyramid_download_frame(P* p, int frame, int level, double* flow, uint32_t* minC) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(frame >= 0 && frame < p->core.batch, "frame %d out of range (batch %d)", frame, p->core.batch);
    FSGM_REQUIRE(level >= 1 && level <= p->prm.numPyd, "level %d out of range 1..%d", level, p->prm.numPyd);
    FSGM_HIP(hipSetDevice(p->prm.device));
    FSGM_HIP(hipStreamSynchronize(p->core.stream));
    const int l = level - 1;
    const size_t np = (size_t)p->core.Ws[l] * p->core.Hs[l];
    if (flow) FSGM_HIP(hipMemcpy(flow, p->core.dFlow[l] + (size_t)frame * 2 * np, 2 * np * sizeof(double), hipMemcpyDeviceToHost));
    if (minC) FSGM_HIP(hipMemcpy(minC, p->minC(l) + (size_t)frame * np, np * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

// The runner-up cost of level 1, 0 at creation: no other level's WTA and no other output changes with it
template <class P>
fsgm_status pyramid_set_runner_up(P* p, int on) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_REQUIRE(on == 0 || on == 1, "%s_set_runner_up: on must be 0 or 1 (got %d)", P::plan_name, on);
    FSGM_HIP(hipSetDevice(p->prm.device));
    const fsgm_status st = p->set_runner_up(on);
    if (st == FSGM_OK) p->core.runner_up = on;
    return st;
}

template <class P>
fsgm_status pyramid_download_runner_up(P* p, int frame, uint32_t* minC2) {
    FSGM_REQUIRE(p && minC2, "%s_download_runner_up: null argument", P::plan_name);
    FSGM_REQUIRE(frame >= 0 && frame < p->core.batch, "frame %d out of range (batch %d)", frame, p->core.batch);
    FSGM_REQUIRE(p->core.runner_up, "%s_download_runner_up: the plan's runner-up switch is off (%s_set_runner_up)", P::plan_name, P::plan_name);
    FSGM_HIP(hipSetDevice(p->prm.device));
    FSGM_HIP(hipStreamSynchronize(p->core.stream));
    const size_t np = (size_t)p->core.W * p->core.H;
    FSGM_HIP(hipMemcpy(minC2, p->minC2() + (size_t)frame * np, np * 4, hipMemcpyDeviceToHost));
    return FSGM_OK;
}

// The median between levels: 0 (off, at creation), 3 or 5.  Any numPyd, toggled between runs, no buffer of its own
inline fsgm_status level_median_check(const char* who, int size) {
    FSGM_REQUIRE(size == 0 || size == 3 || size == 5, "%s: level_median must be 0, 3 or 5 (got %d)", who, size);
    return FSGM_OK;
}

template <class P>
fsgm_status pyramid_set_level_median(P* p, int size) {
    char who[64];
    snprintf(who, sizeof who, "%s_set_level_median", P::plan_name);
    const fsgm_status st = level_median_check(who, size);
    if (st != FSGM_OK) return st;
    FSGM_REQUIRE(p, "%s: null plan", who);
    p->core.level_median = size;
    return FSGM_OK;
}

// impyramid 'reduce' (:28-31) and rgb2gray (:44-45) of every level, all frames' planes in one launch
template <class P>
void pyramid_enqueue_images(P* p) {
    const PyramidCore& c = p->core;
    const int n = p->prm.numPyd, ch = c.channels;
    for (int l = 1; l < n; l++)
        for (int i = 0; i < 2; i++) {
            const std::vector<uint8_t*>& rgb = i ? c.dP1 : c.dP0;
            launch_pyr_reduce(c.stream, ch == 3 ? rgb[l - 1] : p->gray(i, l - 1), ch == 3 ? rgb[l] : p->gray(i, l), c.Ws[l - 1], c.Hs[l - 1], ch * c.batch);
        }
    if (ch == 3)
        for (int l = 0; l < n; l++) {
            launch_pyr_gray(c.stream, c.dP0[l], p->gray(0, l), c.Ws[l], c.Hs[l], c.batch);
            launch_pyr_gray(c.stream, c.dP1[l], p->gray(1, l), c.Ws[l], c.Hs[l], c.batch);
        }
}

template <class P>
fsgm_status pyramid_enqueue(P* p) {
    pyramid_enqueue_images(p);
    for (int l = p->prm.numPyd - 1; l >= 0; l--) {                               // :37
        const fsgm_status st = p->enqueue_level(l);
        if (st != FSGM_OK) return st;
    }
    FSGM_HIP(hipGetLastError());
    return FSGM_OK;
}

template <class P>
fsgm_status pyramid_run(P* p) {
    FSGM_REQUIRE(p, "null plan");
    FSGM_HIP(hipSetDevice(p->prm.device));
    return pyramid_enqueue(p);
}

template <class P>
fsgm_status pyramid_time(P* p, int warmup, int iters, float* ms_avg) {
    FSGM_REQUIRE(p && ms_avg && iters >= 1 && warmup >= 0, "%s_time: bad argument", P::plan_name);
    FSGM_HIP(hipSetDevice(p->prm.device));
    const PyramidCore& c = p->core;
    return time_enqueues(c.stream, c.ev0, c.ev1, warmup, iters, [&] { return pyramid_enqueue(p); }, ms_avg);
}

// The plans behind the host- and device-pointer entry points: the last two per device, keyed by shape, parameters, batch, the
// runner-up switch (a call that asks for minC2 never takes the plan of one that does not, nor the reverse) and the level median
template <class P>
struct PyramidCache : PlanCache<P> {
    PyramidCache() : PlanCache<P>(2, pyramid_destroy<P>) {}
    // the cached plan of this shape, parameter set and batch (the caller holds the device's lock)
    fsgm_status get(P** out, int W, int H, int channels, const typename P::Params* prm, int batch, int ru = 0, int lm = 0) {
        *out = this->find(prm->device, [&](const P* q) {
            return q->core.W == W && q->core.H == H && q->core.channels == channels && q->core.batch == batch && memcmp(&q->prm, prm, sizeof *prm) == 0 &&
                   q->core.runner_up == ru && q->core.level_median == lm;
        });
        if (*out) return FSGM_OK;
        fsgm_status st = pyramid_create(out, W, H, channels, batch, prm);
        if (st == FSGM_OK && ru && (st = pyramid_set_runner_up(*out, 1)) != FSGM_OK) { pyramid_destroy(*out); *out = nullptr; }
        if (st == FSGM_OK) { (*out)->core.level_median = lm; this->insert(prm->device, *out); }
        return st;
    }
};

// A cached plan of batch 2n seen from the flow chain (capi_flow_pp.hip): frames 0..n-1 match I0 -> I1, frames n..2n-1
// I1 -> I0, so one run of the level loop leaves the forward and the backward flow side by side.
struct PyramidPair {
    hipStream_t stream;                          // the plan's: images in, enqueue(), and whatever reads the results
    hipEvent_t ev0, ev1;
    DeviceJoin* join;
    uint8_t *in0, *in1;                          // level-1 inputs, u8 [2n][channels][H][W]: first / second image of each frame
    const double* flow;                          // level-1 flow  [2n][2][H][W]
    const uint32_t* minC;                        // level-1 minC  [2n][H][W]
    const uint32_t* minC2;                       // level-1 runner-up cost [2n][H][W]; null in a plan without the switch
    void* plan;
    fsgm_status (*run)(void* plan);              // the level loop on `stream`
};

// body(pair) under the device's lock, on the cached plan for 2n frames of this shape, these parameters, this runner-up switch and
// this level median
template <class P, class Body>
fsgm_status pyramid_with_pair(PyramidCache<P>& cache, int n, int W, int H, int channels, const typename P::Params* prm, int ru, int lm, Body&& body) {
    FSGM_REQUIRE(n >= 1 && n <= P::max_batch / 2, "%s: n_frames must be in 1..%d (got %d)", P::entry_name, P::max_batch / 2, n);
    FSGM_DEVICE_SLOT(prm->device);
    std::lock_guard<std::mutex> lk(cache.mu(prm->device));
    P* p = nullptr;
    fsgm_status st;
    if ((st = cache.get(&p, W, H, channels, prm, 2 * n, ru, lm)) != FSGM_OK) return st;
    FSGM_HIP(hipSetDevice(prm->device));
    PyramidCore& c = p->core;
    const PyramidPair pr{c.stream, c.ev0, c.ev1, &c.join, pyramid_input(p, 0), pyramid_input(p, 1), c.dFlow[0], p->minC(0), ru ? p->minC2() : nullptr, p,
                         [](void* q) { return pyramid_enqueue(static_cast<P*>(q)); }};
    return body(pr);
}

// host pointers: one call = the whole loop on a cached plan.  ru: minC2 of level 1 comes down too (the _ru form, where it is never
// NULL, or an _lm form that was given one).  lm: the level median, checked when the call is an _lm form
template <class P>
fsgm_status pyramid_host(PyramidCache<P>& cache, const uint8_t* I0, const uint8_t* I1, int W, int H, int channels,
                         const typename P::Params* prm, double* flow, uint32_t* minC, double* const* flowPyd, uint32_t* minC2 = nullptr,
                         bool ru = false, int lm = 0, bool lm_form = false) {
    FSGM_REQUIRE(I0 && I1 && prm && flow, "%s: null argument", P::entry_name);
    FSGM_REQUIRE(!ru || minC2, "%s_ru: null argument (minC2 is required)", P::entry_name);
    if (lm_form) {
        char who[64];
        snprintf(who, sizeof who, "%s_host_lm", P::entry_name);
        const fsgm_status ls = level_median_check(who, lm);
        if (ls != FSGM_OK) return ls;
    }
    FSGM_DEVICE_SLOT(prm->device);
    std::lock_guard<std::mutex> lk(cache.mu(prm->device));
    P* p = nullptr;
    fsgm_status st;
    if ((st = cache.get(&p, W, H, channels, prm, 1, ru, lm)) != FSGM_OK) return st;
    // One call = one stream-ordered sequence with a single host wait (like fsgm_calc_cost_sgm_batch_host): the image pair goes up
    // asynchronously, the level loop follows, every requested map comes down behind it.  (Round 3's form waited after the
    // upload, after the run and once per downloaded map, with blocking copies: 6.3 ms per call around 1.4 ms of kernels.)
    const PyramidCore& c = p->core;
    FSGM_HIP(hipSetDevice(prm->device));
    StreamGuard guard(c.stream);                         // an early exit drains the stream: queued copies use the caller's memory
    const size_t nimg = (size_t)channels * W * H;
    FSGM_HIP(hipMemcpyAsync(pyramid_input(p, 0), I0, nimg, hipMemcpyHostToDevice, c.stream));
    FSGM_HIP(hipMemcpyAsync(pyramid_input(p, 1), I1, nimg, hipMemcpyHostToDevice, c.stream));
    if ((st = pyramid_enqueue(p)) != FSGM_OK) return st;
    const size_t np1 = (size_t)W * H;
    FSGM_HIP(hipMemcpyAsync(flow, c.dFlow[0], 2 * np1 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (minC) FSGM_HIP(hipMemcpyAsync(minC, p->minC(0), np1 * 4, hipMemcpyDeviceToHost, c.stream));
    if (ru) FSGM_HIP(hipMemcpyAsync(minC2, p->minC2(), np1 * 4, hipMemcpyDeviceToHost, c.stream));
    if (flowPyd)
        for (int l = 0; l < prm->numPyd; l++)
            if (flowPyd[l] && flowPyd[l] != flow)
                FSGM_HIP(hipMemcpyAsync(flowPyd[l], c.dFlow[l], 2 * (size_t)c.Ws[l] * c.Hs[l] * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    FSGM_HIP(hipStreamSynchronize(c.stream));
    guard.dismiss();
    return FSGM_OK;
}

// device pointers in and out, ordered on the caller's stream (include/fsgm.h): the level-1 images are read in place by the
// first reduce / gray / census kernels, the level-1 flow and minC are written in place -- no copy at either end
template <class P>
fsgm_status pyramid_device(PyramidCache<P>& cache, int32_t n, const uint8_t* I0, const uint8_t* I1, int W, int H, int channels,
                           const typename P::Params* prm, double* flow, uint32_t* minC, void* stream, int32_t* status, uint32_t* minC2 = nullptr,
                           bool ru = false, int lm = 0, bool lm_form = false) {
    char who[64];
    snprintf(who, sizeof who, "%s_device%s", P::entry_name, lm_form ? "_lm" : ru ? "_ru" : "");
    if (lm_form) {
        const fsgm_status ls = level_median_check(who, lm);
        if (ls != FSGM_OK) return ls;
    }
    FSGM_REQUIRE(n >= 1, "%s: n_frames must be >= 1 (got %d)", who, n);
    FSGM_REQUIRE(I0 && I1 && prm && flow, "%s: null argument", who);
    FSGM_REQUIRE(!ru || minC2, "%s: null argument (minC2 is required)", who);
    FSGM_REQUIRE(W >= 1 && H >= 1, "%s: width/height must be >= 1 (got %d x %d)", who, W, H);
    FSGM_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 (gray) or 3 (RGB planes), got %d", who, channels);
    FSGM_DEVICE_SLOT(prm->device);
    fsgm_status st = pyramid_args<P>(W, H, channels, n, prm);
    if (st != FSGM_OK) return st;
    const size_t np = (size_t)n * W * H;
    const hipStream_t cs = (hipStream_t)stream;
    if ((st = device_check_args(who, prm->device, cs, {{I0, np * channels, 1, true, "I0"},
                                                       {I1, np * channels, 1, true, "I1"},
                                                       {flow, np * 16, 8, true, P::flow_name},
                                                       {minC, np * 4, 4, false, "minC"},
                                                       {ru ? minC2 : nullptr, np * 4, 4, ru, "minC2"},
                                                       {status, 4, 4, false, "status"}})) != FSGM_OK)
        return st;
    std::lock_guard<std::mutex> lk(cache.mu(prm->device));
    P* p = nullptr;
    if ((st = cache.get(&p, W, H, channels, prm, n, ru, lm)) != FSGM_OK) return st;
    const hipStream_t ps = p->core.stream;
    return device_call(p->core.join, cs, ps, [&]() -> fsgm_status {
        Bind<uint8_t> i0(pyramid_input(p, 0), const_cast<uint8_t*>(I0));
        Bind<uint8_t> i1(pyramid_input(p, 1), const_cast<uint8_t*>(I1));
        Bind<double> fl(p->core.dFlow[0], flow);
        Bind<uint32_t> mc(p->minC(0), minC);
        Bind<uint32_t> m2(ru ? p->minC2() : p->minC(0), ru ? minC2 : nullptr);   // (a null value binds nothing)
        const fsgm_status es = pyramid_enqueue(p);
        if (es == FSGM_OK) launch_device_status(ps, nullptr, nullptr, status);
        return es;
    });
}

}  // namespace fsgm
