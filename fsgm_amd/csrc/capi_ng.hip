// capi_ng.hip -- C ABI for the two neighbour-guided variants (include/fsgm.h).
// (SURVEY 8(a) a-11..a-14).  Device memory comes from a process-lifetime arena (NgPool below).
#include "capi_common.h"
#include "epi_kernels.h"
#include "ng_kernels.h"
#include <algorithm>
#include <mutex>
#include <stdlib.h>
#include <utility>
#include <vector>

using namespace fsgm;

namespace {
// Device memory of the two variants comes from one arena that lives as long as the process (like the plans
// behind the other host entry points: a MATLAB session calls the MEX once per frame, and allocating and
// freeing 0.6 GB per call costs more than the kernels).  One call at a time, as in a MEX.
struct NgPool {
    std::mutex mu;
    int device = -1;
    char* base = nullptr;
    size_t cap = 0;
    int small_calls = 0;               // consecutive calls that used at most a quarter of the arena
    hipStream_t stream = nullptr;
    // the last level of the hint-map variant's host entry points, for fsgm_ng_last_decision (kstat: in the arena; null: none)
    const uint32_t* kstat = nullptr;
    NgMatcherSet set;
    int frames = 0;
    long long pixels = 0;
};
NgPool g_pools[FSGM_MAX_DEVICES];      // one arena per device: calls on different devices run side by side

struct DevBufs {                       // the arena of `device` for the duration of one call
    NgPool& g_pool;
    std::unique_lock<std::mutex> lk;
    explicit DevBufs(int device) : g_pool(g_pools[device]), lk(g_pools[device].mu) {}
    std::vector<std::pair<void**, size_t>> req;
    hipStream_t stream = nullptr;
    // Every exit drains the arena's stream before the pool mutex (declared first, released last) lets the next
    // call re-carve the arena or the caller frees its buffers: an early error return may leave copies from the
    // caller's memory and kernels queued.  On the normal path the stream is already idle.
    ~DevBufs() { if (stream) (void)hipStreamSynchronize(stream); }
    void want(void** p, size_t bytes) { req.emplace_back(p, (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255); }
    hipError_t commit(int device) {
        size_t total = 0;
        for (auto& r : req) total += r.second;
        hipError_t e = hipSuccess;
        g_pool.kstat = nullptr;                                  // the arena is carved anew
        // the arena grows to the largest call and shrinks again once eight calls in a row used at most a quarter of it
        // (a session that moved on to smaller frames does not hold the large frames' memory until fsgm_shutdown)
        g_pool.small_calls = (g_pool.cap >= (1u << 24) && total <= g_pool.cap / 4) ? g_pool.small_calls + 1 : 0;
        if (g_pool.device != device || g_pool.cap < total || g_pool.small_calls >= 8) {
            g_pool.small_calls = 0;
            if (g_pool.base) { (void)hipSetDevice(g_pool.device); (void)hipFree(g_pool.base); (void)hipSetDevice(device); }
            if (g_pool.stream && g_pool.device != device) { (void)hipStreamDestroy(g_pool.stream); g_pool.stream = nullptr; }
            g_pool.base = nullptr; g_pool.cap = 0; g_pool.device = device;
            if ((e = hipMalloc((void**)&g_pool.base, total)) != hipSuccess) return e;
            g_pool.cap = total;
        }
        if (!g_pool.stream && (e = hipStreamCreateWithFlags(&g_pool.stream, hipStreamNonBlocking)) != hipSuccess) return e;
        stream = g_pool.stream;
        size_t used = 0;
        for (auto& r : req) { *r.first = g_pool.base + used; used += r.second; }
        return hipSuccess;
    }
};

fsgm_status pick_device(int device) {
    const fsgm_status st = use_device(device);
    if (st != FSGM_OK) return st;
    FSGM_DEVICE_SLOT(device);                                    // g_pools
    return FSGM_OK;
}
}  // namespace

extern "C" {

void fsgm_ng_shutdown_internal(void) {
    for (NgPool& g_pool : g_pools) {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        if (g_pool.device >= 0) (void)hipSetDevice(g_pool.device);
        if (g_pool.base) (void)hipFree(g_pool.base);
        if (g_pool.stream) (void)hipStreamDestroy(g_pool.stream);
        g_pool.base = nullptr; g_pool.cap = 0; g_pool.stream = nullptr; g_pool.device = -1; g_pool.kstat = nullptr;
    }
}

}  // extern "C"

// minC2s: null (the plain call), or one non-null pointer per frame (the _ru forms: the WTA kernel with the runner-up cost)
static fsgm_status ng_batch_host(int32_t n, const fsgm_ng_in* in, const fsgm_ng_out* out, uint32_t* const* minC2s, bool ru, int32_t device) {
    FSGM_REQUIRE(n >= 1 && in && out && (minC2s || !ru), "fsgm_calc_pyd_cost_sgm_ng: null argument");
    if (n > 65535) return fail(FSGM_ERR_UNSUPPORTED, "fsgm_calc_pyd_cost_sgm_ng: n_frames %d exceeds 65535 (the frame is a grid dimension)", n);
    const fsgm_ng_in& a = in[0];
    for (int i = 0; i < n; i++) {
        FSGM_REQUIRE(!ru || minC2s[i], "fsgm_calc_pyd_cost_sgm_ng: frame %d has a null minC2", i);
        FSGM_REQUIRE(in[i].I1 && in[i].I2 && in[i].preMv && out[i].minC && out[i].flow,
                     "fsgm_calc_pyd_cost_sgm_ng: frame %d has a null pointer", i);
        const fsgm_ng_in& b = in[i];
        FSGM_REQUIRE(b.width == a.width && b.height == a.height && b.mvWidth == a.mvWidth && b.mvHeight == a.mvHeight &&
                     b.halfSearchWinSize == a.halfSearchWinSize && b.aggSize == a.aggSize &&
                     b.subPixelRefine == a.subPixelRefine && b.P1 == a.P1 && b.P2 == a.P2,
                     "frames of one batch must share shape and parameters (frame %d differs)", i);
    }
    const int W = a.width, H = a.height, r = a.halfSearchWinSize, rAgg = a.aggSize / 2;
    FSGM_REQUIRE(W >= 1 && H >= 1 && a.mvWidth >= 1 && a.mvHeight >= 1, "bad image / hint-map size");
    FSGM_REQUIRE(r >= 0 && a.aggSize >= 0, "halfSearchWinSize and aggSize must be >= 0");
    const long long D = 9LL * (2 * r + 1) * (2 * r + 1);
    if (D > FSGM_NG_MAX_D) return fail(FSGM_ERR_UNSUPPORTED, "%lld candidates per pixel exceed %d", D, FSGM_NG_MAX_D);
    if ((double)W * H * D >= 2147483648.0) return fail(FSGM_ERR_UNSUPPORTED, "candidate volume exceeds 2^31 entries per frame");
    fsgm_status st = pick_device(device);
    if (st != FSGM_OK) return st;
    const size_t NP = (size_t)W * H, MV = (size_t)a.mvWidth * a.mvHeight, N = NP * D, B = n;
    DevBufs d(device);
    uint8_t *dI1, *dI2; uint32_t *dMinC, *dMinC2 = nullptr; double *dMv, *dFlow;
    NgLevelBufs nb;
    d.want((void**)&dI1, B * NP);
    d.want((void**)&dI2, B * NP);
    d.want((void**)&dMv, B * MV * 16);
    d.want((void**)&dMinC, B * NP * 4);
    d.want((void**)&dFlow, B * NP * 16);
    if (ru) d.want((void**)&dMinC2, B * NP * 4);
    for (const NgBuf& b : ng_level_bufs(nb, W, H, (int)D, n)) d.want(b.slot, b.bytes);
    if ((st = hip_status(d.commit(device), "fsgm_calc_pyd_cost_sgm_ng")) != FSGM_OK) return st;
    for (int i = 0; i < n; i++) {
        FSGM_HIP(hipMemcpyAsync(dI1 + i * NP, in[i].I1, NP, hipMemcpyHostToDevice, d.stream));
        FSGM_HIP(hipMemcpyAsync(dI2 + i * NP, in[i].I2, NP, hipMemcpyHostToDevice, d.stream));
        FSGM_HIP(hipMemcpyAsync(dMv + i * 2 * MV, in[i].preMv, MV * 16, hipMemcpyHostToDevice, d.stream));
    }
    const NgLevel lv = {dI1, dI2, dMv, dMinC, dFlow, W, H, a.mvWidth, a.mvHeight, r, rAgg, a.P1, a.P2, a.subPixelRefine, dMinC2};
    NgMatcherSet ms;
    FSGM_HIP(ng_level_enqueue(d.stream, nb, lv, n, &ms));
    bool want_S = false;
    for (int i = 0; i < n; i++) want_S = want_S || out[i].S;
    if (want_S && D <= 128) {
        launch_ng_l4_to_s(d.stream, nb.S, nb.L4, nb.cm, nb.dk, nb.kstat, W, H, (int)D, n);   // the compact kernel leaves its sums in L4
        launch_ng_fill_repeats(d.stream, nb.S, nb.dd, nb.cm, W, H, (int)D, n);             // the compact kernel adds to kept entries only
    }
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipStreamSynchronize(d.stream));
    d.g_pool.kstat = nb.kstat; d.g_pool.set = ms; d.g_pool.frames = n; d.g_pool.pixels = (long long)NP * n;
    for (int i = 0; i < n; i++) {
        FSGM_HIP(hipMemcpy(out[i].minC, dMinC + i * NP, NP * 4, hipMemcpyDeviceToHost));
        FSGM_HIP(hipMemcpy(out[i].flow, dFlow + i * 2 * NP, NP * 16, hipMemcpyDeviceToHost));
        if (out[i].S) FSGM_HIP(hipMemcpy(out[i].S, nb.S + i * N, N * 4, hipMemcpyDeviceToHost));
        if (ru) FSGM_HIP(hipMemcpy(minC2s[i], dMinC2 + i * NP, NP * 4, hipMemcpyDeviceToHost));
    }
    return FSGM_OK;
}

extern "C" {

fsgm_status fsgm_calc_pyd_cost_sgm_ng_batch_host(int32_t n, const fsgm_ng_in* in, const fsgm_ng_out* out, int32_t device) {
    return ng_batch_host(n, in, out, nullptr, false, device);
}

fsgm_status fsgm_calc_pyd_cost_sgm_ng_host(const fsgm_ng_in* in, const fsgm_ng_out* out, int32_t device) {
    return ng_batch_host(1, in, out, nullptr, false, device);
}

fsgm_status fsgm_calc_pyd_cost_sgm_ng_batch_host_ru(int32_t n, const fsgm_ng_in* in, const fsgm_ng_out* out, uint32_t* const* minC2s,
                                                    int32_t device) {
    FSGM_REQUIRE(minC2s, "fsgm_calc_pyd_cost_sgm_ng_batch_host_ru: null minC2s");
    return ng_batch_host(n, in, out, minC2s, true, device);
}

fsgm_status fsgm_calc_pyd_cost_sgm_ng_host_ru(const fsgm_ng_in* in, const fsgm_ng_out* out, uint32_t* minC2, int32_t device) {
    FSGM_REQUIRE(minC2, "fsgm_calc_pyd_cost_sgm_ng_host_ru: null minC2");
    return ng_batch_host(1, in, out, &minC2, true, device);
}

const char* fsgm_ng_auto_matcher(int32_t width, int32_t height, int32_t D, int32_t frames, uint64_t list_sum, uint64_t sample_pixels,
                                 uint32_t flags) {
    if (width < 1 || height < 1 || D < 1 || frames < 1) return "";
    return ng_auto_matcher(width, height, D, frames, list_sum, sample_pixels, flags);
}

uint64_t fsgm_ng_auto_matcher_lds(int32_t width, int32_t height, int32_t D, int32_t frames) {
    if (width < 1 || height < 1 || D < 1 || D > 256 || frames < 1) return 0;   // (256 / D lines a workgroup)
    return ng_auto_matcher_lds(width, height, D, frames);
}

uint64_t fsgm_ng_sample_pixels(uint64_t pixels) { return ng_sample_pixels(pixels); }

fsgm_status fsgm_ng_last_decision(int32_t device, const char** matcher, uint64_t* list_sum, uint64_t* sample_pixels, uint32_t* flags) {
    FSGM_REQUIRE(matcher && list_sum && sample_pixels && flags, "fsgm_ng_last_decision: null argument");
    const fsgm_status st = pick_device(device);
    if (st != FSGM_OK) return st;
    NgPool& g_pool = g_pools[device];
    std::lock_guard<std::mutex> lk(g_pool.mu);
    FSGM_REQUIRE(g_pool.kstat, "fsgm_ng_last_decision: no level of calc_pyd_cost_sgm_ng has run on device %d", device);
    *list_sum = 0; *sample_pixels = 0; *flags = 0;
    uint32_t choice = ng_choose(g_pool.set, g_pool.frames, 0, 0, 0);                 // the host's, where the set leaves no choice
    if (g_pool.set.device_choice()) {
        uint32_t k[NG_KSTAT_WORDS];
        FSGM_HIP(hipMemcpy(k, g_pool.kstat, sizeof k, hipMemcpyDeviceToHost));
        uint32_t sum = 0;                                                            // (as ng_decide_kernel adds them)
        for (int i = 0; i < 256; i++) sum += k[i];
        choice = k[NG_KSTAT_CHOICE]; *list_sum = sum; *sample_pixels = ng_sample_pixels((unsigned long long)g_pool.pixels); *flags = k[NG_KSTAT_FLAGS];
    }
    *matcher = ng_matcher_name(g_pool.set, choice);
    return FSGM_OK;
}

int64_t fsgm_sgm_ng_rand_draws(int32_t W, int32_t H) { return (int64_t)W * H * 8; }

fsgm_status fsgm_calc_cost_sgm_ng_batch_host(int32_t n, const fsgm_otf_in* in, const fsgm_otf_out* out, int32_t device) {
    FSGM_REQUIRE(n >= 1 && in && out, "fsgm_calc_cost_sgm_ng: null argument");
    if (n > 65535) return fail(FSGM_ERR_UNSUPPORTED, "fsgm_calc_cost_sgm_ng: n_frames %d exceeds 65535 (the frame is a grid dimension)", n);
    const int W = in[0].width, H = in[0].height;
    FSGM_REQUIRE(W >= 1 && H >= 1, "bad image size");
    for (int i = 0; i < n; i++) {
        FSGM_REQUIRE(in[i].I1 && in[i].I2 && out[i].minC && out[i].flow, "fsgm_calc_cost_sgm_ng: frame %d has a null pointer", i);
        FSGM_REQUIRE(in[i].width == W && in[i].height == H && in[i].P1 == in[0].P1 && in[i].P2 == in[0].P2,
                     "frames of one batch must share shape and parameters (frame %d differs)", i);
    }
    fsgm_status st = pick_device(device);
    if (st != FSGM_OK) return st;
    const size_t NP = (size_t)W * H, B = n, rowE = (size_t)W * OTF_E;
    DevBufs d(device);
    uint8_t *dI1, *dI2; uint32_t *dCen1, *dCen2, *dMinC; double* dFlow; int32_t* dRnd; Cand* dLrow;
    d.want((void**)&dI1, B * NP);
    d.want((void**)&dI2, B * NP);
    d.want((void**)&dCen1, B * NP * 4);
    d.want((void**)&dCen2, B * NP * 4);
    d.want((void**)&dRnd, B * NP * 8 * 4);
    d.want((void**)&dLrow, B * 6 * rowE * sizeof(Cand));
    d.want((void**)&dMinC, B * NP * 4);
    d.want((void**)&dFlow, B * NP * 16);
    if ((st = hip_status(d.commit(device), "fsgm_calc_cost_sgm_ng")) != FSGM_OK) return st;
    std::vector<int32_t> drawn;
    for (int i = 0; i < n; i++) {
        const int32_t* rs = in[i].rand_stream;
        if (!rs) {                                   // the reference's own source of hints: libc rand()
            drawn.resize(NP * 8);
            for (size_t k = 0; k < NP * 8; k++) drawn[k] = rand();
            rs = drawn.data();
        }
        FSGM_HIP(hipMemcpy(dRnd + i * NP * 8, rs, NP * 8 * 4, hipMemcpyHostToDevice));
        FSGM_HIP(hipMemcpyAsync(dI1 + i * NP, in[i].I1, NP, hipMemcpyHostToDevice, d.stream));
        FSGM_HIP(hipMemcpyAsync(dI2 + i * NP, in[i].I2, NP, hipMemcpyHostToDevice, d.stream));
    }
    FSGM_HIP(hipMemsetAsync(dLrow, 0, B * 6 * rowE * sizeof(Cand), d.stream));  // :205-207
    launch_census(d.stream, dI1, dCen1, W, H, n);                               // :233-234
    launch_census(d.stream, dI2, dCen2, W, H, n);
    OtfArgs oa;
    oa.I1 = dI1; oa.cen1 = dCen1; oa.cen2 = dCen2; oa.rnd = dRnd; oa.Lrow = dLrow; oa.minC = dMinC; oa.flow = dFlow;
    oa.W = W; oa.H = H; oa.P1 = in[0].P1; oa.P2 = in[0].P2;
    const char* ex = getenv("FSGM_OTF_EXACT");
    oa.exact = (ex && atoi(ex) != 0) ? 1 : 0;
    launch_otf(d.stream, oa, n);
    FSGM_HIP(hipGetLastError());
    FSGM_HIP(hipStreamSynchronize(d.stream));
    for (int i = 0; i < n; i++) {
        FSGM_HIP(hipMemcpy(out[i].minC, dMinC + i * NP, NP * 4, hipMemcpyDeviceToHost));
        FSGM_HIP(hipMemcpy(out[i].flow, dFlow + i * 2 * NP, NP * 16, hipMemcpyDeviceToHost));
    }
    return FSGM_OK;
}

fsgm_status fsgm_calc_cost_sgm_ng_host(const fsgm_otf_in* in, const fsgm_otf_out* out, int32_t device) {
    return fsgm_calc_cost_sgm_ng_batch_host(1, in, out, device);
}

}  // extern "C"
