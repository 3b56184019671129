// capi_sgm.hip -- C ABI of sgm(C, P1, P2) on batches of caller-supplied cost volumes, in host memory or in HBM (include/fsgm.h:
// fsgm_sgm_batch_host, fsgm_sgm_device, their _ru and _exact forms, the float forms).  Everything that can be refused without a device is refused here; the cached plans
// and their pipelines live in capi_epi.hip (capi_sgm.h).
#include "capi_sgm.h"
#include "capi_device.h"
#include "epi_view2.h"
#include <algorithm>
#include <string.h>
#include <vector>

using namespace fsgm;

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

// every host form; ru: the _ru form, exact: the _exact form
static fsgm_status sgm_host(const char* who, int32_t n, const uint8_t* C, int32_t W, int32_t H, int32_t D, int32_t P1, int32_t P2,
                            const fsgm_sgm_params* prm, const uint8_t* guide, uint32_t* bestD, uint32_t* minC, uint32_t* minC2, bool ru,
                            uint32_t* S, bool exact = false) {
    SgmCall c;
    const fsgm_status st = sgm_args(who, n, C, W, H, D, P1, P2, prm, guide, bestD, minC, S, minC2, ru, exact, &c);
    if (st != FSGM_OK) return st;
    // the true maximum of every frame, as fsgm_epi_plan_upload_cost takes it (either layout holds the same bytes)
    const size_t N = (size_t)W * H * D;
    std::vector<int> cmax(n, 0);
    for (int f = 0; f < n; f++) {
        const uint8_t* v = C + (size_t)f * N;
        int m = 0;
        for (size_t i = 0; i < N; i++) m = v[i] > m ? v[i] : m;
        FSGM_REQUIRE(m <= c.prm.cost_bound, "%s: frame %d holds a cost of %d, above cost_bound %d", who, f, m, c.prm.cost_bound);
        cmax[f] = m;
    }
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
    const fsgm_status st = sgm_view2_args(who, n, C, W, H, D, P1, P2, prm, v2, guide, bestD, minC, minC2, S, exact, disp2, minC_v2, conf, &c);
    if (st != FSGM_OK) return st;
    const size_t N = (size_t)W * H * D;                          // the true maximum of every frame, as fsgm_sgm_batch_host takes it
    std::vector<int> cmax(n, 0);
    for (int f = 0; f < n; f++) {
        const uint8_t* v = C + (size_t)f * N;
        int m = 0;
        for (size_t i = 0; i < N; i++) m = v[i] > m ? v[i] : m;
        FSGM_REQUIRE(m <= c.prm.cost_bound, "%s: frame %d holds a cost of %d, above cost_bound %d", who, f, m, c.prm.cost_bound);
        cmax[f] = m;
    }
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

}  // extern "C"
