// capi_sgm.hip -- C ABI of sgm(C, P1, P2) on batches of caller-supplied cost volumes, in host memory or in HBM (include/fsgm.h:
// fsgm_sgm_batch_host, fsgm_sgm_device, their _ru and _exact forms, the float forms).  Everything that can be refused without a device is refused here; the cached plans
// and their pipelines live in capi_epi.hip (capi_sgm.h).
#include "capi_sgm.h"
#include "capi_device.h"
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
