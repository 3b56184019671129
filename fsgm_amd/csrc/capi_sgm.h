// capi_sgm.h -- what capi_sgm.hip (argument and pointer checks of the sgm batch entry points) hands to capi_epi.hip (the
// cached plans and their pipelines): a checked call.
#pragma once
#include "capi_common.h"
#include "cost_float_ingest.h"

namespace fsgm {

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

// host pointers; cmax: the largest byte of each frame's volume (none above prm.cost_bound), of a float volume prm.cost_bound
fsgm_status sgm_run_host(const SgmCall& c, const int* cmax);
// device pointers, checked (device_check_args) by the caller; cs: the caller's stream
fsgm_status sgm_run_device(const SgmCall& c, hipStream_t cs, int32_t* status);

}  // namespace fsgm
