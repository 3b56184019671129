// post_plan.h -- the post-processing chain's one batched enqueue and its plan (capi_post.hip), shared with the pipeline
// of test.m's frame body (fsgm_epipolar_flow_pp_*, capi_epi_driver.hip)
#pragma once
#include "capi_common.h"

namespace fsgm {

// scratch of the chain for nf maps: A, B, D2 f64 [nf][H][W]; parent, size, left i32 [nf][H][W]
struct PostScratch {
    double *A, *B, *D2;
    int32_t *parent, *size, *left;
};

// test.m:45-50 on nf maps, all pointers device memory in the layouts of fsgm.h; filterD2 receives calc_disp_from_first's
// map (s.D2 when the caller wants none), disp may be null, neg (may be null) is set when some D1 value is negative
void post_enqueue_batch(hipStream_t st, const PostScratch& s, int nf, int W, int H, const double* D1, const double* Pd0,
                        const double* nd, const double* O, double vMax, double n, double dMax, double* filterD1,
                        double* filterD2, double* disp, uint32_t* neg);

// a plan for `batch` maps; staging: also the host entry points' upload / download maps
fsgm_status post_plan_create_batch(fsgm_post_plan** out, int32_t W, int32_t H, int32_t batch, int32_t device, bool staging);
PostScratch post_plan_scratch(fsgm_post_plan* p);

}  // namespace fsgm
