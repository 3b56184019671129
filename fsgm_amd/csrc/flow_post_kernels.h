// flow_post_kernels.h -- launch interface of the post-processing kernels for 2-D flows: the chain of test.m:45-49 with the
// scalar vz-index map replaced by a two-channel flow (speckle_filter.m, forward_backward_check.m, scanline_in_fill.m).
// Flows are f64 [nf][2][H][W], plane 0 = u (x), x fastest; a pixel is valid when neither channel is NaN.
// Every launcher covers nf frames with one launch per kernel; no stage reads or writes across a frame boundary.
// nf*W*H must stay below 2^31 (i32 pixel indices).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace fsgm {

// speckle_filter.m with the neighbour test of :55 on vectors: two 4-connected valid pixels join when |du| < maxDiff and
// |dv| < maxDiff; a region of fewer than maxSpeckleSize pixels becomes NaN in both channels; invalid pixels are copied.
// parent, size: i32 [nf*H*W] scratch.
void launch_flow_speckle_filter(hipStream_t st, const double* flow, double* out, int32_t* parent, int32_t* size, int W, int H,
                                double maxDiff, double maxSpeckleSize, int nf);
// forward_backward_check.m with the target p2 = round(p + f(p)) (:20, p in MATLAB's 1-based coordinates): a valid pixel of
// f becomes NaN when p2 leaves the image (:22), b(p2) is invalid (:27) or |f_u + b_u(p2)| > thr or |f_v + b_v(p2)| > thr (:32)
void launch_flow_fb_check(hipStream_t st, const double* f, const double* b, double* out, int W, int H, double thr, int nf);
// scanline_in_fill.m with lines 16 and 19 restored: the gaps are those of channel u (input(v, u) of a 3-D array is its first
// plane), both channels are filled.  left: i32 [nf*H*W] scratch
void launch_flow_in_fill(hipStream_t st, const double* in, double* out, int32_t* left, int W, int H, int nf);
// flow_pp [nf][3][H][W]: the two planes of `filled`, and 1.0 where `checked` is valid, else 0.0
void launch_flow_pack(hipStream_t st, const double* filled, const double* checked, double* flow_pp, int W, int H, int nf);

}  // namespace fsgm
