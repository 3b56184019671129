// post_kernels.h -- launch interface of the post-processing kernels (the reference's MATLAB functions
// speckle_filter.m, calc_disp_from_first.m, forward_backward_check.m, scanline_in_fill.m, vzInd2Disp.m;
// chained by test.m:45-50), and of the same chain on two-channel flows (at the end).  Maps are f64 [H][W], NaN = invalid,
// x fastest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace fsgm {

struct PostGeom {           // the three maps of epipolar_geometry.m that the disparity functions use
    const double* Pd0;      // [2][H][W], 1-based pixel coordinates, plane 0 = x
    const double* nd;       // [2][H][W]
    const double* O;        // [H][W]
    double vMax, n;
};

// Every launcher takes a frame count nf: the maps are nf contiguous frames in the layouts above ([nf][H][W],
// [nf][2][H][W]), one launch per kernel covers the whole batch, and no stage reads or writes across a frame boundary.
// With nf = 1 each kernel computes exactly what the single-map form did.  nf*W*H must stay below 2^31 (i32 indices).

// speckle_filter.m: out = image with every 4-connected region (neighbours joined when both valid and
// |a-b| < maxDiff) of fewer than maxSpeckleSize pixels set to NaN (maxSpeckleSize is per region, i.e. per frame).
// parent, size: i32 [nf*H*W] scratch (parent ends up holding each pixel's region root = the region's first pixel in
// raster order of its frame).  labels (may be null; nf must then be 1): i32 [H*W], regions numbered in raster order of
// their first pixel, 0 = invalid; scan: i32 [H*W/1024 + 2] scratch for it.  neg (may be null): set to 1 when some
// pixel of `image` is negative (the device chain's report of a precondition the host entry points check on the host).
void launch_speckle_filter(hipStream_t st, const double* image, double* out, int32_t* labels, int32_t* parent,
                           int32_t* size, int32_t* scan, int W, int H, double maxDiff, double maxSpeckleSize,
                           int nf = 1, uint32_t* neg = nullptr);
void launch_disp_from_first(hipStream_t st, const double* D1, double* D2, const PostGeom& g, int W, int H, int nf = 1);
void launch_fb_check(hipStream_t st, const double* D1, const double* D2, double* out, const PostGeom& g, int W, int H, int nf = 1);
// left: i32 [nf*H*W] scratch
void launch_scanline_in_fill(hipStream_t st, const double* in, double* out, int32_t* left, int W, int H, int nf = 1);
// vmf.m: 5x5 median per plane, `planes` planes of H x W (a batch of flows: nf * channels)
void launch_vmf(hipStream_t st, const double* in, double* out, int W, int H, int planes);
void launch_vzind2disp(hipStream_t st, const double* w, const double* O, double* D, size_t n_px, double vMax, double n);

// D1 = bestD / 256 (the matcher's fixed-point vz index, vz_to_disp = 0, as a vz index map; exact)
void launch_vz_from_bestd(hipStream_t st, const uint32_t* bestD, double* D1, size_t n_px);
// test.m:38-42 and :50-54 in one pass over nf frames: flow [nf][3][H][W] from D1, flow2 from filterD1;
// O [nf][H][W], nd / rflow [nf][2][H][W]
void launch_epi_pp_flow(hipStream_t st, const double* D1, const double* filterD1, const double* O, const double* nd,
                        const double* rflow, double* flow, double* flow2, int W, int H, int nf, double vMax, double n);

// ---- the same chain on 2-D flows (the scalar vz-index map replaced by a two-channel flow) ----
// Flows are f64 [nf][2][H][W], plane 0 = u (x), x fastest; a pixel is valid when neither channel is NaN.
// 2*nf*W*H must stay below 2^31.

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
