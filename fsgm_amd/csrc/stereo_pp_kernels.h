// stereo_pp_kernels.h -- launch interface of the rectified-stereo post-processing kernels (stereo_pp_kernels.hip):
// calc_disp_from_first.m and forward_backward_check.m on the rectified geometry Pd0 = (x + 1, y + 1), direction
// (direction, 0), disparity = d_min + w.  Maps are f64 [nf][H][W], NaN = invalid, x fastest; no stage reads or writes across
// a frame boundary.  nf*W*H must stay below 2^31.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace fsgm {

// the widest row the row kernel takes: its LDS row is 8 * W bytes and the request stays within 64 KiB
constexpr int STEREO_PP_MAX_WIDTH = 8192;
// dynamic LDS of stereo_row_kernel, computed here for the launcher and for fsgm_stereo_pp_launch_lds
inline size_t stereo_row_lds(int W) { return (size_t)W * 8; }

// The second-view map of D1 and the check of D1 against it in one launch (one workgroup per output row and frame):
// D2 (may be null) receives the map, -1 where nothing lands; out (may be null) receives D1 with every pixel that fails the
// check set to NaN.  Neither may overlap D1.  neg (may be null) is set to 1 when some D1 value is negative.
void launch_stereo_row(hipStream_t st, const double* D1, double* D2, double* out, int W, int H, int nf, double d_min, double direction,
                       double thr, uint32_t* neg);
// forward_backward_check.m against a given second-view map: each pixel decides about itself only
void launch_stereo_fb_check(hipStream_t st, const double* D1, const double* D2, double* out, int W, int H, int nf, double d_min,
                            double direction, double thr);
// w = (disp - 256 * d_min) / 256: the candidate-index map of the matcher's int32 true disparities * 256 (exact)
void launch_stereo_index(hipStream_t st, const int32_t* disp, double* w, size_t n_px, int32_t d_min);
// the outputs of the chain, each may be null: disp_pp = d_min + filled, disp_checked = d_min + checked (NaN stays NaN),
// disp2 = -1 where D2 is -1 and d_min + D2 elsewhere
void launch_stereo_pack(hipStream_t st, const double* filled, const double* checked, const double* D2, double* disp_pp,
                        double* disp_checked, double* disp2, size_t n_px, double d_min);
// uniqueness test on the matcher's minC and runner-up cost minC2 (0xFFFFFFFF: no runner-up, never rejected), ratio in [0, 100]:
// out = NaN where (u64)minC2 * (100 - ratio) < (u64)minC * 100, map elsewhere.  out may be map itself, nothing else may overlap
void launch_stereo_uniqueness(hipStream_t st, const double* map, const uint32_t* minC, const uint32_t* minC2, double* out, size_t n_px,
                              int ratio);
// the same on a two-plane flow: map, out f64 [n][2][frame_px], minC, minC2 u32 [n][frame_px], n_px = n * frame_px; both planes of a
// rejected pixel become NaN
void launch_flow_uniqueness(hipStream_t st, const double* map, const uint32_t* minC, const uint32_t* minC2, double* out, size_t n_px,
                            size_t frame_px, int ratio);

}  // namespace fsgm
