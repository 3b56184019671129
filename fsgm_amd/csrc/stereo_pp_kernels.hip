// stereo_pp_kernels.hip -- gfx950 kernels of the rectified-stereo post-processing chain (include/fsgm.h, "Rectified stereo:
// checked, filtered and filled disparity maps"): calc_disp_from_first.m and forward_backward_check.m with the rectified
// geometry substituted -- Pd0 = (x + 1, y + 1) in MATLAB's 1-based coordinates, direction (direction, 0), and
// disp = d_min + w in place of vzInd2Disp, w the candidate-index map (bestD / 256, >= 0 whatever d_min is).
//
// Arithmetic.  In the chain every operand is a multiple of 1/256 below 2^20 -- w < 1024, |d_min| <= 1024, x + 1 <= 8192 --
// so d_min + w, its product with +-1, the sum with x + 1 and the difference w - D2 are exact in fp64 and do not depend on
// contraction; floor and round then act on exact values.  On their own the stages take arbitrary non-negative doubles: the
// intrinsics below fix one rounding per operation, in the order the MATLAB lines write them (:13-14 / :17-18: disp .* off,
// then Pd0 + that).  The target's y is Pd0y + disp * 0 = y + 1 for every finite disp; an infinite disp has no target in
// either coordinate, so the y tests of :24-46 and :22 are those of x alone.
#include "stereo_pp_kernels.h"
#include "post_device.h"
#include <algorithm>

namespace fsgm {

// x of the target of pixel x (0-based) with value v, before floor / round: Pd0x + disp * direction
__device__ __forceinline__ double stereo_target_x(int x, double v, double d_min, double direction) {
    const double disp = __dadd_rn(d_min, v);
    return __dadd_rn((double)(x + 1), __dmul_rn(disp, direction));
}

// forward_backward_check.m:12-34 for one pixel, d2_at(t) the second-view value at 0-based column t of the pixel's row
template <class D2At>
__device__ __forceinline__ double stereo_check_px(int x, double v, int W, double d_min, double direction, double thr, D2At&& d2_at) {
    if (isnan(v)) return v;                                                                      // :12
    const double p2x = round(stereo_target_x(x, v, d_min, direction));                           // :20, half away from zero
    if (!(p2x >= 1.0 && p2x <= (double)W)) return FSGM_NAN;                                      // :22
    const double d2 = d2_at((int)p2x - 1);
    if (d2 == -1.0 || fabs(__dsub_rn(v, d2)) > thr) return FSGM_NAN;                             // :27, :32
    return v;
}

// =============================================================================================
// The fused row kernel: workgroup (r, f) builds row r of frame f's second-view map in LDS and checks row r of D1 against it.
// calc_disp_from_first.m:16-46 offers a pixel's value to the cells (s0x | s1x, s0y | s1y); here s0y is the pixel's own row
// and s1y the row below, so row r of D2 receives the offers of rows r - 1 and r of D1, at the same two columns each.  A cell
// starts at -1 (:6) and takes an offer when it holds 0 or something smaller (:25): for non-negative values that is "keep the
// maximum", whatever the order of the offers -- an LDS atomic maximum on the bit patterns (non-negative doubles order like
// integers, -1.0 is a negative integer; v + 0.0 turns -0.0, whose pattern is INT64_MIN, into +0.0).  NaN fails :25: no offer.
// Row 0 of a frame has no row above and the splat stops at the frame's last row: nothing crosses a frame boundary.  The
// barrier between splat and check is a workgroup barrier on LDS only; D2 and out are written with plain stores, each cell by
// the one workgroup that owns its row.  Global traffic: rows r - 1 and r of D1 in (row r a second time for the check, from
// cache), D2 and out out.  The LDS row is 8 * W bytes; consecutive lanes touch consecutive 8-byte cells in the fill, the
// read-out and -- where the disparity is locally constant -- the atomics, so the accesses are conflict-free there.
// A negative value (the precondition broken) raises *neg and offers nothing; every access stays in bounds.
// =============================================================================================
__global__ __launch_bounds__(256) void stereo_row_kernel(const double* __restrict__ D1, double* __restrict__ D2, double* __restrict__ out,
                                                         int W, int H, int f0, double d_min, double direction, double thr,
                                                         uint32_t* neg) {
    extern __shared__ long long row[];
    const int r = blockIdx.x;
    const size_t base = ((size_t)f0 + blockIdx.y) * ((size_t)W * H);
    for (int x = threadIdx.x; x < W; x += 256) row[x] = __double_as_longlong(-1.0);              // :6
    __syncthreads();
    for (int s = r > 0 ? r - 1 : 0; s <= r; s++) {
        const double* src = D1 + base + (size_t)s * W;
        for (int x = threadIdx.x; x < W; x += 256) {
            const double v = src[x];
            if (v < 0.0) {
                if (neg) *neg = 1u;                                                              // every writer stores the same value
            } else if (v >= 0.0) {
                const double sx0 = floor(stereo_target_x(x, v, d_min, direction));               // :16
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const double sx = sx0 + (double)k;                                           // :17
                    if (sx >= 1.0 && sx <= (double)W) atomicMax(&row[(int)sx - 1], __double_as_longlong(v + 0.0));
                }
            }
        }
    }
    __syncthreads();
    const size_t o = base + (size_t)r * W;
    for (int x = threadIdx.x; x < W; x += 256) {
        if (D2) D2[o + x] = __longlong_as_double(row[x]);
        if (out) out[o + x] = stereo_check_px(x, D1[o + x], W, d_min, direction, thr, [&](int t) { return __longlong_as_double(row[t]); });
    }
}

// frames f0 + blockIdx.z
__global__ __launch_bounds__(256) void stereo_fb_check_kernel(const double* __restrict__ D1, const double* __restrict__ D2,
                                                              double* __restrict__ out, int W, int H, int f0, double d_min,
                                                              double direction, double thr) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t o = ((size_t)f0 + blockIdx.z) * ((size_t)W * H) + (size_t)y * W;
    out[o + x] = stereo_check_px(x, D1[o + x], W, d_min, direction, thr, [&](int t) { return D2[o + t]; });
}

__global__ __launch_bounds__(256) void stereo_index_kernel(const int32_t* __restrict__ disp, double* __restrict__ w, size_t n_px, int32_t shift) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_px) w[i] = __ddiv_rn((double)(disp[i] - shift), 256.0);
}

__global__ __launch_bounds__(256) void stereo_pack_kernel(const double* __restrict__ filled, const double* __restrict__ checked,
                                                          const double* __restrict__ D2, double* __restrict__ disp_pp,
                                                          double* __restrict__ disp_checked, double* __restrict__ disp2, size_t n_px,
                                                          double d_min) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    if (disp_pp) disp_pp[i] = __dadd_rn(d_min, filled[i]);                                       // NaN + d_min stays NaN
    if (disp_checked) disp_checked[i] = __dadd_rn(d_min, checked[i]);
    if (disp2) {
        const double v = D2[i];
        disp2[i] = v == -1.0 ? -1.0 : __dadd_rn(d_min, v);
    }
}

// Uniqueness test (OpenCV's uniquenessRatio on the matcher's own sums): NaN where the runner-up cost is within `ratio` percent
// of the winner's, the input elsewhere (NaN stays NaN).  Products in 64 bits: minC2 may be anything below 2^32.  map and out
// may be the same array (no __restrict__ on them): every element is read before it is written, by the same lane.
__global__ __launch_bounds__(256) void stereo_uniqueness_kernel(const double* map, const uint32_t* __restrict__ minC,
                                                                const uint32_t* __restrict__ minC2, double* out, size_t n_px,
                                                                uint32_t keep) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_px; i += stride) {
        const uint32_t c = minC[i], c2 = minC2[i];
        const bool reject = c2 != 0xFFFFFFFFu && (uint64_t)c2 * keep < (uint64_t)c * 100u;
        const double v = map[i];
        out[i] = reject ? __builtin_nan("") : v;
    }
}

// The same test for a two-plane flow, map and out [n][2][frame_px], minC and minC2 [n][frame_px]: both planes of a rejected pixel
// become NaN.  One lane a pixel; it reads both of the pixel's values before it writes either, so out may be map itself.
__global__ __launch_bounds__(256) void flow_uniqueness_kernel(const double* map, const uint32_t* __restrict__ minC,
                                                              const uint32_t* __restrict__ minC2, double* out, size_t n_px,
                                                              size_t frame_px, uint32_t keep) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_px; i += stride) {
        const uint32_t c = minC[i], c2 = minC2[i];
        const bool reject = c2 != 0xFFFFFFFFu && (uint64_t)c2 * keep < (uint64_t)c * 100u;
        const size_t f = i / frame_px, at = i + f * frame_px;                 // f * 2 * frame_px + the pixel's index in its frame
        const double vx = map[at], vy = map[at + frame_px];
        out[at] = reject ? __builtin_nan("") : vx;
        out[at + frame_px] = reject ? __builtin_nan("") : vy;
    }
}

// launchers: the frame index of a grid stays within 65535, more frames (tiny maps only) take one launch per 65535
constexpr int STEREO_MAX_GRID_FRAMES = 65535;

void launch_stereo_row(hipStream_t st, const double* D1, double* D2, double* out, int W, int H, int nf, double d_min, double direction,
                       double thr, uint32_t* neg) {
    for (int f0 = 0; f0 < nf; f0 += STEREO_MAX_GRID_FRAMES)
        hipLaunchKernelGGL(stereo_row_kernel, dim3(H, std::min(nf - f0, STEREO_MAX_GRID_FRAMES)), dim3(256), stereo_row_lds(W), st, D1, D2,
                           out, W, H, f0, d_min, direction, thr, neg);
}

void launch_stereo_fb_check(hipStream_t st, const double* D1, const double* D2, double* out, int W, int H, int nf, double d_min,
                            double direction, double thr) {
    for (int f0 = 0; f0 < nf; f0 += STEREO_MAX_GRID_FRAMES)
        hipLaunchKernelGGL(stereo_fb_check_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, STEREO_MAX_GRID_FRAMES)), dim3(256), 0,
                           st, D1, D2, out, W, H, f0, d_min, direction, thr);
}

void launch_stereo_index(hipStream_t st, const int32_t* disp, double* w, size_t n_px, int32_t d_min) {
    hipLaunchKernelGGL(stereo_index_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, disp, w, n_px, 256 * d_min);
}

void launch_stereo_pack(hipStream_t st, const double* filled, const double* checked, const double* D2, double* disp_pp,
                        double* disp_checked, double* disp2, size_t n_px, double d_min) {
    hipLaunchKernelGGL(stereo_pack_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, filled, checked, D2, disp_pp,
                       disp_checked, disp2, n_px, d_min);
}

void launch_stereo_uniqueness(hipStream_t st, const double* map, const uint32_t* minC, const uint32_t* minC2, double* out, size_t n_px,
                              int ratio) {
    const size_t blocks = (n_px + 255) / 256;                    // grid-stride: at most 8 blocks for each of 256 CUs
    hipLaunchKernelGGL(stereo_uniqueness_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, map, minC, minC2, out,
                       n_px, (uint32_t)(100 - ratio));
}

void launch_flow_uniqueness(hipStream_t st, const double* map, const uint32_t* minC, const uint32_t* minC2, double* out, size_t n_px,
                            size_t frame_px, int ratio) {
    const size_t blocks = (n_px + 255) / 256;
    hipLaunchKernelGGL(flow_uniqueness_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, map, minC, minC2, out,
                       n_px, frame_px, (uint32_t)(100 - ratio));
}

}  // namespace fsgm
