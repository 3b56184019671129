// flow_post_kernels.hip -- gfx950 kernels of the post-processing chain for 2-D flows (flow_post_kernels.h).  Each kernel is
// the order-free form of its scalar sibling in post_kernels.hip (where the argument for that form is written down) with
// the map value replaced by a flow vector; the rules that extend the reference to vectors are stated at each kernel.
#include "flow_post_kernels.h"
#include "post_device.h"
#include <algorithm>
#include <math.h>

namespace fsgm {

constexpr int MAX_GRID_Z = 65535;
#define FSGM_NAN __longlong_as_double(0x7FF8000000000000LL)

// =============================================================================================
// speckle_filter.m:1-103 on vectors.  Pixel g = f*W*H + y*W + x of the union-find has its u at f*2*W*H + y*W + x and
// its v one plane further.  The join rule (|du| < maxDiff and |dv| < maxDiff, both strict as :55) is symmetric, so the
// regions are the connected components of that graph and the union-find of the scalar filter applies unchanged.
// =============================================================================================
__global__ __launch_bounds__(256) void flow_ccl_init_kernel(int32_t* parent, int32_t* size, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        parent[i] = i;
        size[i] = 0;
    }
}

__device__ __forceinline__ bool flow_joins(double u, double v, double u2, double v2, double maxDiff) {
    return !isnan(u2) && !isnan(v2) && fabs(__dsub_rn(u, u2)) < maxDiff && fabs(__dsub_rn(v, v2)) < maxDiff;
}

// frames f0 + blockIdx.z
__global__ __launch_bounds__(256) void flow_ccl_merge_kernel(const double* __restrict__ flow, int32_t* parent, int W, int H, int f0,
                                                             double maxDiff) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int NP = W * H, f = f0 + (int)blockIdx.z, g = f * NP + y * W + x;
    const double* p = flow + (size_t)f * 2 * NP + (size_t)y * W + x;
    const double u = p[0], v = p[NP];
    if (isnan(u) || isnan(v)) return;
    if (x + 1 < W && flow_joins(u, v, p[1], p[NP + 1], maxDiff)) ccl_union(parent, g, g + 1);            // :53-60 / :63-70
    if (y + 1 < H && flow_joins(u, v, p[W], p[NP + W], maxDiff)) ccl_union(parent, g, g + W);            // :73-80 / :83-90
}

__global__ __launch_bounds__(256) void flow_ccl_count_kernel(const double* __restrict__ flow, int32_t* parent, int32_t* size, int NP, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (g < n) {
        const int f = g / NP;
        const size_t q = (size_t)g + (size_t)f * NP;                                                     // = f*2*NP + pixel
        valid = !isnan(flow[q]) && !isnan(flow[q + NP]);
    }
    int r = -1;
    if (valid) {
        r = ccl_find(parent, g);
        parent[g] = r;                                           // only ever replaces an ancestor by the root
    }
    ccl_add_sizes(valid, r, size);                               // :48 regionPixelNum
}

__global__ __launch_bounds__(256) void flow_speckle_apply_kernel(const double* __restrict__ flow, double* __restrict__ out,
                                                                 const int32_t* __restrict__ parent, const int32_t* __restrict__ size,
                                                                 int NP, int n, double maxSpeckleSize) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int f = g / NP;
    const size_t q = (size_t)g + (size_t)f * NP;
    const double u = flow[q], v = flow[q + NP];
    const bool drop = !isnan(u) && !isnan(v) && (double)size[parent[g]] < maxSpeckleSize;                // :94
    out[q] = drop ? FSGM_NAN : u;
    out[q + NP] = drop ? FSGM_NAN : v;
}

// =============================================================================================
// forward_backward_check.m:1-39 with the epipolar walk (:15-18) replaced by the flow vector: each pixel decides about
// itself only.  The two sums of :32 are one fp64 add each (no product next to them: nothing to contract).
// =============================================================================================
__global__ __launch_bounds__(256) void flow_fb_check_kernel(const double* __restrict__ fw, const double* __restrict__ bw,
                                                            double* __restrict__ out, int W, int H, int f0, double thr) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t NP = (size_t)W * H, base = ((size_t)f0 + blockIdx.z) * 2 * NP, q = base + (size_t)y * W + x;
    const double u = fw[q], v = fw[q + NP];
    bool keep = true;
    if (!isnan(u) && !isnan(v)) {                                                                        // :12
        const double p2x = round(__dadd_rn((double)(x + 1), u));                                         // :20, half away from zero
        const double p2y = round(__dadd_rn((double)(y + 1), v));
        if (!(p2x >= 1.0 && p2x <= (double)W && p2y >= 1.0 && p2y <= (double)H)) keep = false;           // :22
        else {
            const size_t t = base + (size_t)((int)p2y - 1) * W + ((int)p2x - 1);
            const double bu = bw[t], bv = bw[t + NP];
            if (isnan(bu) || isnan(bv)) keep = false;                                                    // :27, NaN for the -1 marker
            else if (fabs(__dadd_rn(u, bu)) > thr || fabs(__dadd_rn(v, bv)) > thr) keep = false;         // :32
        }
    }
    out[q] = keep ? u : FSGM_NAN;
    out[q + NP] = keep ? v : FSGM_NAN;
}

// =============================================================================================
// scanline_in_fill.m:1-70 with :16 and :19 restored.  The gaps are those of channel u: with l / r the nearest column to
// the left / right whose u is a number in the ORIGINAL row, a pixel whose u is NaN takes, per channel, min(c[l], c[r])
// (:15-16), c[r] (:30-37) or c[l] (:39-46); then the cells above the first / below the last row whose u is a number take
// that row's vector (:50-69).  One workgroup per (frame, row), then one thread per (frame, column).
// =============================================================================================
__global__ __launch_bounds__(256) void flow_infill_rows_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                               int32_t* __restrict__ left, int W, int H) {
    __shared__ int sh[4];
    __shared__ int carry_sh;
    const size_t NP = (size_t)W * H, f = blockIdx.x / H, y = blockIdx.x - f * H;
    const size_t row = f * 2 * NP + y * W, lrow = (size_t)blockIdx.x * W;
    const double* u = in + row;
    const double* v = u + NP;
    int carry = -1;                                              // nearest valid column so far, from the left
    for (int base = 0; base < W; base += 256) {
        const int x = base + threadIdx.x;
        const int mine = (x < W && !isnan(u[x])) ? x : -1;
        const int l = max(block_scan_max_256(mine, sh), carry);
        if (x < W) left[lrow + x] = l;
        if (threadIdx.x == 255) carry_sh = l;
        __syncthreads();
        carry = carry_sh;
        __syncthreads();
    }
    carry = -1;                                                  // from the right, in mirrored coordinates xr = W-1-x
    for (int base = 0; base < W; base += 256) {
        const int xr = base + threadIdx.x, x = W - 1 - xr;
        const int mine = (xr < W && !isnan(u[x])) ? xr : -1;     // max over xr = min over x
        const int rr = max(block_scan_max_256(mine, sh), carry);
        if (xr < W) {
            double ru = u[x], rv = v[x];
            if (isnan(ru)) {
                const int l = left[lrow + x], r = rr < 0 ? -1 : W - 1 - rr;
                if (l >= 0 && r >= 0) { ru = fmin(u[l], u[r]); rv = fmin(v[l], v[r]); }                  // :15-16
                else if (r >= 0) { ru = u[r]; rv = v[r]; }                                               // :30-37
                else if (l >= 0) { ru = u[l]; rv = v[l]; }                                               // :39-46
            }
            out[row + x] = ru;
            out[row + NP + x] = rv;
        }
        if (threadIdx.x == 255) carry_sh = rr;
        __syncthreads();
        carry = carry_sh;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void flow_infill_cols_kernel(double* io, int W, int H, int nf) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nf * W) return;
    const int f = t / W, x = t - f * W;
    const size_t NP = (size_t)W * H;
    double* u = io + (size_t)f * 2 * NP + x;
    int first = -1, last = -1;
    for (int y = 0; y < H; y++)
        if (!isnan(u[(size_t)y * W])) { if (first < 0) first = y; last = y; }
    if (first < 0) return;
    for (int c = 0; c < 2; c++) {
        double* p = u + c * NP;
        const double top = p[(size_t)first * W], bot = p[(size_t)last * W];
        for (int y = 0; y < first; y++) p[(size_t)y * W] = top;                  // :52-59
        for (int y = last + 1; y < H; y++) p[(size_t)y * W] = bot;               // :61-68
    }
}

// the filled flow and the validity of the checked one (test.m:53's third plane) as one [3][H][W] frame
__global__ __launch_bounds__(256) void flow_pack_kernel(const double* __restrict__ filled, const double* __restrict__ checked,
                                                        double* __restrict__ flow_pp, size_t NP, size_t n_px) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    const size_t f = i / NP, q = i + f * NP, o = q + f * NP;
    flow_pp[o] = filled[q];
    flow_pp[o + NP] = filled[q + NP];
    flow_pp[o + 2 * NP] = (isnan(checked[q]) || isnan(checked[q + NP])) ? 0.0 : 1.0;
}

// =============================================================================================
// launchers (frame-indexed grids put the frame in blockIdx.z: one launch per 65535 frames)
// =============================================================================================
void launch_flow_speckle_filter(hipStream_t st, const double* flow, double* out, int32_t* parent, int32_t* size, int W, int H,
                                double maxDiff, double maxSpeckleSize, int nf) {
    const int NP = W * H, n = NP * nf, nb = (n + 255) / 256;
    hipLaunchKernelGGL(flow_ccl_init_kernel, dim3(nb), dim3(256), 0, st, parent, size, n);
    for (int f0 = 0; f0 < nf; f0 += MAX_GRID_Z)
        hipLaunchKernelGGL(flow_ccl_merge_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, MAX_GRID_Z)), dim3(256), 0, st,
                           flow, parent, W, H, f0, maxDiff);
    hipLaunchKernelGGL(flow_ccl_count_kernel, dim3(nb), dim3(256), 0, st, flow, parent, size, NP, n);
    hipLaunchKernelGGL(flow_speckle_apply_kernel, dim3(nb), dim3(256), 0, st, flow, out, parent, size, NP, n, maxSpeckleSize);
}

void launch_flow_fb_check(hipStream_t st, const double* f, const double* b, double* out, int W, int H, double thr, int nf) {
    for (int f0 = 0; f0 < nf; f0 += MAX_GRID_Z)
        hipLaunchKernelGGL(flow_fb_check_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, MAX_GRID_Z)), dim3(256), 0, st,
                           f, b, out, W, H, f0, thr);
}

void launch_flow_in_fill(hipStream_t st, const double* in, double* out, int32_t* left, int W, int H, int nf) {
    hipLaunchKernelGGL(flow_infill_rows_kernel, dim3(H * nf), dim3(256), 0, st, in, out, left, W, H);
    hipLaunchKernelGGL(flow_infill_cols_kernel, dim3((W * nf + 255) / 256), dim3(256), 0, st, out, W, H, nf);
}

void launch_flow_pack(hipStream_t st, const double* filled, const double* checked, double* flow_pp, int W, int H, int nf) {
    const size_t NP = (size_t)W * H, n_px = NP * nf;
    hipLaunchKernelGGL(flow_pack_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, filled, checked, flow_pp, NP, n_px);
}

}  // namespace fsgm
