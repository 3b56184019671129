// post_kernels.hip -- gfx950 kernels for the reference's post-processing chain (test.m:45-50), on scalar maps and on
// two-channel flows.  The MATLAB originals are sequential (raster scans, a FIFO flood fill, first-come writes); each
// kernel computes the same result in an order-free form and says why that is the same thing.  The speckle filter and the
// hole fill are one kernel set for both (templated on the channel count); the consistency checks differ in kind -- the
// epipolar one walks the geometry, the flow one follows the vector -- and stay two kernels.
#include "post_kernels.h"
#include "post_device.h"
#include "fsgm_device.h"
#include "../../include/fsgm.h"
#include <algorithm>

namespace fsgm {

// =============================================================================================
// speckle_filter.m:1-103.  The flood fill (:43-92) joins a pixel to a neighbour when both are valid
// and |a-b| < maxDiff -- a symmetric relation, so its regions are the connected components of that
// graph whatever the seed order; a region is dropped when it has fewer than maxSpeckleSize pixels
// (:94-97, and :27-30 for its later pixels).  Components by lock-free union-find: the root of a
// region is its smallest pixel index = the flood fill's seed (first pixel in raster order), so
// numbering the roots in index order reproduces the reference's labels (:37,:101).
// A batch of nf frames is one graph over the global indices f*W*H + i with no edge across a frame boundary (the merge
// tests y + 1 < H against the frame's own H), so every component lies inside one frame and its root -- the smallest
// global index -- is the smallest index of its frame: the per-frame results are those of nf single-map runs.
// The kernels take the channel count CH: a scalar map (CH = 1) or a flow (CH = 2, u then v; a pixel is valid when neither
// is NaN, and two pixels join when |du| < maxDiff and |dv| < maxDiff -- symmetric too, so the argument above holds unchanged).
// post_device.h has the three rules that depend on CH.  neg (may be null) is for scalar maps only.
// =============================================================================================
template <int CH>
__global__ __launch_bounds__(256) void ccl_init_kernel(int32_t* parent, int32_t* size, int n, const double* __restrict__ img,
                                                      uint32_t* neg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        parent[i] = i;
        size[i] = 0;
        if constexpr (CH == 1)
            if (neg && img[i] < 0.0) *neg = 1u;                  // every writer stores the same value
    }
}

// frames f0 + blockIdx.z
template <int CH>
__global__ __launch_bounds__(256) void ccl_merge_kernel(const double* __restrict__ img, int32_t* parent, int W, int H, int f0, double maxDiff) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int NP = W * H, f = f0 + (int)blockIdx.z, g = f * NP + y * W + x;
    const double* p = img + px_first<CH>(g, f, NP);
    const Px<CH> v = px_load<CH>(p, NP);
    if (!px_valid(v)) return;
    if (x + 1 < W && px_joins(v, px_load<CH>(p + 1, NP), maxDiff)) ccl_union(parent, g, g + 1);          // :53-60 (and :63-70 seen from the other side)
    if (y + 1 < H && px_joins(v, px_load<CH>(p + W, NP), maxDiff)) ccl_union(parent, g, g + W);          // :73-80 / :83-90
}

template <int CH>
__global__ __launch_bounds__(256) void ccl_count_kernel(const double* __restrict__ img, int32_t* parent, int32_t* size, int NP, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const bool valid = g < n && px_valid<CH>(img + px_first<CH>(g, NP), NP);
    int r = -1;
    if (valid) {
        r = ccl_find(parent, g);
        parent[g] = r;                                           // only ever replaces an ancestor by the root
    }
    ccl_add_sizes(valid, r, size);                               // :48 regionPixelNum
}

template <int CH>
__global__ __launch_bounds__(256) void speckle_apply_kernel(const double* __restrict__ img, double* __restrict__ out,
                                                            const int32_t* __restrict__ parent, const int32_t* __restrict__ size,
                                                            int NP, int n, double maxSpeckleSize) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const auto q = px_first<CH>(g, NP);
    Px<CH> v = px_load<CH>(img + q, NP);
    if (px_valid(v) && (double)size[parent[g]] < maxSpeckleSize)                                         // :94
#pragma unroll
        for (int c = 0; c < CH; c++) v.c[c] = FSGM_NAN;
#pragma unroll
    for (int c = 0; c < CH; c++) out[q + c * NP] = v.c[c];
}

// labels: rank of each region's root among all roots, in index order (3 small kernels: per-block
// counts, a scan of the block counts, ranks)
constexpr int SCAN_CHUNK = 1024;
__device__ __forceinline__ int block_sum_256(int v, int* sh) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const int t = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return t;
}
__global__ __launch_bounds__(256) void roots_count_kernel(const double* __restrict__ img, const int32_t* __restrict__ parent, int32_t* scan, int n) {
    __shared__ int sh[4];
    int c = 0;
    for (int k = 0; k < 4; k++) {
        const int i = blockIdx.x * SCAN_CHUNK + k * 256 + threadIdx.x;
        if (i < n && !isnan(img[i]) && parent[i] == i) c++;
    }
    const int t = block_sum_256(c, sh);
    if (threadIdx.x == 0) scan[blockIdx.x] = t;
}
__global__ void roots_scan_kernel(int32_t* scan, int nb) {       // nb is a few hundred: one thread
    if (threadIdx.x || blockIdx.x) return;
    int acc = 0;
    for (int b = 0; b < nb; b++) { const int t = scan[b]; scan[b] = acc; acc += t; }
}
__global__ __launch_bounds__(256) void roots_rank_kernel(const double* __restrict__ img, const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ scan, int32_t* rank, int n) {
    // rank[root] = 1 + number of roots before it; one wave-ordered pass per 256-pixel row of the chunk
    __shared__ int sh[4];
    int base = scan[blockIdx.x];
    for (int k = 0; k < 4; k++) {
        const int i = blockIdx.x * SCAN_CHUNK + k * 256 + threadIdx.x;
        const bool root = i < n && !isnan(img[i]) && parent[i] == i;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(root);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int before = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (lane == 0) sh[wave] = __popcll(bal);
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; w++) off += sh[w];
        const int tot = sh[0] + sh[1] + sh[2] + sh[3];
        if (root) rank[i] = base + off + before + 1;
        base += tot;
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void labels_kernel(const double* __restrict__ img, const int32_t* __restrict__ parent,
                                                     const int32_t* __restrict__ rank, int32_t* labels, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    labels[i] = isnan(img[i]) ? 0 : rank[parent[i]];             // :18 zeros, :40/:56 curLabel
}

// =============================================================================================
// vzInd2Disp.m:1-5
// =============================================================================================
__device__ __forceinline__ double vzind2disp(double w, double O, double vMax, double n) {
    const double vzRatio = __dmul_rn(__ddiv_rn(w, n), vMax);
    const double vzInd = __ddiv_rn(vzRatio, __dsub_rn(1.0, vzRatio));
    return __dmul_rn(O, vzInd);
}
__global__ __launch_bounds__(256) void vzind2disp_kernel(const double* __restrict__ w, const double* __restrict__ O,
                                                         double* __restrict__ D, size_t n_px, double vMax, double n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_px) D[i] = vzind2disp(w[i], O[i], vMax, n);
}

// =============================================================================================
// calc_disp_from_first.m:1-52.  Every pixel offers its value to the four pixels around its target
// (:24-46); a cell starts at -1 (:6) and takes an offer when it holds 0 or something smaller, which
// for maps of non-negative values (vz indices; the precondition of this kernel) is "keep the
// maximum": atomicMax on the bit patterns (non-negative doubles order like integers, -1.0 is a
// negative integer).  A NaN value makes every comparison of :24 false: no offer.  -0.0 passes the
// non-negative check but its pattern is INT64_MIN, below -1.0's: the offer is v + 0.0, which turns -0.0
// into +0.0 (the MATLAB rule stores -0.0 there; the two compare equal in forward_backward_check.m:27,32).
// =============================================================================================
__global__ __launch_bounds__(256) void fill_kernel(double* p, double v, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
// frames f0 + blockIdx.z: D1 / D2 / O at f*NP, Pd0 / nd at f*2*NP; every target lies in the pixel's own frame
__global__ __launch_bounds__(256) void disp_from_first_kernel(const double* __restrict__ D1, double* D2, PostGeom g, int W, int H, int f0) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t NP = (size_t)W * H, f = (size_t)f0 + blockIdx.z, p = f * NP + (size_t)y * W + x, q = f * NP + p;
    const double v = D1[p];
    const double disp = vzind2disp(v, g.O[p], g.vMax, g.n);                                      // :11
    const double p2x = __dadd_rn(g.Pd0[q], __dmul_rn(disp, g.nd[q]));                            // :13-14
    const double p2y = __dadd_rn(g.Pd0[NP + q], __dmul_rn(disp, g.nd[NP + q]));
    const double sx0 = floor(p2x), sy0 = floor(p2y);                                             // :16
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double sx = sx0 + (double)(k & 1), sy = sy0 + (double)(k >> 1);                    // :17, four corners :24-46
        if (sx >= 1.0 && sx <= (double)W && sy >= 1.0 && sy <= (double)H)
            atomicMax((long long*)&D2[f * NP + (size_t)((int)sy - 1) * W + ((int)sx - 1)], __double_as_longlong(v + 0.0));
    }
}

// forward_backward_check.m:1-39: each pixel decides about itself only
__global__ __launch_bounds__(256) void fb_check_map_kernel(const double* __restrict__ D1, const double* __restrict__ D2,
                                                           double* __restrict__ out, PostGeom g, int W, int H, int f0) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t NP = (size_t)W * H, f = (size_t)f0 + blockIdx.z, p = f * NP + (size_t)y * W + x, q = f * NP + p;
    const double v = D1[p];
    double r = v;
    if (!isnan(v)) {                                                                             // :12
        const double disp = vzind2disp(v, g.O[p], g.vMax, g.n);                                  // :15
        const double p2x = round(__dadd_rn(g.Pd0[q], __dmul_rn(disp, g.nd[q])));                 // :17-20, half away from zero
        const double p2y = round(__dadd_rn(g.Pd0[NP + q], __dmul_rn(disp, g.nd[NP + q])));
        if (!(p2x >= 1.0 && p2x <= (double)W && p2y >= 1.0 && p2y <= (double)H)) r = FSGM_NAN;        // :22 (a NaN target fails every test of :22 and reads D2(NaN): MATLAB errors; here: invalid)
        else {
            const double d2 = D2[f * NP + (size_t)((int)p2y - 1) * W + ((int)p2x - 1)];
            if (d2 == -1.0 || fabs(__dsub_rn(v, d2)) > 2.0) r = FSGM_NAN;                             // :27,:32 (thr :6)
        }
    }
    out[p] = r;
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
// scanline_in_fill.m:1-70.  Row pass: a run of NaN between two valid pixels takes the smaller of
// the two (:11-22; the run must not touch column 1, :14 -- that case is the left extrapolation),
// runs at the row ends take the nearest valid value (:30-46).  In order-free form: with l / r the
// nearest valid column to the left / right of a NaN pixel in the ORIGINAL row, the result is
// min(v[l], v[r]), v[r] or v[l].  l by a running-maximum scan, r by a running-minimum scan from the
// right (one workgroup per row).  Column pass (:50-69): only the cells above the first / below the
// last valid cell of a column are filled; one thread per column walks it (coalesced across columns).
// A batch: the row pass sees nf*H independent rows; the column pass has one thread per (frame, column), which walks
// the H rows of its own frame only.
// On a flow (CH = 2; scanline_in_fill.m with :16 and :19 restored) the gaps are those of channel u: l / r and the first /
// last row are those whose u is a number, and every channel takes its own min(c[l], c[r]), c[r] or c[l] there.
// =============================================================================================
template <int CH>
__global__ __launch_bounds__(256) void infill_rows_kernel(const double* __restrict__ in, double* __restrict__ out, int32_t* __restrict__ left,
                                                          int W, int H) {
    __shared__ int sh[4];
    __shared__ int carry_sh;
    const size_t NP = (size_t)W * H, lrow = (size_t)blockIdx.x * W;      // lrow: the (frame, row)'s place in `left`
    size_t row = lrow;
    if constexpr (CH > 1) row = px_first<CH>(lrow, (size_t)(blockIdx.x / H), NP);
    const double* v = in + row;
    int carry = -1;                                              // nearest valid column so far, from the left
    for (int base = 0; base < W; base += 256) {
        const int x = base + threadIdx.x;
        const int mine = (x < W && !isnan(v[x])) ? x : -1;
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
        const int mine = (xr < W && !isnan(v[x])) ? xr : -1;     // max over xr = min over x
        const int rr = max(block_scan_max_256(mine, sh), carry);
        if (xr < W) {
            Px<CH> res = px_load<CH>(v + x, NP);
            if (isnan(res.c[0])) {
                const int l = left[lrow + x], r = rr < 0 ? -1 : W - 1 - rr;
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    const double* vc = v + c * NP;
                    if (l >= 0 && r >= 0) res.c[c] = fmin(vc[l], vc[r]);   // :15-16
                    else if (r >= 0) res.c[c] = vc[r];                     // :30-37
                    else if (l >= 0) res.c[c] = vc[l];                     // :39-46
                }
            }
#pragma unroll
            for (int c = 0; c < CH; c++) out[row + c * NP + x] = res.c[c];
        }
        if (threadIdx.x == 255) carry_sh = rr;
        __syncthreads();
        carry = carry_sh;
        __syncthreads();
    }
}
template <int CH>
__global__ __launch_bounds__(256) void infill_cols_kernel(double* io, int W, int H, int nf) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nf * W) return;
    const int f = t / W, x = t - f * W;
    const size_t NP = (size_t)W * H;
    io += (size_t)f * CH * NP + x;
    int first = -1, last = -1;
    for (int y = 0; y < H; y++)
        if (!isnan(io[(size_t)y * W])) { if (first < 0) first = y; last = y; }
    if (first < 0) return;
    for (int c = 0; c < CH; c++) {
        double* p = io + c * NP;
        const double top = p[(size_t)first * W], bot = p[(size_t)last * W];
        for (int y = 0; y < first; y++) p[(size_t)y * W] = top;                  // :52-59
        for (int y = last + 1; y < H; y++) p[(size_t)y * W] = bot;               // :61-68
    }
}

// =============================================================================================
// vmf.m:1-14: a 5x5 median per channel (medfilt2, zero padding): the 13th smallest of 25.  One thread
// per pixel; the minimum of the remaining values is removed 12 times, the 13th minimum is the median
// (selection by repeated min/max exchange over a register array: no data-dependent indexing).
// NaN sorts above every number (MATLAB's sort; medfilt2's own rule is unpinned): a NaN enters the
// selection as +Inf, which leaves the 13th smallest unchanged while at least 13 window values are numbers; with fewer,
// the 13th smallest is a NaN.
// =============================================================================================
__global__ __launch_bounds__(256) void vmf_kernel(const double* __restrict__ in, double* __restrict__ out, int W, int H, int z0) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t plane = ((size_t)z0 + blockIdx.z) * W * H;
    double w[25];
    int nans = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int yy = y + dy, xx = x + dx;
            const bool in_img = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const double v = in_img ? in[plane + (size_t)(in_img ? yy : 0) * W + (in_img ? xx : 0)] : 0.0;   // zero padding
            nans += isnan(v) ? 1 : 0;
            w[(dy + 2) * 5 + dx + 2] = isnan(v) ? __longlong_as_double(0x7FF0000000000000LL) : v;
        }
    // partial selection sort: after pass i, w[i] holds the (i+1)-th smallest
#pragma unroll
    for (int i = 0; i < 13; i++)
#pragma unroll
        for (int j = i + 1; j < 25; j++) {
            const double a = w[i], b = w[j];
            w[i] = fmin(a, b);
            w[j] = fmax(a, b);
        }
    out[plane + (size_t)y * W + x] = nans > 12 ? FSGM_NAN : w[12];
}

// =============================================================================================
// test.m's per-frame body around the chain: D1 = bestD/256, then flow (:38-42) and flow2 (:50-54) in one pass
// =============================================================================================
__global__ __launch_bounds__(256) void vz_from_bestd_kernel(const uint32_t* __restrict__ bestD, double* __restrict__ D1, size_t n_px) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_px) D1[i] = __ddiv_rn((double)bestD[i], 256.0);
}

__global__ __launch_bounds__(256) void epi_pp_flow_kernel(const double* __restrict__ D1, const double* __restrict__ filterD1,
                                                          const double* __restrict__ O, const double* __restrict__ nd,
                                                          const double* __restrict__ rflow, double* __restrict__ flow,
                                                          double* __restrict__ flow2, size_t NP, size_t n_px, double vMax, double n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    const size_t f = i / NP, p = i - f * NP, m = 2 * f * NP + p, q = 3 * f * NP + p;
    const double w = D1[i], fw = filterD1[i], o = O[i];
    const double nx = nd[m], ny = nd[m + NP], rx = rflow[m], ry = rflow[m + NP];
    const double d = vzind2disp(w, o, vMax, n);                                                    // :39
    flow[q] = __dadd_rn(__dmul_rn(d, nx), rx);                                                     // :40-41
    flow[q + NP] = __dadd_rn(__dmul_rn(d, ny), ry);
    flow[q + 2 * NP] = isnan(w) ? 0.0 : 1.0;                                                       // :42
    const double fd = vzind2disp(fw, o, vMax, n);                                                  // :50
    flow2[q] = __dadd_rn(__dmul_rn(fd, nx), rx);                                                   // :51-52
    flow2[q + NP] = __dadd_rn(__dmul_rn(fd, ny), ry);
    flow2[q + 2 * NP] = isnan(fw) ? 0.0 : 1.0;                                                     // :53
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
// launchers.  Frame-indexed grids put the frame in blockIdx.z, whose range is 65535: more frames (only tiny maps
// can have that many below 2^31 pixels) take one launch per 65535.
// =============================================================================================
constexpr int MAX_GRID_Z = 65535;

void launch_vmf(hipStream_t st, const double* in, double* out, int W, int H, int planes) {
    for (int z0 = 0; z0 < planes; z0 += MAX_GRID_Z)
        hipLaunchKernelGGL(vmf_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(planes - z0, MAX_GRID_Z)), dim3(256), 0, st, in, out, W, H, z0);
}

void launch_vz_from_bestd(hipStream_t st, const uint32_t* bestD, double* D1, size_t n_px) {
    hipLaunchKernelGGL(vz_from_bestd_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, bestD, D1, n_px);
}

void launch_epi_pp_flow(hipStream_t st, const double* D1, const double* filterD1, const double* O, const double* nd,
                        const double* rflow, double* flow, double* flow2, int W, int H, int nf, double vMax, double n) {
    const size_t NP = (size_t)W * H, n_px = NP * nf;
    hipLaunchKernelGGL(epi_pp_flow_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, D1, filterD1, O, nd, rflow,
                       flow, flow2, NP, n_px, vMax, n);
}

template <int CH>
static void speckle_enqueue(hipStream_t st, const double* img, double* out, int32_t* parent, int32_t* size, int W, int H,
                            double maxDiff, double maxSpeckleSize, int nf, uint32_t* neg) {
    const int NP = W * H, n = NP * nf, nb = (n + 255) / 256;
    hipLaunchKernelGGL(ccl_init_kernel<CH>, dim3(nb), dim3(256), 0, st, parent, size, n, img, neg);
    for (int f0 = 0; f0 < nf; f0 += MAX_GRID_Z)
        hipLaunchKernelGGL(ccl_merge_kernel<CH>, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, MAX_GRID_Z)), dim3(256), 0, st, img, parent,
                           W, H, f0, maxDiff);
    hipLaunchKernelGGL(ccl_count_kernel<CH>, dim3(nb), dim3(256), 0, st, img, parent, size, NP, n);
    hipLaunchKernelGGL(speckle_apply_kernel<CH>, dim3(nb), dim3(256), 0, st, img, out, parent, size, NP, n, maxSpeckleSize);
}

void launch_speckle_filter(hipStream_t st, const double* image, double* out, int32_t* labels, int32_t* parent,
                           int32_t* size, int32_t* scan, int W, int H, double maxDiff, double maxSpeckleSize, int nf, uint32_t* neg) {
    speckle_enqueue<1>(st, image, out, parent, size, W, H, maxDiff, maxSpeckleSize, nf, neg);
    if (labels && nf == 1) {
        const int n = W * H, nb = (n + 255) / 256, nc = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
        hipLaunchKernelGGL(roots_count_kernel, dim3(nc), dim3(256), 0, st, image, parent, scan, n);
        hipLaunchKernelGGL(roots_scan_kernel, dim3(1), dim3(64), 0, st, scan, nc);
        hipLaunchKernelGGL(roots_rank_kernel, dim3(nc), dim3(256), 0, st, image, parent, scan, size, n);    // size reused as rank
        hipLaunchKernelGGL(labels_kernel, dim3(nb), dim3(256), 0, st, image, parent, size, labels, n);
    }
}

void launch_flow_speckle_filter(hipStream_t st, const double* flow, double* out, int32_t* parent, int32_t* size, int W, int H,
                                double maxDiff, double maxSpeckleSize, int nf) {
    speckle_enqueue<2>(st, flow, out, parent, size, W, H, maxDiff, maxSpeckleSize, nf, nullptr);
}

void launch_disp_from_first(hipStream_t st, const double* D1, double* D2, const PostGeom& g, int W, int H, int nf) {
    const size_t n = (size_t)W * H * nf;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D2, -1.0, n);   // :6
    for (int f0 = 0; f0 < nf; f0 += MAX_GRID_Z)
        hipLaunchKernelGGL(disp_from_first_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, MAX_GRID_Z)), dim3(256), 0, st,
                           D1, D2, g, W, H, f0);
}

void launch_fb_check(hipStream_t st, const double* D1, const double* D2, double* out, const PostGeom& g, int W, int H, int nf) {
    for (int f0 = 0; f0 < nf; f0 += MAX_GRID_Z)
        hipLaunchKernelGGL(fb_check_map_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, MAX_GRID_Z)), dim3(256), 0, st,
                           D1, D2, out, g, W, H, f0);
}

void launch_flow_fb_check(hipStream_t st, const double* f, const double* b, double* out, int W, int H, double thr, int nf) {
    for (int f0 = 0; f0 < nf; f0 += MAX_GRID_Z)
        hipLaunchKernelGGL(flow_fb_check_kernel, dim3((W + 63) / 64, (H + 3) / 4, std::min(nf - f0, MAX_GRID_Z)), dim3(256), 0, st,
                           f, b, out, W, H, f0, thr);
}

template <int CH>
static void in_fill_enqueue(hipStream_t st, const double* in, double* out, int32_t* left, int W, int H, int nf) {
    hipLaunchKernelGGL(infill_rows_kernel<CH>, dim3(H * nf), dim3(256), 0, st, in, out, left, W, H);
    hipLaunchKernelGGL(infill_cols_kernel<CH>, dim3((W * nf + 255) / 256), dim3(256), 0, st, out, W, H, nf);
}
void launch_scanline_in_fill(hipStream_t st, const double* in, double* out, int32_t* left, int W, int H, int nf) {
    in_fill_enqueue<1>(st, in, out, left, W, H, nf);
}
void launch_flow_in_fill(hipStream_t st, const double* in, double* out, int32_t* left, int W, int H, int nf) {
    in_fill_enqueue<2>(st, in, out, left, W, H, nf);
}

void launch_flow_pack(hipStream_t st, const double* filled, const double* checked, double* flow_pp, int W, int H, int nf) {
    const size_t NP = (size_t)W * H, n_px = NP * nf;
    hipLaunchKernelGGL(flow_pack_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, filled, checked, flow_pp, NP, n_px);
}

void launch_vzind2disp(hipStream_t st, const double* w, const double* O, double* D, size_t n_px, double vMax, double n) {
    hipLaunchKernelGGL(vzind2disp_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, w, O, D, n_px, vMax, n);
}

}  // namespace fsgm
