// epi_kernels.hip -- the shared remainder of the calc_cost_sgm path: what the other matcher families use too.  The census
// transform (capi_pyd, capi_ng and ng_kernels launch it as well), the forward-backward check, vz_convert and the bandwidth probe.
// The stages of the path itself have a unit each: epi_cost.hip (cost), epi_lines.hip + epi_lines_split.hip (line aggregation),
// epi_wta.hip (WTA), epi_sweep.hip and epi_band.hip (fused aggregation).
// (reference: calc_cost_sgm.cpp + common.cpp; citations per kernel).
//
// Data layout in HBM (all per frame, frames strided):
//   images  u8  [H][W]            census u32 [H][W]
//   maps    f64 [2][H][W] / [H][W]
//   cost volume C and per-path costs L_r: u8 [H][W][D], d fastest -> one pixel's D costs are
//   D contiguous bytes (128 B at D=128 = one L2 line), read 16 B per lane.
//
// No MFMA anywhere: this is integer stencil / scan work bound by HBM and VALU issue.
#include "epi_kernels.h"
#include "fsgm_device.h"

namespace fsgm {

// =============================================================================================
// census 5x5  (common.cpp:3-27): code = sum over the 25 taps, row-major from (-2,-2), of
// (nbr >= ctr) << (25 - tap); replicate border.
// =============================================================================================
__global__ __launch_bounds__(256) void census5x5_kernel(const uint8_t* __restrict__ img,
                                                        uint32_t* __restrict__ cen, int W, int H) {
    const int NP = W * H;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const uint8_t* im = img + (size_t)blockIdx.y * NP;
    const int y = p / W, x = p - y * W;
    const unsigned ctr = im[p];
    uint32_t code = 0;
#pragma unroll
    for (int oy = -2; oy <= 2; oy++) {
        const int y2 = clampi(y + oy, 0, H - 1);
#pragma unroll
        for (int ox = -2; ox <= 2; ox++) {
            const int x2 = clampi(x + ox, 0, W - 1);
            code = (code + (im[y2 * W + x2] >= ctr ? 1u : 0u)) << 1;
        }
    }
    cen[(size_t)blockIdx.y * NP + p] = code;
}

// The same transform, four pixels a thread (round 4; the one-pixel kernel above spends 213 instructions a pixel, most of them
// the clamped addresses of its 25 byte loads, and ran at VALU busy 1.03: 0.005 of the cost stage's 0.046 ms per frame).  A thread
// owns pixels x0 .. x0 + 3 of a row (x0 a multiple of 4) and loads the 12 bytes x0 - 4 .. x0 + 7 of each of the five rows as
// three dwords; a tap is one compare with an SDWA byte select and one add-with-carry: code = 2 code + [nbr >= ctr], the
// reference's (code + bit) << 1 with the last shift applied at the end.  Threads whose bytes would leave the image -- the two
// border rows, the first and the last columns -- take the clamped form above.
template <int BYTE>
__device__ __forceinline__ unsigned long long census_cmp(const uint32_t w, const uint32_t ctr) {      // lane mask of [byte BYTE of w >= ctr]
    unsigned long long m;
    if (BYTE == 0) asm("v_cmp_le_u32_sdwa %0, %1, %2 src0_sel:DWORD src1_sel:BYTE_0" : "=s"(m) : "v"(ctr), "v"(w));
    if (BYTE == 1) asm("v_cmp_le_u32_sdwa %0, %1, %2 src0_sel:DWORD src1_sel:BYTE_1" : "=s"(m) : "v"(ctr), "v"(w));
    if (BYTE == 2) asm("v_cmp_le_u32_sdwa %0, %1, %2 src0_sel:DWORD src1_sel:BYTE_2" : "=s"(m) : "v"(ctr), "v"(w));
    if (BYTE == 3) asm("v_cmp_le_u32_sdwa %0, %1, %2 src0_sel:DWORD src1_sel:BYTE_3" : "=s"(m) : "v"(ctr), "v"(w));
    return m;
}
__device__ __forceinline__ void census_acc(uint32_t& code, const unsigned long long m) {              // code = 2 code + bit
    asm("v_addc_co_u32 %0, vcc, %0, %0, %1" : "+v"(code) : "s"(m) : "vcc");
}
// one tap of each of the thread's four pixels: the four compares first, then the four accumulations -- a mask is read three
// instructions after it is written (back to back the pair needs a wait state: an s_nop per tap)
#define FSGM_CENSUS_TAPS(w0, b0, w1, b1, w2, b2, w3, b3)                                                                  \
    do {                                                                                                                    \
        const unsigned long long m0 = census_cmp<b0>(w0, c0), m1 = census_cmp<b1>(w1, c1), m2 = census_cmp<b2>(w2, c2),     \
                                 m3 = census_cmp<b3>(w3, c3);                                                               \
        census_acc(k0, m0); census_acc(k1, m1); census_acc(k2, m2); census_acc(k3, m3);                                     \
    } while (0)

__global__ __launch_bounds__(256) void census5x5_quad_kernel(const uint8_t* __restrict__ img, uint32_t* __restrict__ cen, int W, int H) {
    const int Wq = (W + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Wq * H) return;
    const size_t NP = (size_t)W * H;
    const uint8_t* im = img + blockIdx.y * NP;
    uint32_t* out = cen + blockIdx.y * NP;
    const int y = q / Wq, x0 = (q - y * Wq) * 4;
    if (y >= 2 && y <= H - 3 && x0 >= 4 && x0 + 7 <= W - 1) {
        const uint8_t* r0 = im + (size_t)y * W + x0;
        const uint32_t cw = *(const uint32_t*)r0;                           // (rows start at y W: dword loads at any byte address)
        const uint32_t c0 = cw & 0xFFu, c1 = (cw >> 8) & 0xFFu, c2 = (cw >> 16) & 0xFFu, c3 = cw >> 24;
        uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0;
#pragma unroll
        for (int oy = -2; oy <= 2; oy++) {
            const uint8_t* r = r0 + (ptrdiff_t)oy * W;
            const uint32_t L = *(const uint32_t*)(r - 4), M = oy == 0 ? cw : *(const uint32_t*)r, R = *(const uint32_t*)(r + 4);
            // pixel 0: columns x0 - 2 .. x0 + 2 = L.2 L.3 M.0 M.1 M.2; pixel 1: L.3 M.0 .. M.3; pixel 2: M.0 .. M.3 R.0; pixel 3: M.1 .. M.3 R.0 R.1
            FSGM_CENSUS_TAPS(L, 2, L, 3, M, 0, M, 1);                       // dx = -2
            FSGM_CENSUS_TAPS(L, 3, M, 0, M, 1, M, 2);                       // dx = -1
            FSGM_CENSUS_TAPS(M, 0, M, 1, M, 2, M, 3);                       // dx = 0
            FSGM_CENSUS_TAPS(M, 1, M, 2, M, 3, R, 0);                       // dx = +1
            FSGM_CENSUS_TAPS(M, 2, M, 3, R, 0, R, 1);                       // dx = +2
        }
        uint32_t* o = out + (size_t)y * W + x0;
        o[0] = k0 << 1; o[1] = k1 << 1; o[2] = k2 << 1; o[3] = k3 << 1;
        return;
    }
    for (int i = 0; i < 4; i++) {                                             // borders: replicate (common.cpp:17-18)
        const int x = x0 + i;
        if (x >= W) break;
        const unsigned ctr = im[(size_t)y * W + x];
        uint32_t code = 0;
        for (int oy = -2; oy <= 2; oy++) {
            const int y2 = clampi(y + oy, 0, H - 1);
            for (int ox = -2; ox <= 2; ox++) code = (code + (im[(size_t)y2 * W + clampi(x + ox, 0, W - 1)] >= ctr ? 1u : 0u)) << 1;
        }
        out[(size_t)y * W + x] = code;
    }
}

void launch_census(hipStream_t st, const uint8_t* img, uint32_t* cen, int W, int H, int frames) {
    const char* qe = getenv("FSGM_CENSUS_QUAD");                // A/B switch and test hook: 0 never, 1 whenever the shape allows, unset: by size
    const bool quad = !(qe && qe[0] == '0'), force = qe && qe[0] == '1';
    // (a single 1242x375 frame is a latency-bound launch: 466 k threads of the one-pixel kernel finish before 116 k threads of
    // this one -- cost stage 0.060 against 0.064 ms; from a few frames on the instruction count decides: 0.0427 -> 0.0408 at 512)
    if (quad && W >= 16 && H >= 5 && (force || (long long)W * H * frames >= 2000000)) {
        dim3 grid((((W + 3) / 4) * H + 255) / 256, frames);
        hipLaunchKernelGGL(census5x5_quad_kernel, grid, dim3(256), 0, st, img, cen, W, H);
        return;
    }
    dim3 grid((W * H + 255) / 256, frames);
    hipLaunchKernelGGL(census5x5_kernel, grid, dim3(256), 0, st, img, cen, W, H);
}

// =============================================================================================
// forward-backward consistency check  (calc_cost_sgm.cpp:429-480 calc_disp_from_first, :482-536
// forward_backward_check; dead code in the shipped reference -- its call at :589-590 is commented
// out -- offered here as an option).  Runs on bestD (vz index * 256) before vz->disparity.
// The reference's scatter "D2[t] = D1 if D2[t] is invalid or smaller" in raster order is a
// maximum over the contributing pixels, so it is done with atomicMax on D1+1 (0 = invalid).
// =============================================================================================
__device__ __forceinline__ double fb_displacement(const FbArgs& a, size_t f, int p, uint32_t d1) {
    const double d = __ddiv_rn((double)d1, 256.0);                                 // :447 / :502
    if (a.linear) return d;                                                        // :453 / :508 (built without USE_VZIND)
    const double r = __dmul_rn(__ddiv_rn(d, (double)a.n), a.vMax);
    const double vz = __ddiv_rn(r, __dsub_rn(1.0, r));
    return __dmul_rn(a.off[f * (size_t)a.W * a.H + p], vz);                        // :451 / :506
}

// start position - 1 (:456-457 / :510-511) and direction (:459-460 / :513-514) of pixel p: read from the maps, or those of a
// rectified pair -- Pd0 = (x + 1 + rect_shift, y + 1), direction (+-1, 0) -- through the same fp64 operations
struct FbRay { double bx, by, ux, uy; };
__device__ __forceinline__ FbRay fb_ray(const FbArgs& a, size_t f, int p) {
    const int NP = a.W * a.H;
    FbRay r;
    if (a.rect) {
        const int y = p / a.W, x = p - y * a.W;
        r.bx = __dsub_rn((double)(x + 1 + a.rect_shift), 1.0); r.by = __dsub_rn((double)(y + 1), 1.0);
        r.ux = (double)a.rect; r.uy = 0.0;
    } else {
        const double* p0 = a.pd0 + f * 2 * (size_t)NP;
        const double* nd = a.nd + f * 2 * (size_t)NP;
        r.bx = __dsub_rn(p0[p], 1.0); r.by = __dsub_rn(p0[NP + p], 1.0);
        r.ux = nd[p]; r.uy = nd[NP + p];
    }
    return r;
}

__global__ __launch_bounds__(256) void fb_scatter_kernel(FbArgs a) {
    const int NP = a.W * a.H;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const size_t f = blockIdx.y;
    const uint32_t d1 = a.D1[f * (size_t)NP + p];
    const double d = fb_displacement(a, f, p, d1);
    const FbRay r = fb_ray(a, f, p);
    const int p2x = f64_to_i32_x86(__dadd_rn(r.bx, __dmul_rn(d, r.ux)));            // :462
    const int p2y = f64_to_i32_x86(__dadd_rn(r.by, __dmul_rn(d, r.uy)));            // :463
    uint32_t* enc = a.D2enc + f * (size_t)NP;
#pragma unroll
    for (int dy = 0; dy <= 1; dy++)
#pragma unroll
        for (int dx = 0; dx <= 1; dx++) {
            const long long tx = (long long)dx + p2x, ty = (long long)dy + p2y;
            if (tx >= 0 && tx < a.W && ty >= 0 && ty < a.H) atomicMax(&enc[ty * a.W + tx], d1 + 1u);    // :471-474
        }
}

__global__ __launch_bounds__(256) void fb_check_kernel(FbArgs a) {
    const int NP = a.W * a.H;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const size_t f = blockIdx.y;
    const uint32_t INVALID = 512u << 8;                                            // :5
    const uint32_t* enc = a.D2enc + f * (size_t)NP;
    const uint32_t mine = enc[p];
    a.D2[f * (size_t)NP + p] = mine ? mine - 1u : INVALID;                         // plhs[3] in natural form
    const uint32_t d1 = a.D1[f * (size_t)NP + p];
    const double d = fb_displacement(a, f, p, d1);
    const FbRay r = fb_ray(a, f, p);
    const int p2x = round_to_i32_x86(__dadd_rn(r.bx, __dmul_rn(d, r.ux)));          // :516
    const int p2y = round_to_i32_x86(__dadd_rn(r.by, __dmul_rn(d, r.uy)));          // :517
    uint8_t ok = 1;                                                                // :485
    if (p2x < 0 || p2x > a.W - 1 || p2y < 0 || p2y > a.H - 1) ok = 0;              // :519-522
    else {
        const uint32_t t = enc[p2y * a.W + p2x];
        if (t == 0) ok = 0;                                                        // :524-527
        else {
            long long diff = (long long)(int32_t)d1 - (long long)(int32_t)(t - 1u);   // :529
            if (diff < 0) diff = -diff;
            if (diff > a.thr) ok = 0;
        }
    }
    a.conf[f * (size_t)NP + p] = ok;
}

// convert_vzInd_to_disp as its own pass (calc_cost_sgm.cpp:414-426), used when the check above
// has to see bestD before the conversion
__global__ __launch_bounds__(256) void vz_convert_kernel(uint32_t* __restrict__ bestD, const double* __restrict__ off,
                                                         int NP, int n, double vMax) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const size_t i = (size_t)blockIdx.y * NP + p;
    const double d = __ddiv_rn((double)bestD[i], 256.0);
    const double r = __dmul_rn(__ddiv_rn(d, (double)n), vMax);
    const double vz = __ddiv_rn(r, __dsub_rn(1.0, r));
    bestD[i] = f64_to_u32_x86(__dmul_rn(__dmul_rn(off[i], vz), 256.0));
}

void launch_fb_check(hipStream_t st, const FbArgs& a, int frames) {
    const int NP = a.W * a.H;
    (void)hipMemsetAsync(a.D2enc, 0, (size_t)frames * NP * 4, st);                 // :440-442 all invalid
    dim3 grid((NP + 255) / 256, frames);
    hipLaunchKernelGGL(fb_scatter_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(fb_check_kernel, grid, dim3(256), 0, st, a);
}

void launch_vz_convert(hipStream_t st, uint32_t* bestD, const double* off, int W, int H, int D, double vMax, int frames) {
    dim3 grid((W * H + 255) / 256, frames);
    hipLaunchKernelGGL(vz_convert_kernel, grid, dim3(256), 0, st, bestD, off, W * H, D + 1, vMax);
}

// Bandwidth probe: one 16-byte element per thread, streaming (non-temporal) loads and stores, as many 256-thread
// workgroups as elements / 256 -- the shape that copies fastest on this chip (tools/ubench/copy_rates.hip: 6.5 TB/s,
// against 5.2-5.5 TB/s for grid-stride loops with 2-8 elements in flight per thread and 4.7-5.4 for hipMemcpyAsync).
__global__ __launch_bounds__(256) void copy16_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) store_nt(dst + i, load_nt(src + i));
}

void launch_copy16(hipStream_t st, void* dst, const void* src, size_t bytes) {
    const size_t n16 = bytes / 16;
    hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (uint4*)dst, (const uint4*)src, n16);
}

}  // namespace fsgm
