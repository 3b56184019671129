// cost_float_ingest.hip -- the kernels of cost_float_ingest.h: n caller volumes of float32 / float16 / bfloat16 in HBM -> a
// plan's u8 C, quantised by the rule of include/fsgm.h (fsgm_cost_format) on the way.
#include "cost_float_ingest.h"
#include "pyd_kernels.h"
#include <hip/hip_fp16.h>
#include <algorithm>
#include <cmath>
#include <string.h>

namespace fsgm {

// ---- the element types: how a voxel lies in memory and how it widens to fp32 (exact for all three)
struct CostF32 {
    using raw = float;
    static __device__ float widen(raw v) { return v; }
};
struct CostF16 {
    using raw = uint16_t;
    static __device__ float widen(raw v) { return __half2float(__ushort_as_half(v)); }
};
struct CostBF16 {
    using raw = uint16_t;
    static __device__ float widen(raw v) { return __uint_as_float((uint32_t)v << 16); }
};

// Steps 2-5 of the rule: one multiply and one add, each rounded on its own (never an FMA), round to nearest even, clamp.
// B is the bound as a float.  !(r <= B) is r > B or NaN; -0.0 is neither below 0 nor above B and converts to 0.
__device__ inline uint32_t quantise(float x, float scale, float offset, float B, uint32_t* over) {
    const float r = rintf(__fadd_rn(__fmul_rn(x, scale), offset));
    const bool lo = r < 0.0f, hi = !(r <= B);
    *over |= (uint32_t)(lo | hi);
    return (uint32_t)(hi ? B : fminf(fmaxf(r, 0.0f), B));
}
// four neighbouring voxels into the four bytes of a dword, the first in byte 0
template <class T>
__device__ inline uint32_t quantise4(const typename T::raw* e, float scale, float offset, float B, uint32_t* over) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) v |= quantise(T::widen(e[j]), scale, offset, B, over) << (8 * j);
    return v;
}

// ---- [n][H][W][D] -> the same layout in bytes: 16 bytes a lane and load (4 fp32 voxels, 8 of the 16-bit types), FQ_ROUNDS loads
// in flight, 4 or 8 bytes a lane and store.  The destination is aligned, the source is promised to lie on its element size
// only (the load is written as a copy).  The flag is one ballot and at the most one store a wave: no LDS.
constexpr int FQ_ROUNDS = 4;
template <class T>
__global__ __launch_bounds__(256) void ingestf_hwd_kernel(const typename T::raw* __restrict__ src, uint8_t* __restrict__ dst, size_t total,
                                                          float scale, float offset, float B, uint32_t* __restrict__ flag) {
    using R = typename T::raw;
    constexpr int E = 16 / sizeof(R), ROUND = 256 * E, BLOCK = FQ_ROUNDS * ROUND;
    const size_t i0 = (size_t)blockIdx.x * BLOCK + threadIdx.x * E;
    uint32_t over = 0;
    if ((size_t)(blockIdx.x + 1) * BLOCK <= total) {
        R v[FQ_ROUNDS][E];
#pragma unroll
        for (int k = 0; k < FQ_ROUNDS; k++) __builtin_memcpy(v[k], src + i0 + k * ROUND, 16);
#pragma unroll
        for (int k = 0; k < FQ_ROUNDS; k++) {
            uint32_t q[E / 4];
#pragma unroll
            for (int h = 0; h < E / 4; h++) q[h] = quantise4<T>(v[k] + 4 * h, scale, offset, B, &over);
            uint8_t* o = dst + i0 + k * ROUND;                   // (a multiple of E from an aligned base)
            if constexpr (E == 4) *reinterpret_cast<uint32_t*>(o) = q[0];
            else *reinterpret_cast<uint2*>(o) = make_uint2(q[0], q[1]);
        }
    } else {                                                     // the last workgroup: voxel by voxel
        for (int k = 0; k < FQ_ROUNDS; k++)
            for (size_t j = i0 + k * ROUND; j < i0 + k * ROUND + E && j < total; j++)
                dst[j] = (uint8_t)quantise(T::widen(src[j]), scale, offset, B, &over);
    }
    if (flag && __builtin_amdgcn_ballot_w64(over != 0) != 0 && (threadIdx.x & 63) == 0) *flag = 1u;
}

// ---- [n][H][W][Sx*Sy] -> [n][H][W][Sx][RS]: ingest2d_hwd_pad_kernel's mapping (sgm2d_ingest.hip), one thread a destination
// dword from up to 4 source voxels; those at or beyond Sy are padding, never read, and written 0.
template <class T>
__global__ __launch_bounds__(256) void ingestf_hwd_pad_kernel(const typename T::raw* __restrict__ src, uint8_t* __restrict__ dst,
                                                              size_t dwords, int Sy, int RQ, int PQ, int D, size_t srcN, size_t dstN,
                                                              float scale, float offset, float B, uint32_t* __restrict__ flag) {
    using R = typename T::raw;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    uint32_t over = 0;
    if (g < dwords) {
        const size_t px = g / (unsigned)PQ;
        const int r = (int)(g - px * (unsigned)PQ), sx = r / RQ, q = r - sx * RQ;
        const R* s = src + f * srcN + px * (size_t)D + (size_t)sx * Sy + 4 * q;
        const int nb = min(4, Sy - 4 * q);                       // >= 1: RQ = ceil(Sy / 4)
        uint32_t v = 0;
        if (nb == 4) {
            R e[4];
            __builtin_memcpy(e, s, sizeof(e));
            v = quantise4<T>(e, scale, offset, B, &over);
        } else {
            for (int e = 0; e < nb; e++) v |= quantise(T::widen(s[e]), scale, offset, B, &over) << (8 * e);
        }
        *reinterpret_cast<uint32_t*>(dst + f * dstN + 4 * g) = v;
    }
    if (flag && __builtin_amdgcn_ballot_w64(over != 0) != 0 && (threadIdx.x & 63) == 0) *flag = 1u;
}

// ---- [n][channels][H][W] -> [n][H][W][PS]: ingest2d_chw_kernel's tile (sgm2d_ingest.hip) -- INGEST_TX pixels by INGEST_TD
// bytes of the padded candidate index p = sx*RS + sy, one workgroup per tile, image row and frame; channel sx*Sy + sy, or
// sy*Sx + sx with YX.  The 1-D matcher's [n][D][H][W] -> [n][H][W][D] is the case Sx = 1, Sy = RS = PS = D: p is the channel.
// In: 16 bytes along x a lane (4 fp32 voxels, 8 of the 16-bit types), so a tile row is 16 or 8 lanes and a pass of the
// workgroup 16 or 32 rows; every load of a lane is issued before the first is quantised.  The quantised bytes go into the LDS
// tile as the u8 kernel's do ([p][x], rows 17 dwords apart): the tile holds bytes, the LDS request is the u8 kernel's.  A row
// whose p is padding or beyond PS holds zeros, which is how the padding bytes of the destination get their 0; voxels beyond
// the image row are never read and never flagged.  Out: the u8 kernel's 4 x 4 byte transposition and stores, unchanged.
template <class T, bool YX>
__global__ __launch_bounds__(256) void ingestf_chw_kernel(const typename T::raw* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                                          int Sx, int Sy, int RS, int PS, int txn, int tpn, float scale, float offset,
                                                          float B, uint32_t* __restrict__ flag) {
    using R = typename T::raw;
    constexpr int PW = INGEST_PITCH / 4;
    constexpr int E = 16 / sizeof(R), XL = INGEST_TX / E, RP = 256 / XL, K = INGEST_TD / RP;
    __shared__ uint32_t tile[INGEST_TD * PW + 1];                // (the last word: some lane flagged a voxel)
    uint32_t& any_over = tile[INGEST_TD * PW];
    const int t = threadIdx.x;
    unsigned b = blockIdx.x;
    const int x0 = (int)(b % (unsigned)txn) * INGEST_TX; b /= (unsigned)txn;
    const int p0 = (int)(b % (unsigned)tpn) * INGEST_TD;
    const int y = (int)(b / (unsigned)tpn);
    const size_t HW = (size_t)H * W, srcN = HW * Sx * Sy, dstN = HW * PS, f = blockIdx.y;
    uint32_t over = 0;
    if (t == 0) any_over = 0;
    {
        const int xl = t % XL, pr = t / XL, x = x0 + E * xl;
        const R* s = src + f * srcN + (size_t)y * W + x;
        const bool full = x + E <= W;
        const R* row[K];                                         // the voxel at (channel of p, y, x), NULL where the tile row holds zeros
        R r[K][E];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int p = p0 + pr + RP * k, sx = p / RS, sy = p - sx * RS;
            row[k] = (p < PS && sy < Sy && x < W) ? s + (size_t)(YX ? sy * Sx + sx : sx * Sy + sy) * HW : nullptr;
            if (row[k] && full) __builtin_memcpy(r[k], row[k], 16);
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            uint32_t q[E / 4];
#pragma unroll
            for (int h = 0; h < E / 4; h++) q[h] = 0;
            if (row[k] && full) {
#pragma unroll
                for (int h = 0; h < E / 4; h++) q[h] = quantise4<T>(r[k] + 4 * h, scale, offset, B, &over);
            } else if (row[k]) {
                for (int j = 0; j < W - x; j++) q[j >> 2] |= quantise(T::widen(row[k][j]), scale, offset, B, &over) << (8 * (j & 3));
            }
#pragma unroll
            for (int h = 0; h < E / 4; h++) tile[(pr + RP * k) * PW + xl * (E / 4) + h] = q[h];
        }
    }
    __syncthreads();
    if (over != 0) any_over = 1u;
    {
        const int l = t & 31, half = (t >> 5) & 1, w = t >> 6;
        const int pq = half * 8 + (l & 7), xq = w * 4 + (l >> 3);
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = tile[(4 * pq + k) * PW + xq];
        transpose4x4(v);
        const int p = p0 + 4 * pq;
        const bool whole = (PS & 3) == 0 && p + 4 <= PS;         // then every address below is a multiple of 4
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = x0 + 4 * xq + j;
            if (x < W && p < PS) {
                uint8_t* o = dst + f * dstN + ((size_t)y * W + x) * PS + p;
                if (whole) *reinterpret_cast<uint32_t*>(o) = v[j];
                else
                    for (int e = 0; e < PS - p && e < 4; e++) o[e] = (uint8_t)(v[j] >> (8 * e));
            }
        }
    }
    if (flag) {
        __syncthreads();
        if (t == 0 && any_over != 0) *flag = 1u;
    }
}

fsgm_status check_cost_format(const char* who, const fsgm_cost_format* fmt, CostFormat* out) {
    FSGM_REQUIRE(fmt, "%s: null fmt (the cost format of a float volume)", who);
    FSGM_REQUIRE(fmt->dtype == FSGM_COST_F32 || fmt->dtype == FSGM_COST_F16 || fmt->dtype == FSGM_COST_BF16,
                 "%s: fmt->dtype must be FSGM_COST_F32 (0), _F16 (1) or _BF16 (2), got %d", who, fmt->dtype);
    FSGM_REQUIRE(std::isfinite(fmt->scale) && fmt->scale != 0.0f, "%s: fmt->scale must be finite and not zero (got %g)", who, (double)fmt->scale);
    FSGM_REQUIRE(std::isfinite(fmt->offset), "%s: fmt->offset must be finite (got %g)", who, (double)fmt->offset);
    for (int r : fmt->reserved) FSGM_REQUIRE(r == 0, "%s: the reserved words of fsgm_cost_format must be zero", who);
    out->dtype = fmt->dtype; out->scale = fmt->scale; out->offset = fmt->offset;
    return FSGM_OK;
}

// f(tag) with the element type of `dtype` (a checked CostFormat's)
template <class F>
static void with_element_type(int dtype, F&& f) {
    if (dtype == FSGM_COST_F32) f(CostF32{});
    else if (dtype == FSGM_COST_F16) f(CostF16{});
    else f(CostBF16{});
}

// the channel-major layouts of both matchers: src at frame 0 of the launch, at the most 65535 frames
template <class T>
static void launch_chw(hipStream_t st, const typename T::raw* src, uint8_t* dst, int nf, int W, int H, int Sx, int Sy, int RS, int PS, bool yx,
                       const CostFormat& fmt, float B, uint32_t* flag) {
    const int txn = (W + INGEST_TX - 1) / INGEST_TX, tpn = (PS + INGEST_TD - 1) / INGEST_TD;
    const dim3 grid((unsigned)((size_t)txn * tpn * H), (unsigned)nf);
    if (yx) hipLaunchKernelGGL(HIP_KERNEL_NAME(ingestf_chw_kernel<T, true>), grid, dim3(256), 0, st, src, dst, W, H, Sx, Sy, RS, PS, txn, tpn,
                               fmt.scale, fmt.offset, B, flag);
    else    hipLaunchKernelGGL(HIP_KERNEL_NAME(ingestf_chw_kernel<T, false>), grid, dim3(256), 0, st, src, dst, W, H, Sx, Sy, RS, PS, txn, tpn,
                               fmt.scale, fmt.offset, B, flag);
}

void launch_sgm_ingest_float(hipStream_t st, const void* src, const CostFormat& fmt, uint8_t* dst, int n, int W, int H, int D, int layout,
                             int bound, uint32_t* flag) {
    const size_t N = (size_t)W * H * D;
    const float B = (float)bound;
    with_element_type(fmt.dtype, [&](auto tag) {
        using T = decltype(tag);
        using R = typename T::raw;
        const R* s = static_cast<const R*>(src);
        if (layout == FSGM_COST_LAYOUT_HWD) {
            // (launches of 2^34 voxels at the most: the grid's x extent stays below 2^31 whatever n is)
            constexpr size_t BLOCK = (size_t)FQ_ROUNDS * 256 * (16 / sizeof(R));
            const size_t total = (size_t)n * N, step = (size_t)1 << 34;
            for (size_t o = 0; o < total; o += step) {
                const size_t count = std::min(step, total - o);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(ingestf_hwd_kernel<T>), dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(256), 0, st, s + o,
                                   dst + o, count, fmt.scale, fmt.offset, B, flag);
            }
            return;
        }
        for (int f0 = 0; f0 < n; f0 += 65535)                    // (the grid's y extent)
            launch_chw<T>(st, s + (size_t)f0 * N, dst + (size_t)f0 * N, std::min(65535, n - f0), W, H, 1, D, D, D, false, fmt, B, flag);
    });
}

void launch_sgm2d_ingest_float(hipStream_t st, const void* src, const CostFormat& fmt, uint8_t* dst, int n, int W, int H, int Sx, int Sy,
                               int layout, int bound, uint32_t* flag) {
    const int D = Sx * Sy, RS = pyd_row_stride(Sx, Sy), PS = Sx * RS;
    if (layout == FSGM_COST2D_LAYOUT_HWD && PS == D) {           // the plan's layout is the caller's: the 1-D matcher's pass
        launch_sgm_ingest_float(st, src, fmt, dst, n, W, H, D, FSGM_COST_LAYOUT_HWD, bound, flag);
        return;
    }
    const float B = (float)bound;
    const size_t HW = (size_t)W * H, srcN = HW * D, dstN = HW * PS;
    with_element_type(fmt.dtype, [&](auto tag) {
        using T = decltype(tag);
        using R = typename T::raw;
        for (int f0 = 0; f0 < n; f0 += 65535) {                  // (the grid's y extent)
            const int nf = std::min(65535, n - f0);
            const R* s = static_cast<const R*>(src) + (size_t)f0 * srcN;
            uint8_t* d = dst + (size_t)f0 * dstN;
            if (layout == FSGM_COST2D_LAYOUT_HWD) {
                // (W*H*D < 2^31 and PS <= 4 D: a frame has fewer than 2^31 dwords, the grid's x extent stays below 2^23)
                const size_t dwords = dstN / 4;
                hipLaunchKernelGGL(HIP_KERNEL_NAME(ingestf_hwd_pad_kernel<T>), dim3((unsigned)((dwords + 255) / 256), (unsigned)nf), dim3(256), 0,
                                   st, s, d, dwords, Sy, RS / 4, PS / 4, D, srcN, dstN, fmt.scale, fmt.offset, B, flag);
            } else {
                launch_chw<T>(st, s, d, nf, W, H, Sx, Sy, RS, PS, layout == FSGM_COST2D_LAYOUT_DHW_YX, fmt, B, flag);
            }
        }
    });
}

}  // namespace fsgm

extern "C" fsgm_cost_format fsgm_cost_format_default(void) {
    fsgm_cost_format f;
    memset(&f, 0, sizeof(f));
    f.dtype = FSGM_COST_F32;
    f.scale = 1.0f;
    return f;
}
