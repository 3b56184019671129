// epi_wta.hip -- winner-takes-all over the line kernels' per-path volumes (calc_cost_sgm.cpp:259-308, :414-426): the packed
// kernels of every class of FSGM_LINE_CLASSES (epi_kernels.h), plain and with the runner-up cost, the generic kernels for any
// other D, and the debug sum over paths.
#include "epi_kernels.h"
#include "fsgm_device.h"
#include "epi_wta_tail.h"

namespace fsgm {

// =============================================================================================
// S = sum over paths (debug tap of the reference's Sp, calc_cost_sgm.cpp:227-232)
// =============================================================================================
__global__ __launch_bounds__(256) void sum_paths_kernel(const uint8_t* __restrict__ L, uint32_t* __restrict__ S,
                                                        size_t n, size_t dir_stride, int ndirs) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t s = 0;
    for (int r = 0; r < ndirs; r++) s += L[r * dir_stride + i];
    S[i] = s;
}
// an exact plan's volumes hold y_r = L_r - C: S = ndirs * C + the sum of the y_r
__global__ __launch_bounds__(256) void sum_paths_exact_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ C,
                                                              uint32_t* __restrict__ S, size_t n, size_t dir_stride, int ndirs) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t s = (uint32_t)ndirs * C[i];
    for (int r = 0; r < ndirs; r++) s += L[r * dir_stride + i];
    S[i] = s;
}

// =============================================================================================
// WTA + sub-pixel + vz->disparity  (calc_cost_sgm.cpp:259-308, :414-426), shared tail.
// c_1, c, c1 are S[best-1], S[best], S[best+1] (u32 in the reference).
// =============================================================================================
__device__ __forceinline__ uint32_t sum_at(const uint8_t* Lf, size_t dir_stride, int ndirs, size_t idx) {
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) s += r < ndirs ? (uint32_t)Lf[r * dir_stride + idx] : 0u;   // loads issued together
    return s;
}
// exact path arithmetic: the volumes hold y_r = L_r - C and the costs' share of S = ndirs * C + their sum (<= 8 * 510 = 4080) is
// added where S is read: nothing when !EX (Cf is null then and never read)
#define FSGM_WTA_C_SHARE(idx) (EX ? (uint32_t)a.ndirs * Cf[idx] : 0u)

// packed WTA: LPP lanes per pixel, DPL d per lane (16, or 12 / 20 / 28 for D = 48 .. 224); sums kept as 2 x u16 (8 paths x 255 < 65536)
// RU: also the runner-up cost a.minC2 = min { S[d] : |d - best| >= 2 } (all ones where no such d exists)
// EX: the volumes hold y_r = L_r - C and the lane's bytes of C are one more volume, counted ndirs times: S <= 8 * 510 = 4080 still
// fits the packed u16 sums, the LDS row and the key (S << 8 | d < 2^20); wta_finish takes u32 and has no narrower intermediate
template <int LPP, int DPL, bool RU = false, bool EX = false>
__device__ __forceinline__ void wta_packed_body(const WtaArgs& a, const WtaCostArgs x = WtaCostArgs{nullptr, 0}) {
    constexpr int D = LPP * DPL, NK = DPL / 4;
    constexpr int PPB = 256 / LPP;                           // pixels per block
    constexpr uint32_t MASK = 0x00FF00FFu;
    static_assert(DPL % 4 == 0 && D <= 256, "the key holds d in 8 bits");
    __shared__ uint32_t sS[256 * DPL / 2];                   // u16 S[PPB][D]
    const int tid = threadIdx.x;
    const int NP = a.W * a.H;
    const int gp = blockIdx.x * PPB + tid / LPP, j = tid % LPP;
    const bool valid = gp < NP;
    const int p = valid ? gp : NP - 1;
    const size_t f = blockIdx.y;
    const uint8_t* __restrict__ Lf = a.L + f * a.l_frame_stride;
    const uint8_t* __restrict__ Cf = EX ? x.C + f * x.c_frame_stride : nullptr;
    uint32_t E[NK], O[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) E[k] = O[k] = 0;
    const size_t off = (size_t)p * D + (size_t)j * DPL;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        if (r < a.ndirs) {
            uint32_t w[NK];
            if constexpr (NK == 4) {
                const uint4 v = FSGM_LINE_NT ? load_nt(Lf + (size_t)r * a.l_dir_stride + off) : *(const uint4*)(Lf + (size_t)r * a.l_dir_stride + off);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else load_nt_words<NK>(Lf + (size_t)r * a.l_dir_stride + off, w);     // the lane's DPL bytes, no more
#pragma unroll
            for (int k = 0; k < NK; k++) { E[k] += w[k] & MASK; O[k] += (w[k] >> 8) & MASK; }
        }
    }
    if constexpr (EX) {                                      // ndirs * C: 8 * 255 a half, no carry between the halves
        uint32_t w[NK];
        if constexpr (NK == 4) {
            const uint4 v = *(const uint4*)(Cf + off);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < NK; k++) w[k] = *(const uint32_t*)(Cf + off + 4 * k);      // 4-byte aligned only (D = 48 .. 224)
        }
        const uint32_t n = (uint32_t)a.ndirs;
#pragma unroll
        for (int k = 0; k < NK; k++) { E[k] += n * (w[k] & MASK); O[k] += n * ((w[k] >> 8) & MASK); }
    }
    // S to LDS in natural d order; key = (S << 8) | d, minimum key = first minimum (:267)
    uint32_t key = 0xFFFFFFFFu;
    uint32_t* row = sS + (size_t)(tid / LPP) * (D / 2) + j * (DPL / 2);
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const uint32_t s0 = E[k] & 0xFFFF, s1 = O[k] & 0xFFFF, s2 = E[k] >> 16, s3 = O[k] >> 16;
        row[2 * k] = s0 | (s1 << 16);
        row[2 * k + 1] = s2 | (s3 << 16);
        const uint32_t d0 = (uint32_t)j * DPL + 4 * k;
        key = min(key, min(min((s0 << 8) | d0, (s1 << 8) | (d0 + 1)), min((s2 << 8) | (d0 + 2), (s3 << 8) | (d0 + 3))));
    }
    key = group_min_u32<LPP>(key);
    if constexpr (RU) {
        // group_min_u32 is a butterfly: every lane of the pixel holds the winning key.  Each lane masks its own DPL sums, still
        // in E[] / O[]: (d - best + 1) as u32 is 0, 1 or 2 exactly for the three d of the exclusion window, which may reach into
        // the neighbouring lane's first or last d -- every lane tests against best itself, so nothing is exchanged.
        const uint32_t lo = (key & 0xFF) - 1u;               // d - lo > 2  <=>  |d - best| >= 2 (wraps past 2 below the window)
        uint32_t m2 = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const uint32_t d0 = (uint32_t)j * DPL + 4 * k;
            const uint32_t s0 = E[k] & 0xFFFF, s1 = O[k] & 0xFFFF, s2 = E[k] >> 16, s3 = O[k] >> 16;
            m2 = min(m2, d0 - lo > 2u ? s0 : 0xFFFFFFFFu);
            m2 = min(m2, d0 + 1 - lo > 2u ? s1 : 0xFFFFFFFFu);
            m2 = min(m2, d0 + 2 - lo > 2u ? s2 : 0xFFFFFFFFu);
            m2 = min(m2, d0 + 3 - lo > 2u ? s3 : 0xFFFFFFFFu);
        }
        m2 = group_min_u32<LPP>(m2);
        if (j == 0 && valid) a.minC2[f * (size_t)NP + p] = m2;
    }
    __syncthreads();
    if (j == 0 && valid) {
        const uint32_t best = key & 0xFF, minc = key >> 8;
        const uint16_t* srow = (const uint16_t*)(sS + (size_t)(tid / LPP) * (D / 2));
        uint32_t c_1 = 0, c1 = 0;
        if (a.subpixel && best > 1) {
            c_1 = srow[best - 1];
            if (best + 1 < (uint32_t)D) c1 = srow[best + 1];
            else if (p + 1 < NP) c1 = sum_at(Lf, a.l_dir_stride, a.ndirs, (size_t)(p + 1) * D) + FSGM_WTA_C_SHARE((size_t)(p + 1) * D);   // next pixel's d=0 (:296)
            else c1 = 0;                                      // past the end of Sp: defined as 0 here
        }
        wta_finish(a, f, p, best, minc, c_1, c1);
    }
}
template <int LPP>
__global__ __launch_bounds__(256) void wta_packed_kernel(WtaArgs a) { wta_packed_body<LPP, 16>(a); }
template <int LPP, int DPL>
__global__ __launch_bounds__(256) void wta_split_kernel(WtaArgs a) { wta_packed_body<LPP, DPL>(a); }
// the same with the runner-up cost: kernels of their own, so that the ones above stay what they were
template <int LPP>
__global__ __launch_bounds__(256) void wta_packed_ru_kernel(WtaArgs a) { wta_packed_body<LPP, 16, true>(a); }
template <int LPP, int DPL>
__global__ __launch_bounds__(256) void wta_split_ru_kernel(WtaArgs a) { wta_packed_body<LPP, DPL, true>(a); }
// and over an exact plan's volumes
template <int LPP>
__global__ __launch_bounds__(256) void wta_packed_exact_kernel(WtaArgs a, WtaCostArgs x) { wta_packed_body<LPP, 16, false, true>(a, x); }
template <int LPP, int DPL>
__global__ __launch_bounds__(256) void wta_split_exact_kernel(WtaArgs a, WtaCostArgs x) { wta_packed_body<LPP, DPL, false, true>(a, x); }

// generic WTA: one wave per pixel, lanes stride over d
template <bool RU>
__device__ __forceinline__ void wta_generic_body(const WtaArgs& a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NP = a.W * a.H, D = a.D;
    const int p = blockIdx.x * 4 + wave;
    if (p >= NP) return;
    const size_t f = blockIdx.y;
    const uint8_t* __restrict__ Lf = a.L + f * a.l_frame_stride;
    uint32_t key = 0xFFFFFFFFu;
    for (int d = lane; d < D; d += 64) {
        const uint32_t s = sum_at(Lf, a.l_dir_stride, a.ndirs, (size_t)p * D + d);
        key = min(key, (s << 12) | (uint32_t)d);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, s));
    if constexpr (RU) {                                      // second strided pass, the window around best (known to every lane) masked
        const int best = (int)(key & 0xFFF);
        uint32_t m2 = 0xFFFFFFFFu;
        for (int d = lane; d < D; d += 64)
            if (d < best - 1 || d > best + 1) m2 = min(m2, sum_at(Lf, a.l_dir_stride, a.ndirs, (size_t)p * D + d));
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) m2 = min(m2, (uint32_t)__shfl_xor((int)m2, s));
        if (lane == 0) a.minC2[f * (size_t)NP + p] = m2;
    }
    if (lane == 0) {
        const uint32_t best = key & 0xFFF, minc = key >> 12;
        uint32_t c_1 = 0, c1 = 0;
        if (a.subpixel && best > 1) {
            c_1 = sum_at(Lf, a.l_dir_stride, a.ndirs, (size_t)p * D + best - 1);
            if ((size_t)p * D + best + 1 < (size_t)NP * D) c1 = sum_at(Lf, a.l_dir_stride, a.ndirs, (size_t)p * D + best + 1);
        }
        wta_finish(a, f, p, best, minc, c_1, c1);
    }
}
__global__ __launch_bounds__(256) void wta_generic_kernel(WtaArgs a) { wta_generic_body<false>(a); }
__global__ __launch_bounds__(256) void wta_generic_ru_kernel(WtaArgs a) { wta_generic_body<true>(a); }
#undef FSGM_WTA_C_SHARE
// the generic WTA over an exact plan's volumes, a short body of its own beside the two-pass one above (no runner-up here).
// S = ndirs * C + the sum of the y_r <= 4080 < 2^12: the key still holds it
__global__ __launch_bounds__(256) void wta_generic_exact_kernel(WtaArgs a, WtaCostArgs x) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NP = a.W * a.H, D = a.D;
    const int p = blockIdx.x * 4 + wave;
    if (p >= NP) return;
    const size_t f = blockIdx.y;
    const uint8_t* __restrict__ Lf = a.L + f * a.l_frame_stride;
    const uint8_t* __restrict__ Cf = x.C + f * x.c_frame_stride;
    auto s_at = [&](size_t idx) -> uint32_t { return sum_at(Lf, a.l_dir_stride, a.ndirs, idx) + (uint32_t)a.ndirs * Cf[idx]; };
    uint32_t key = 0xFFFFFFFFu;
    for (int d = lane; d < D; d += 64) key = min(key, (s_at((size_t)p * D + d) << 12) | (uint32_t)d);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, s));
    if (lane == 0) {
        const uint32_t best = key & 0xFFF, minc = key >> 12;
        uint32_t c_1 = 0, c1 = 0;
        if (a.subpixel && best > 1) {
            c_1 = s_at((size_t)p * D + best - 1);
            if ((size_t)p * D + best + 1 < (size_t)NP * D) c1 = s_at((size_t)p * D + best + 1);
        }
        wta_finish(a, f, p, best, minc, c_1, c1);
    }
}

// =============================================================================================
// launchers
// =============================================================================================
// one class: the same grid for the plain kernel and for the one that also writes the runner-up cost
template <int LPP, int DPL>
static void launch_wta_class(hipStream_t st, const WtaArgs& a, int frames, const WtaCostArgs& x) {
    const int NP = a.W * a.H;
    dim3 grid((NP + 256 / LPP - 1) / (256 / LPP), frames);
    if (x.C) {                                                   // an exact plan's volumes
        if constexpr (DPL == 16) hipLaunchKernelGGL(wta_packed_exact_kernel<LPP>, grid, dim3(256), 0, st, a, x);
        else hipLaunchKernelGGL((wta_split_exact_kernel<LPP, DPL>), grid, dim3(256), 0, st, a, x);
        return;
    }
    if constexpr (DPL == 16) hipLaunchKernelGGL((a.minC2 ? wta_packed_ru_kernel<LPP> : wta_packed_kernel<LPP>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((a.minC2 ? wta_split_ru_kernel<LPP, DPL> : wta_split_kernel<LPP, DPL>), grid, dim3(256), 0, st, a);
}

void launch_wta(hipStream_t st, const WtaArgs& a, int frames, bool packed, WtaCostArgs x) {
    if (!packed) {
        dim3 grid((a.W * a.H + 3) / 4, frames);
        if (x.C) hipLaunchKernelGGL(wta_generic_exact_kernel, grid, dim3(256), 0, st, a, x);
        else if (a.minC2) hipLaunchKernelGGL(wta_generic_ru_kernel, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(wta_generic_kernel, grid, dim3(256), 0, st, a);
        return;
    }
    switch (a.D) {
#define FSGM_X(D, LPP, DPL) case D: launch_wta_class<LPP, DPL>(st, a, frames, x); break;
        FSGM_LINE_CLASSES(FSGM_X)
#undef FSGM_X
        default: break;                                      // (the callers ask agg_line_split)
    }
}

void launch_sum_paths(hipStream_t st, const uint8_t* L, uint32_t* S, size_t n, size_t dir_stride, int ndirs) {
    hipLaunchKernelGGL(sum_paths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, L, S, n, dir_stride, ndirs);
}

void launch_sum_paths_exact(hipStream_t st, const uint8_t* L, const uint8_t* C, uint32_t* S, size_t n, size_t dir_stride, int ndirs) {
    hipLaunchKernelGGL(sum_paths_exact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, L, C, S, n, dir_stride, ndirs);
}

}  // namespace fsgm
