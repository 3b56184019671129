// epi_view2.hip -- the second view's winner-take-all over the diagonal of S (include/fsgm.h, "Second view"): for second-view pixel
// (x2, y) the first minimum over i of S[y][x2 - dir * (d_min + i)][i], read from the path volumes the line kernels' WTA has just
// read.  A tiled kernel for D <= 256 (the sums of a tile's diagonals in LDS as u16), a generic one up to 1024 (one wave a pixel),
// and the left-right check on two disparity maps.  No kernel of another file is involved.
#include "epi_view2.h"
#include "fsgm_device.h"

namespace fsgm {

// Second-view pixels per workgroup of the tiled kernel: T * D u16 sums are at most 32 KB, and a tile reads T + D - 1 first-view
// columns for T outputs, so a small D takes a wide tile
int view2_tile(int D) { return D > 256 ? 0 : D > 128 ? 64 : D > 64 ? 128 : 256; }
size_t view2_lds_bytes(int D) {
    const int T = view2_tile(D);
    return T ? (size_t)T * D * 2 + 256 * sizeof(uint32_t) : 0;   // sS[D][T] u16, one partial key a thread
}

// sub-pixel offset: wta_finish's parabola (epi_wta_tail.h), the same f64 operations in the same order.  best is a first minimum,
// so c_1 > c >= 0 and c1 >= c: the divisor is c - c_1 < 0 when c1 < c_1 and c - c1 < 0 otherwise (then c1 >= c_1 > c) -- never zero
__device__ __forceinline__ uint32_t view2_value(const View2Args& a, uint32_t best, uint32_t c, bool sub_ok, uint32_t c_1, uint32_t c1) {
    uint32_t v = best * 256u;
    if (sub_ok) {
        const double dc_1 = (double)c_1, dc = (double)c, dc1 = (double)c1;
        double sub = (double)best;
        if (dc1 < dc_1) sub = __dadd_rn(sub, __ddiv_rn(__ddiv_rn(__dsub_rn(dc1, dc_1), __dsub_rn(dc, dc_1)), 2.0));
        else            sub = __dadd_rn(sub, __ddiv_rn(__ddiv_rn(__dsub_rn(dc1, dc_1), __dsub_rn(dc, dc1)), 2.0));
        v = f64_to_u32_x86(__dmul_rn(sub, 256.0));
    }
    return v + a.add;
}
// candidate i of second-view pixel x2 is first-view pixel x2 - dir * (d_min + i): in the image?
__device__ __forceinline__ bool view2_in(const View2Args& a, int x2, int i) {
    const int x = x2 - a.dir * (a.d_min + i);
    return x >= 0 && x < a.W;
}

// Tiled kernel: a workgroup owns T consecutive second-view pixels of one row of one frame.  The first-view columns that hold
// their candidates, [xlo, xhi], are one contiguous range of (xhi - xlo + 1) * D bytes in every path volume: the lanes walk it
// VB bytes each (coalesced), sum the paths (and ndirs * C of an exact plan, S <= 4080) and scatter each voxel's sum to
// sS[i][x2 - x0] when its second-view pixel lies in the tile.  Then T pixels scan their D candidates in NQ = 256 / T interleaved
// parts (lanes read consecutive u16) under the key (S << 8) | i, whose minimum is the first minimum.
// VB = 4 wants D % 4 == 0 (every address is then a whole dword), VB = 1 takes any D.
template <int VB>
__global__ __launch_bounds__(256) void view2_tiled_kernel(View2Args a, int T, int tiles) {
    extern __shared__ uint32_t view2_smem[];
    uint16_t* sS = (uint16_t*)view2_smem;
    const int tid = threadIdx.x, D = a.D, W = a.W, s = a.dir, dm = a.d_min;
    uint32_t* sK = view2_smem + (size_t)T * D / 2;
    const int tile = blockIdx.x % tiles, y = blockIdx.x / tiles, x0 = tile * T;
    const size_t f = blockIdx.y;
    const uint8_t* __restrict__ Lf = a.L + f * a.l_frame_stride;
    const uint8_t* __restrict__ Cf = a.C ? a.C + f * a.c_frame_stride : nullptr;
    const long long lo = s < 0 ? (long long)x0 + dm : (long long)x0 - dm - (D - 1);
    const long long hi = s < 0 ? (long long)x0 + T - 1 + dm + D - 1 : (long long)x0 + T - 1 - dm;
    const int xlo = (int)(lo < 0 ? 0 : lo), xhi = (int)(hi > W - 1 ? W - 1 : hi);
    const int nbytes = lo > W - 1 || hi < 0 ? 0 : (xhi - xlo + 1) * D;
    const size_t base = ((size_t)y * W + xlo) * D;
    for (int k = tid * VB; k < nbytes; k += 256 * VB) {
        uint32_t S[VB];
        if constexpr (VB == 4) {
            constexpr uint32_t MASK = 0x00FF00FFu;
            uint32_t E = 0, O = 0;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                if (r < a.ndirs) {
                    const uint32_t w = *(const uint32_t*)(Lf + (size_t)r * a.l_dir_stride + base + k);
                    E += w & MASK; O += (w >> 8) & MASK;
                }
            }
            if (Cf) {
                const uint32_t w = *(const uint32_t*)(Cf + base + k), n = (uint32_t)a.ndirs;
                E += n * (w & MASK); O += n * ((w >> 8) & MASK);         // 8 * 255 + 8 * 255 a half: no carry
            }
            S[0] = E & 0xFFFF; S[1] = O & 0xFFFF; S[2] = E >> 16; S[3] = O >> 16;
        } else {
            uint32_t v = Cf ? (uint32_t)a.ndirs * Cf[base + k] : 0u;
#pragma unroll
            for (int r = 0; r < 8; r++) v += r < a.ndirs ? (uint32_t)Lf[(size_t)r * a.l_dir_stride + base + k] : 0u;
            S[0] = v;
        }
        const int c = k / D, i0 = k - c * D;                         // (VB divides D: the lane's bytes share a column)
        const int t0 = xlo + c + s * (dm + i0) - x0;
#pragma unroll
        for (int j = 0; j < VB; j++) {
            const int t = t0 + s * j;
            if (t >= 0 && t < T) sS[(size_t)(i0 + j) * T + t] = (uint16_t)S[j];
        }
    }
    __syncthreads();
    const int NQ = 256 / T, t = tid & (T - 1), q = tid / T, x2 = x0 + t;
    uint32_t key = 0xFFFFFFFFu;
    if (x2 < W)
        for (int i = q; i < D; i += NQ)
            if (view2_in(a, x2, i)) key = min(key, ((uint32_t)sS[(size_t)i * T + t] << 8) | (uint32_t)i);
    sK[tid] = key;
    __syncthreads();
    if (q != 0 || x2 >= W) return;
    for (int g = 1; g < NQ; g++) key = min(key, sK[g * T + t]);
    const size_t o = f * ((size_t)W * a.H) + (size_t)y * W + x2;
    if (key == 0xFFFFFFFFu) {                                        // no candidate in the image (a valid key is below 2^20)
        a.disp2[o] = a.marker;
        if (a.minC2v) a.minC2v[o] = 0xFFFFFFFFu;
        return;
    }
    const int best = (int)(key & 0xFF);
    const bool sub_ok = a.subpixel && best >= 1 && best + 1 < D && view2_in(a, x2, best - 1) && view2_in(a, x2, best + 1);
    uint32_t c_1 = 0, c1 = 0;
    if (sub_ok) { c_1 = sS[(size_t)(best - 1) * T + t]; c1 = sS[(size_t)(best + 1) * T + t]; }
    a.disp2[o] = view2_value(a, (uint32_t)best, key >> 8, sub_ok, c_1, c1);
    if (a.minC2v) a.minC2v[o] = key >> 8;
}

// Generic kernel (256 < D <= 1024, untuned like the other generic kernels): one wave a second-view pixel, lanes stride over i,
// key (S << 12) | i as wta_generic_kernel's
__global__ __launch_bounds__(256) void view2_generic_kernel(View2Args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t NP = (size_t)a.W * a.H;
    const size_t p = (size_t)blockIdx.x * 4 + wave;
    if (p >= NP) return;
    const int y = (int)(p / a.W), x2 = (int)(p - (size_t)y * a.W), D = a.D;
    const size_t f = blockIdx.y;
    const uint8_t* __restrict__ Lf = a.L + f * a.l_frame_stride;
    const uint8_t* __restrict__ Cf = a.C ? a.C + f * a.c_frame_stride : nullptr;
    auto s_at = [&](int i) -> uint32_t {                             // i is a candidate of x2: the voxel lies in the volume
        const size_t idx = ((size_t)y * a.W + (size_t)(x2 - a.dir * (a.d_min + i))) * D + i;
        uint32_t v = Cf ? (uint32_t)a.ndirs * Cf[idx] : 0u;
#pragma unroll
        for (int r = 0; r < 8; r++) v += r < a.ndirs ? (uint32_t)Lf[(size_t)r * a.l_dir_stride + idx] : 0u;
        return v;
    };
    uint32_t key = 0xFFFFFFFFu;
    for (int i = lane; i < D; i += 64)
        if (view2_in(a, x2, i)) key = min(key, (s_at(i) << 12) | (uint32_t)i);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, m));
    if (lane != 0) return;
    const size_t o = f * NP + p;
    if (key == 0xFFFFFFFFu) {
        a.disp2[o] = a.marker;
        if (a.minC2v) a.minC2v[o] = 0xFFFFFFFFu;
        return;
    }
    const int best = (int)(key & 0xFFF);
    const bool sub_ok = a.subpixel && best >= 1 && best + 1 < D && view2_in(a, x2, best - 1) && view2_in(a, x2, best + 1);
    uint32_t c_1 = 0, c1 = 0;
    if (sub_ok) { c_1 = s_at(best - 1); c1 = s_at(best + 1); }
    a.disp2[o] = view2_value(a, (uint32_t)best, key >> 12, sub_ok, c_1, c1);
    if (a.minC2v) a.minC2v[o] = key >> 12;
}

// the left-right check, one thread a pixel
__global__ __launch_bounds__(256) void view2_check_kernel(View2CheckArgs a) {
    const size_t NP = (size_t)a.W * a.H;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const size_t f = blockIdx.y;
    const size_t row = p / a.W;
    const long long x = (long long)(p - row * a.W);
    const long long d1 = (((long long)(int32_t)a.disp[f * NP + p] - a.pre1) << a.shift1) + a.add1;
    const long long x2 = x + a.dir * ((d1 + 128) >> 8);              // arithmetic shift, no clamp
    uint8_t ok = 0;
    if (x2 >= 0 && x2 < a.W) {
        const uint32_t r2 = a.disp2[f * NP + row * a.W + (size_t)x2];
        const long long d2 = (long long)(int32_t)r2 + a.add2;
        const long long diff = d1 > d2 ? d1 - d2 : d2 - d1;
        ok = r2 != a.marker2 && diff <= (long long)a.max_diff;
    }
    a.conf[f * NP + p] = ok;
}

void launch_view2(hipStream_t st, const View2Args& a, int frames) {
    const int T = view2_tile(a.D);
    if (T == 0) {
        const size_t NP = (size_t)a.W * a.H;
        hipLaunchKernelGGL(view2_generic_kernel, dim3((unsigned)((NP + 3) / 4), frames), dim3(256), 0, st, a);
        return;
    }
    const int tiles = (a.W + T - 1) / T;
    const dim3 grid((unsigned)((size_t)tiles * a.H), frames);
    const size_t lds = view2_lds_bytes(a.D);
    const bool words = a.D % 4 == 0 && ((uintptr_t)a.L | (uintptr_t)a.C | a.l_frame_stride | a.l_dir_stride | a.c_frame_stride) % 4 == 0;
    if (words) hipLaunchKernelGGL(view2_tiled_kernel<4>, grid, dim3(256), lds, st, a, T, tiles);
    else       hipLaunchKernelGGL(view2_tiled_kernel<1>, grid, dim3(256), lds, st, a, T, tiles);
}

void launch_view2_check(hipStream_t st, const View2CheckArgs& a, int frames) {
    const size_t NP = (size_t)a.W * a.H;
    hipLaunchKernelGGL(view2_check_kernel, dim3((unsigned)((NP + 255) / 256), frames), dim3(256), 0, st, a);
}

}  // namespace fsgm
