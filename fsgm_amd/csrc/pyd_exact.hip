// pyd_exact.hip -- gfx950 kernels of the 2-D matcher with EXACT path arithmetic (include/fsgm.h, fsgm_pyd_plan_set_exact):
// the recurrence of calc_pyd_cost_sgm.cpp:34-89 (sgm_step), :114-296 (sgm2d) with every narrowing to unsigned char taken out.
//
//   path start (:182 etc.)  L[c] = C[c], stored minimum m = 0
//   step                    L[c] = C[c] + min(Lp[ctr], min over the 5x5 around ctr except ctr of Lp + P1, m_p + P2) - m_p,
//                           ctr the hint-shifted centre (:46-47), cells outside the window absent, m = min_c L[c] (the true one)
//
// With 0 <= P1, P2 <= 255 (the entry points refuse anything else):
//   L <= 255 + P2 <= 510              the minimum never exceeds the jump term m_p + P2, and C <= 255
//   L + P1, m_p + P2 <= 765           both below the absent marker of the LDS grid
//   y = L - C = min(...) - m_p        in [0, P2]: every real cell is >= m_p and the jump term is m_p + P2; after a path start
//                                     the stored minimum is 0 and y = min(...) <= 0 + P2 as well
// so a path writes y, one byte, into the path volumes the plain kernels fill with L (same size, same layout), and the WTA reads
// C as one more volume and rebuilds S = sum_r w_r * (C + y_r) <= 8 * 510 = 4080.
// Both kernels take either volume layout through RS / PS (pyd_kernels.h).
#include "pyd_kernels.h"
#include "fsgm_device.h"

namespace fsgm {

constexpr uint32_t PYD_EXACT_ABSENT = 0x7F00;                // pyd_agg_kernel's marker
constexpr uint32_t PYD_EXACT_LMAX = 255 + 255;               // L <= max C + max P2
static_assert(PYD_EXACT_LMAX + 255 < PYD_EXACT_ABSENT, "a real cell + P1 and the jump term stay below an absent cell");
static_assert(8 * PYD_EXACT_LMAX == 4080, "S of 8 paths");

// =============================================================================================
// 2-D path aggregation, exact.  pyd_agg_kernel<false, .>'s structure (pyd_kernels.hip): one wave per path line, the previous
// pixel's path costs in LDS as a padded grid of u32 cells with an absent ring, the separable hint shift tabulated once per
// step, the next step's costs / hint delta / adaptive-P2 decision fetched while the current one computes.  The grid holds
// the full L (up to 510); HBM gets y = L - C.  Including the centre cell in the "+P1" minimum is harmless (P1 >= 0 and the
// centre itself is a term), and an absent cell is a number above every real term, the jump term among them.
// =============================================================================================
template <int NCMAX>                                       // NCMAX >= ceil(Sx*Sy / 64) candidates per lane
__global__ __launch_bounds__(256) void pyd_agg_exact_kernel(PydAggArgs a) {
    extern __shared__ uint32_t sDynPydX[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (i < a.ndirs && (int)blockIdx.x >= a.blk_begin[i]) slot = i;
    const int code = a.dir_code[slot];
    const int base = code & 3;
    const bool mirror = (code & 4) != 0;
    const int W = a.W, H = a.H, Sx = a.Sx, Sy = a.Sy, D = Sx * Sy;
    const int GY = Sy + 2 * PYD_PADW, GN = (Sx + 2 * PYD_PADW) * GY;     // padded grid
    const int NP = W * H;
    const int nlines = base == 0 ? H : W;
    const int len = base == 0 ? W : H;
    const int line = ((int)blockIdx.x - a.blk_begin[slot]) * 4 + wave;
    // per-wave LDS: two padded grids + the two shift tables (pyd_agg_lds)
    uint32_t* const wbase = sDynPydX + (size_t)wave * (2 * GN + 2 * PYD_MAXS);
    uint32_t* pre = wbase;
    uint32_t* cur = wbase + GN;
    int32_t* const xtab = (int32_t*)(wbase + 2 * GN);
    int32_t* const ytab = xtab + PYD_MAXS;
    if (line >= nlines) return;                              // wave-uniform
    for (int i = lane; i < 2 * GN; i += 64) wbase[i] = PYD_EXACT_ABSENT;
    const size_t f = blockIdx.y;
    const int RS = a.RS, PS = a.PS;
    const uint8_t* __restrict__ Cf = a.C + f * (size_t)NP * PS;
    const uint8_t* __restrict__ If = a.I1 + f * (size_t)NP;
    uint8_t* __restrict__ Yf = a.L + (f * a.ndirs + slot) * (size_t)NP * PS;
    const double* __restrict__ mvxp = a.mv + f * 2 * (size_t)a.mvW * a.mvH;
    const double* __restrict__ mvyp = mvxp + (size_t)a.mvW * a.mvH;
    // path direction in pass-0 coordinates; the predecessor of p is p - r
    const int rx = base == 1 ? 0 : (base == 3 ? -1 : 1), ry = base == 0 ? 0 : 1;
    auto cell = [&](int sx, int sy) { return (sx + PYD_PADW) * GY + sy + PYD_PADW; };

    int x = base == 0 ? 0 : line, y = base == 0 ? line : 0;
    auto actual = [&](int cx, int cy, int& ax, int& ay) { ax = mirror ? W - 1 - cx : cx; ay = mirror ? H - 1 - cy : cy; };
    auto is_start = [&](int t, int cx) { return (t == 0) || (base == 2 && cx == 0) || (base == 3 && cx == W - 1); };
    auto advance = [&](int& cx, int& cy) {
        if (base == 0) cx++;
        else {
            cy++;
            if (base == 2) { cx++; if (cx == W) cx = 0; }
            if (base == 3) { cx--; if (cx < 0) cx = W - 1; }
        }
    };
    struct Fetch { uint32_t c[NCMAX]; double dx, dy; uint32_t P2; };
    // branch-free: at a path start the predecessor may lie outside the image, its coordinates are clamped and the values unused
    auto fetch = [&](int cx, int cy, Fetch& o) {
        int ax, ay;
        actual(cx, cy, ax, ay);
        const size_t off = ((size_t)ay * W + ax) * PS;
#pragma unroll
        for (int i = 0; i < NCMAX; i++) {
            const int d = min(lane + 64 * i, D - 1);
            o.c[i] = Cf[off + (d / Sy) * RS + d % Sy];
        }
        const int px = clampi(mirror ? ax + rx : ax - rx, 0, W - 1), py = clampi(mirror ? ay + ry : ay - ry, 0, H - 1);
        o.dx = __dsub_rn(mvxp[(size_t)ay * a.mvW + ax], mvxp[(size_t)py * a.mvW + px]);   // :213 etc.
        o.dy = __dsub_rn(mvyp[(size_t)ay * a.mvW + ax], mvyp[(size_t)py * a.mvW + px]);
        const int dI = abs((int)If[(size_t)W * ay + ax] - (int)If[(size_t)W * py + px]);
        o.P2 = (uint32_t)((a.adaptive && dI > 50) ? a.P2 / 8 : a.P2);                // :91-95
    };

    Fetch nxt;
    fetch(x, y, nxt);
    int xn = x, yn = y;
    advance(xn, yn);
    const uint32_t P1 = (uint32_t)a.P1;
    uint32_t m = 0;
    for (int t = 0; t < len; t++) {
        const Fetch now = nxt;
        {                                                    // in flight while this step computes
            const bool last = t + 1 >= len;
            fetch(last ? x : xn, last ? y : yn, nxt);
        }
        const bool start = is_start(t, x);
        int ax, ay;
        actual(x, y, ax, ay);
        const size_t off = ((size_t)ay * W + ax) * PS;
        if (start) {
#pragma unroll
            for (int i = 0; i < NCMAX; i++) {
                const int d = lane + 64 * i;
                if (d < D) {
                    const int sx = d / Sy, sy = d - sx * Sy;
                    cur[cell(sx, sy)] = now.c[i];
                    Yf[off + sx * RS + sy] = 0;                                  // L = C
                }
            }
            m = 0;                                                               // :182 stored minimum 0
        } else {
            // shift tables: xpre(sx), ypre(sy), clamped so that every tap stays in the padded grid
            if (lane < Sx) xtab[lane] = clampi(f64_to_i32_x86(__dadd_rn(__dadd_rn((double)lane, now.dx), 0.5)), -3, Sx + 2);   // :47
            if (lane < Sy) ytab[lane] = clampi(f64_to_i32_x86(__dadd_rn(__dadd_rn((double)lane, now.dy), 0.5)), -3, Sy + 2);   // :46
            __builtin_amdgcn_wave_barrier();
            const uint32_t jump = m + now.P2;                                    // :50-53, <= 510 + 255
            uint32_t lo = PYD_EXACT_ABSENT;
#pragma unroll
            for (int i = 0; i < NCMAX; i++) {
                const int d = lane + 64 * i;
                if (d < D) {
                    const int sx = d / Sy, sy = d - sx * Sy;
                    const uint32_t* ctr = pre + cell(xtab[sx], ytab[sy]);
                    uint32_t nb = 0xFFFFu;
#pragma unroll
                    for (int mm = -2; mm <= 2; mm++)
#pragma unroll
                        for (int k = -2; k <= 2; k++) nb = min(nb, ctr[mm * GY + k]);
                    const uint32_t best = min(min(jump, ctr[0]), nb + P1);       // :56-79; >= m, <= m + P2
                    const uint32_t yv = best - m;                                // y = L - C in [0, P2]: one byte
                    const uint32_t v = now.c[i] + yv;                            // :83 without the narrowing
                    cur[cell(sx, sy)] = v;
                    Yf[off + sx * RS + sy] = (uint8_t)yv;
                    lo = min(lo, v);
                }
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, s));
            m = lo;                                                              // :88, the true minimum
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t* tmp = pre; pre = cur; cur = tmp;
        x = xn; y = yn;
        advance(xn, yn);
    }
}

// =============================================================================================
// WTA + y/x parabola  (calc_pyd_cost_sgm.cpp:298-364) on C and the y volumes.  pyd_wta_kernel's structure: one wave per pixel,
// RU / NK as there.
// =============================================================================================
__device__ __forceinline__ uint32_t pyd_exact_sum_at(const PydWtaArgs& a, uint32_t wsum, const uint8_t* Cf, const uint8_t* Yf, size_t vol,
                                                     size_t idx) {
    uint32_t v[8];
    const uint32_t c = Cf[idx];
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = r < a.ndirs ? (uint32_t)Yf[r * vol + idx] : 0u;   // all loads in flight together
    uint32_t s = wsum * c;
#pragma unroll
    for (int r = 0; r < 8; r++) s += a.weight[r] * v[r];
    return s;
}

template <bool RU, int NK>
__global__ __launch_bounds__(256) void pyd_wta_exact_kernel(PydWtaExactArgs xa) {
    const PydWtaArgs& a = xa.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NP = a.W * a.H, Sy = a.Sy, Sx = a.Sx, D = Sx * Sy;
    const int p = blockIdx.x * 4 + wave;
    if (p >= NP) return;
    const size_t f = blockIdx.y;
    const size_t vol = (size_t)NP * a.PS;
    const uint8_t* __restrict__ Yf = a.L + f * a.ndirs * vol;
    const uint8_t* __restrict__ Cf = xa.C + f * vol;
    uint32_t wsum = 0;                                       // S = sum_r w_r * (C + y_r)
#pragma unroll
    for (int r = 0; r < 8; r++) wsum += r < a.ndirs ? a.weight[r] : 0u;
    auto at = [&](uint32_t d) { return (size_t)p * a.PS + (d / Sy) * a.RS + d % Sy; };
    auto sum = [&](uint32_t d) { return pyd_exact_sum_at(a, wsum, Cf, Yf, vol, at(d)); };
    uint32_t lo = 0xFFFFFFFFu, idx = 0xFFFFFFFFu;
    [[maybe_unused]] uint32_t keep[NK > 0 ? NK : 1];
    if constexpr (NK > 0) {
#pragma unroll
        for (int i = 0; i < NK; i++) {
            const int d = lane + 64 * i;
            keep[i] = 0xFFFFFFFFu;                           // a lane without a candidate here: the identity
            if (d < D) {
                const uint32_t s = sum(d);
                if (a.S) a.S[(f * NP + p) * D + d] = s;
                if (s < lo) { lo = s; idx = d; }
                keep[i] = s;
            }
        }
    } else {
        for (int d = lane; d < D; d += 64) {
            const uint32_t s = sum(d);
            if (a.S) a.S[(f * NP + p) * D + d] = s;
            if (s < lo) { lo = s; idx = d; }                 // ascending d per lane: first minimum
        }
    }
    uint32_t glo = lo;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) glo = min(glo, (uint32_t)__shfl_xor((int)glo, s));
    uint32_t gidx = lo == glo ? idx : 0xFFFFFFFFu;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) gidx = min(gidx, (uint32_t)__shfl_xor((int)gidx, s));
    if constexpr (RU) {
        const int bx = (int)gidx / Sy, by = (int)gidx - bx * Sy;
        uint32_t c2 = 0xFFFFFFFFu;                           // FSGM_NO_RUNNER_UP: the identity of the minimum
        if constexpr (NK > 0) {
#pragma unroll
            for (int i = 0; i < NK; i++) {
                const int d = lane + 64 * i, sx = d / Sy, sy = d - sx * Sy;
                if (max(abs(sx - bx), abs(sy - by)) >= 2) c2 = min(c2, keep[i]);      // (d >= D: keep[i] is the identity)
            }
        } else {
            for (int d = lane; d < D; d += 64) {
                const int sx = d / Sy, sy = d - sx * Sy;
                if (max(abs(sx - bx), abs(sy - by)) >= 2) c2 = min(c2, sum(d));
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c2 = min(c2, (uint32_t)__shfl_xor((int)c2, s));
        if (lane == 0) a.minC2[f * NP + p] = c2;
    }
    if (lane == 0) {
        a.bestD[f * NP + p] = gidx;
        a.minC[f * NP + p] = glo;
        double subx = 0.0, suby = 0.0;
        if (a.subpixel) {
            const double c0 = (double)glo;
            const int dx = gidx / Sy, dy = gidx % Sy;                            // :333-334
            if (dy > 0 && dy < Sy - 1) suby = pyd_parabola((double)sum(gidx - 1), c0, (double)sum(gidx + 1));
            if (dx > 0 && dx < Sx - 1) subx = pyd_parabola((double)sum(gidx - Sy), c0, (double)sum(gidx + Sy));
        }
        a.mvSub[f * 2 * (size_t)NP + p] = subx;              // zero when subpixel is off (:476 zero-init output)
        a.mvSub[f * 2 * (size_t)NP + NP + p] = suby;
    }
}

// =============================================================================================
// launchers
// =============================================================================================
void launch_pyd_agg_exact(hipStream_t st, const PydAggArgs& a, int frames) {
    if (a.ndirs == 0) return;
    dim3 grid(a.blk_begin[8], frames);
    const size_t lds = pyd_agg_lds(a.Sx, a.Sy);
    const int nc = (a.Sx * a.Sy + 63) / 64;
    if (nc <= 2)      hipLaunchKernelGGL((pyd_agg_exact_kernel<2>), grid, dim3(256), lds, st, a);    // up to 11x11
    else if (nc <= 4) hipLaunchKernelGGL((pyd_agg_exact_kernel<4>), grid, dim3(256), lds, st, a);
    else              hipLaunchKernelGGL((pyd_agg_exact_kernel<16>), grid, dim3(256), lds, st, a);
}

void launch_pyd_wta_exact(hipStream_t st, const PydWtaArgs& w, const uint8_t* C, int frames) {
    PydWtaExactArgs a;
    a.w = w; a.C = C;
    dim3 grid((w.W * w.H + 3) / 4, frames);
    if (!w.minC2)                  hipLaunchKernelGGL((pyd_wta_exact_kernel<false, 0>), grid, dim3(256), 0, st, a);
    else if (w.Sx * w.Sy <= 256)   hipLaunchKernelGGL((pyd_wta_exact_kernel<true, 4>), grid, dim3(256), 0, st, a);
    else                           hipLaunchKernelGGL((pyd_wta_exact_kernel<true, 0>), grid, dim3(256), 0, st, a);
}

}  // namespace fsgm
