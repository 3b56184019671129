// sgm2d_ingest.hip -- the kernels of sgm2d_ingest.h: n caller volumes in HBM -> a fsgm_pyd_plan's C (padded candidate rows),
// saturated at the declared bound.
#include "sgm2d_ingest.h"
#include "capi_common.h"
#include "pyd_kernels.h"
#include "pyd_plan.h"
#include <algorithm>

namespace fsgm {

// ---- [n][H][W][Sx*Sy] -> [n][H][W][Sx][RS], RS a multiple of 4 above Sy (the rows layout with padding; without padding the
// two layouts are one and launch_sgm_ingest's straight copy runs).  One thread a destination dword: dword q of row sx of a
// pixel takes source bytes sx*Sy + 4q .. + 3 of that pixel, those at or beyond Sy are padding and written 0.  The source
// promises no alignment (a row starts at any byte), so the up to 4 bytes are byte loads; neighbouring lanes read
// neighbouring bytes and store neighbouring dwords.  No LDS: the flag is one ballot and at the most one store a wave.
template <bool SAT>
__global__ __launch_bounds__(256) void ingest2d_hwd_pad_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t dwords,
                                                               int Sy, int RQ, int PQ, int D, size_t srcN, size_t dstN, uint32_t c,
                                                               uint32_t* __restrict__ flag) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    uint32_t over = 0;
    if (g < dwords) {
        const size_t px = g / (unsigned)PQ;
        const int r = (int)(g - px * (unsigned)PQ), sx = r / RQ, q = r - sx * RQ;
        const uint8_t* s = src + f * srcN + px * (size_t)D + (size_t)sx * Sy + 4 * q;
        const int nb = min(4, Sy - 4 * q);                       // >= 1: RQ = ceil(Sy / 4)
        uint32_t v = 0;
        for (int e = 0; e < nb; e++) v |= (uint32_t)s[e] << (8 * e);
        if (SAT) v = saturate4(v, c, &over);                     // (padding bytes are 0: never above a bound >= 1)
        *reinterpret_cast<uint32_t*>(dst + f * dstN + 4 * g) = v;
    }
    if (SAT && flag && __builtin_amdgcn_ballot_w64(over != 0) != 0 && (threadIdx.x & 63) == 0) *flag = 1u;
}

// ---- [n][channels][H][W] -> [n][H][W][PS]: one workgroup per (tile of INGEST_TX pixels x INGEST_TD bytes of the padded
// candidate index p = sx*RS + sy, image row, frame); channel sx*Sy + sy, or sy*Sx + sx with YX.  The tile is ingest_dhw_kernel's
// (sgm_ingest.hip), indexed by p instead of by the channel, so that the transposed tile is what a pixel holds from p0 on.
// In: 4 bytes along x a lane, 16 lanes = 64 contiguous bytes of one channel's image row, the tile into LDS as [p][x], rows
// 17 dwords apart; a row whose p is padding (sy >= Sy) or beyond PS is stored as zeros, which is how the padding bytes of
// the destination get their 0.  Out: a lane takes a 4 x 4 block (4 values of p x 4 pixels) as four ds_read_b32, transposes it
// in registers and stores 4 bytes along p for each of its 4 pixels: 16 lanes = the tile's 64 contiguous bytes of a pixel.
// LDS banks ((a / 4) % 32 for ds_write_b32 and ds_read_b32, lanes conflict within a half wave): the stores of a half wave
// cover two tile rows of 16 dwords, 17 apart -- banks 0..15 and 17..31, 0: one bank is hit twice; the loads of a half wave are
// 8 block rows (68 dwords apart: 4 mod 32) by 4 block columns (1 apart): 32 different banks.
// Alignment: in the rows layout RS, so PS and every p0 + 4 dq, is a multiple of 4 and every store is a whole aligned dword;
// in the unpadded layout (a side above 11, PS = Sx*Sy) an odd PS or the tile's tail takes the byte path.
template <bool YX>
__global__ __launch_bounds__(256) void ingest2d_chw_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H, int Sx,
                                                           int Sy, int RS, int PS, int txn, int tpn, uint32_t c, int sat,
                                                           uint32_t* __restrict__ flag) {
    constexpr int PW = INGEST_PITCH / 4;
    __shared__ uint32_t tile[INGEST_TD * PW + 1];                // (the last word: some lane met a byte above the bound)
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
        const int xq = t & 15, pr = t >> 4, x = x0 + 4 * xq;
        const uint8_t* s = src + f * srcN + (size_t)y * W + x;
        uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = p0 + pr + 16 * k, sx = p / RS, sy = p - sx * RS;
            if (p < PS && sy < Sy && x < W) {
                const uint8_t* q = s + (size_t)(YX ? sy * Sx + sx : sx * Sy + sy) * HW;
                if (x + 4 <= W) __builtin_memcpy(&r[k], q, 4);
                else
                    for (int j = 0; j < W - x; j++) r[k] |= (uint32_t)q[j] << (8 * j);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (sat) r[k] = saturate4(r[k], c, &over);
            tile[(pr + 16 * k) * PW + xq] = r[k];
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
    if (sat && flag) {
        __syncthreads();
        if (t == 0 && any_over != 0) *flag = 1u;
    }
}

size_t sgm2d_ingest_lds_bytes(int layout) {
    return layout == FSGM_COST2D_LAYOUT_HWD ? 0 : (size_t)INGEST_TD * INGEST_PITCH + 4;
}

void launch_sgm2d_ingest(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int W, int H, int Sx, int Sy, int layout, int bound,
                         uint32_t* flag) {
    const int D = Sx * Sy, RS = pyd_row_stride(Sx, Sy), PS = Sx * RS;
    if (layout == FSGM_COST2D_LAYOUT_HWD && PS == D) {           // the plan's layout is the caller's: the 1-D matcher's copy
        launch_sgm_ingest(st, src, dst, n, W, H, D, FSGM_COST_LAYOUT_HWD, bound, flag);
        return;
    }
    const bool sat = bound < 255;
    const uint32_t c = (uint32_t)(sat ? bound + 1 : 255) * 0x01010101u;
    const size_t HW = (size_t)W * H, srcN = HW * D, dstN = HW * PS;
    for (int f0 = 0; f0 < n; f0 += 65535) {                      // (the grid's y extent)
        const int nf = std::min(65535, n - f0);
        const uint8_t* s = src + (size_t)f0 * srcN;
        uint8_t* d = dst + (size_t)f0 * dstN;
        if (layout == FSGM_COST2D_LAYOUT_HWD) {
            // (W*H*D < 2^31 and PS <= 4 D: a frame has fewer than 2^31 dwords, the grid's x extent stays below 2^23)
            const size_t dwords = dstN / 4;
            const dim3 grid((unsigned)((dwords + 255) / 256), (unsigned)nf);
            if (sat) hipLaunchKernelGGL(ingest2d_hwd_pad_kernel<true>, grid, dim3(256), 0, st, s, d, dwords, Sy, RS / 4, PS / 4, D, srcN, dstN, c, flag);
            else     hipLaunchKernelGGL(ingest2d_hwd_pad_kernel<false>, grid, dim3(256), 0, st, s, d, dwords, Sy, RS / 4, PS / 4, D, srcN, dstN, c, flag);
            continue;
        }
        const int txn = (W + INGEST_TX - 1) / INGEST_TX, tpn = (PS + INGEST_TD - 1) / INGEST_TD;
        const dim3 grid((unsigned)((size_t)txn * tpn * H), (unsigned)nf);
        if (layout == FSGM_COST2D_LAYOUT_DHW_YX)
            hipLaunchKernelGGL(ingest2d_chw_kernel<true>, grid, dim3(256), 0, st, s, d, W, H, Sx, Sy, RS, PS, txn, tpn, c, sat ? 1 : 0, flag);
        else
            hipLaunchKernelGGL(ingest2d_chw_kernel<false>, grid, dim3(256), 0, st, s, d, W, H, Sx, Sy, RS, PS, txn, tpn, c, sat ? 1 : 0, flag);
    }
}

}  // namespace fsgm

extern "C" fsgm_status fsgm_sgm2d_ingest_lds(int32_t layout, int32_t halfX, int32_t halfY, uint64_t* bytes) {
    FSGM_REQUIRE(bytes, "fsgm_sgm2d_ingest_lds: null argument");
    FSGM_REQUIRE(layout == FSGM_COST2D_LAYOUT_HWD || layout == FSGM_COST2D_LAYOUT_DHW || layout == FSGM_COST2D_LAYOUT_DHW_YX,
                 "fsgm_sgm2d_ingest_lds: layout must be FSGM_COST2D_LAYOUT_HWD (0), _DHW (1) or _DHW_YX (2), got %d", layout);
    fsgm_status st = fsgm::pyd_check_sides(halfX, halfY, 0);
    if (st == FSGM_OK) st = fsgm::pyd_check_count(halfX, halfY);
    if (st != FSGM_OK) return st;
    *bytes = fsgm::sgm2d_ingest_lds_bytes(layout);
    return FSGM_OK;
}
