// sgm_ingest.hip -- the kernels of sgm_ingest.h: n caller volumes in HBM -> a plan's C, saturated at the declared bound.
#include "sgm_ingest.h"
#include "capi_common.h"
#include <algorithm>

namespace fsgm {

// ---- [n][H][W][D] -> the same layout: one wave a workgroup, 4 KiB a wave as four rounds of 16 bytes a lane, the destination
// aligned, the source wherever the caller has it (global memory takes a 16-byte load at any byte address; the load is written
// as a copy so that no alignment is promised).  One wave: the flag needs no LDS.
constexpr int HWD_ROUNDS = 4, HWD_BLOCK_BYTES = HWD_ROUNDS * 64 * 16;
template <bool SAT>
__global__ __launch_bounds__(64) void ingest_hwd_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t total,
                                                        uint32_t c, uint32_t* __restrict__ flag) {
    const size_t i0 = (size_t)blockIdx.x * HWD_BLOCK_BYTES + threadIdx.x * 16;
    uint32_t over = 0;
    if ((size_t)(blockIdx.x + 1) * HWD_BLOCK_BYTES <= total) {
        uint4 v[HWD_ROUNDS];
#pragma unroll
        for (int k = 0; k < HWD_ROUNDS; k++) __builtin_memcpy(&v[k], src + i0 + k * 1024, 16);
#pragma unroll
        for (int k = 0; k < HWD_ROUNDS; k++) {
            if (SAT) {
                v[k].x = saturate4(v[k].x, c, &over); v[k].y = saturate4(v[k].y, c, &over);
                v[k].z = saturate4(v[k].z, c, &over); v[k].w = saturate4(v[k].w, c, &over);
            }
            *reinterpret_cast<uint4*>(dst + i0 + k * 1024) = v[k];
        }
    } else {                                                     // the last workgroup: byte by byte
        for (int k = 0; k < HWD_ROUNDS; k++)
            for (size_t j = i0 + k * 1024; j < i0 + k * 1024 + 16 && j < total; j++) {
                uint32_t b = src[j];
                if (SAT) b = saturate4(b, c, &over) & 0xFFu;     // (the upper bytes are 0: never above a bound >= 1)
                dst[j] = (uint8_t)b;
            }
    }
    if (SAT && flag && __builtin_amdgcn_ballot_w64(over != 0) != 0 && threadIdx.x == 0) *flag = 1u;
}

// ---- [n][D][H][W] -> [n][H][W][D]: one workgroup per (tile of INGEST_TX pixels x INGEST_TD candidates, image row, frame).
// In: 4 bytes along x a lane, 16 lanes = 64 contiguous bytes per candidate row, the tile into LDS as it lies ([d][x], rows
// 17 dwords apart).  Out: a lane takes a 4 x 4 block (4 candidates x 4 pixels) as four ds_read_b32, transposes it in
// registers and stores 4 bytes along d for each of its 4 pixels: 16 lanes = the tile's 64 contiguous bytes of a pixel.
// LDS banks ((a / 4) % 32 for both accesses, 32 lanes a group): the stores of a group cover two rows of 16 dwords, 17 apart
// -- one bank is hit twice, which a store does not pay for; the loads of a group are 8 block rows (68 dwords apart: 4 mod 32)
// by 4 block columns (1 apart): 32 banks, no conflict.
__global__ __launch_bounds__(256) void ingest_dhw_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H, int D,
                                                         int txn, int tdn, uint32_t c, int sat, uint32_t* __restrict__ flag) {
    constexpr int PW = INGEST_PITCH / 4;
    __shared__ uint32_t tile[INGEST_TD * PW + 1];                // (the last word: some lane met a byte above the bound)
    uint32_t& any_over = tile[INGEST_TD * PW];
    const int t = threadIdx.x;
    unsigned b = blockIdx.x;
    const int x0 = (int)(b % (unsigned)txn) * INGEST_TX; b /= (unsigned)txn;
    const int d0 = (int)(b % (unsigned)tdn) * INGEST_TD;
    const int y = (int)(b / (unsigned)tdn);
    const size_t HW = (size_t)H * W, N = HW * D, f = blockIdx.y;
    uint32_t over = 0;
    if (t == 0) any_over = 0;
    {
        const int xq = t & 15, dr = t >> 4, x = x0 + 4 * xq;
        const uint8_t* s = src + f * N + (size_t)y * W + x;
        uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int d = d0 + dr + 16 * k;
            if (d < D && x < W) {
                const uint8_t* q = s + (size_t)d * HW;
                if (x + 4 <= W) __builtin_memcpy(&r[k], q, 4);
                else
                    for (int j = 0; j < W - x; j++) r[k] |= (uint32_t)q[j] << (8 * j);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (sat) r[k] = saturate4(r[k], c, &over);
            tile[(dr + 16 * k) * PW + xq] = r[k];
        }
    }
    __syncthreads();
    if (over != 0) any_over = 1u;
    {
        const int l = t & 31, half = (t >> 5) & 1, w = t >> 6;
        const int dq = half * 8 + (l & 7), xq = w * 4 + (l >> 3);
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = tile[(4 * dq + k) * PW + xq];
        transpose4x4(v);
        const int d = d0 + 4 * dq;
        const bool whole = (D & 3) == 0 && d + 4 <= D;           // then every address below is a multiple of 4
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = x0 + 4 * xq + j;
            if (x < W && d < D) {
                uint8_t* o = dst + f * N + ((size_t)y * W + x) * D + d;
                if (whole) *reinterpret_cast<uint32_t*>(o) = v[j];
                else
                    for (int e = 0; e < D - d && e < 4; e++) o[e] = (uint8_t)(v[j] >> (8 * e));
            }
        }
    }
    if (sat && flag) {
        __syncthreads();
        if (t == 0 && any_over != 0) *flag = 1u;
    }
}

size_t sgm_ingest_lds_bytes(int layout) {
    return layout == FSGM_COST_LAYOUT_DHW ? (size_t)INGEST_TD * INGEST_PITCH + 4 : 0;
}

void launch_sgm_ingest(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int W, int H, int D, int layout, int bound,
                       uint32_t* flag) {
    const bool sat = bound < 255;
    const uint32_t c = (uint32_t)(sat ? bound + 1 : 255) * 0x01010101u;
    const size_t N = (size_t)W * H * D;
    if (layout == FSGM_COST_LAYOUT_HWD) {
        // (launches of 2^34 bytes at the most: the grid's x extent stays below 2^31 whatever n is)
        const size_t total = (size_t)n * N, step = (size_t)1 << 34;
        for (size_t o = 0; o < total; o += step) {
            const size_t bytes = std::min(step, total - o);
            const dim3 grid((unsigned)((bytes + HWD_BLOCK_BYTES - 1) / HWD_BLOCK_BYTES));
            if (sat) hipLaunchKernelGGL(ingest_hwd_kernel<true>, grid, dim3(64), 0, st, src + o, dst + o, bytes, c, flag);
            else     hipLaunchKernelGGL(ingest_hwd_kernel<false>, grid, dim3(64), 0, st, src + o, dst + o, bytes, c, flag);
        }
        return;
    }
    const int txn = (W + INGEST_TX - 1) / INGEST_TX, tdn = (D + INGEST_TD - 1) / INGEST_TD;
    for (int f0 = 0; f0 < n; f0 += 65535) {                      // (the grid's y extent)
        const int nf = std::min(65535, n - f0);
        hipLaunchKernelGGL(ingest_dhw_kernel, dim3((unsigned)((size_t)txn * tdn * H), (unsigned)nf), dim3(256), 0, st,
                           src + (size_t)f0 * N, dst + (size_t)f0 * N, W, H, D, txn, tdn, c, sat ? 1 : 0, flag);
    }
}

}  // namespace fsgm

extern "C" fsgm_status fsgm_sgm_ingest_lds(int32_t layout, int32_t dMax, uint64_t* bytes) {
    FSGM_REQUIRE(bytes, "fsgm_sgm_ingest_lds: null argument");
    FSGM_REQUIRE(layout == FSGM_COST_LAYOUT_HWD || layout == FSGM_COST_LAYOUT_DHW,
                 "fsgm_sgm_ingest_lds: layout must be FSGM_COST_LAYOUT_HWD (0) or FSGM_COST_LAYOUT_DHW (1), got %d", layout);
    FSGM_REQUIRE(dMax >= 1 && dMax <= 1024, "fsgm_sgm_ingest_lds: dMax must be 1..1024 (got %d)", dMax);
    *bytes = fsgm::sgm_ingest_lds_bytes(layout);
    return FSGM_OK;
}
