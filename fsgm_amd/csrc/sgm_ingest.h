// sgm_ingest.h -- caller-supplied cost volumes, already in HBM, into a plan's C (u8 [n][H][W][D], d fastest): a straight copy
// for volumes that arrive in that layout, a transposition through an LDS tile for [n][D][H][W] (a contiguous torch
// (N, D, H, W) tensor).  Both saturate every byte at the caller's declared bound on the way and raise a device flag when a
// byte was above it (include/fsgm.h, fsgm_sgm_device).  Kernels: sgm_ingest.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsgm {

// The transposing kernel's tile: INGEST_TX pixels along x by INGEST_TD candidates, one workgroup of 256 threads per tile and
// image row.  The tile lies in LDS as the source has it, [d][x], rows INGEST_PITCH bytes apart.
constexpr int INGEST_TX = 64, INGEST_TD = 64, INGEST_PITCH = INGEST_TX + 4;

// min(x, bound) on the four bytes of x, c = (bound + 1) in every byte (bound <= 254); *over |= the bytes that were above.
// Per byte, x >= c: where the top bits differ x's decides, where they agree the 7-bit difference (no borrow crosses a byte:
// every byte of x | hi is >= 0x80, every byte of c & ~hi <= 0x7f).
__host__ __device__ inline uint32_t saturate4(uint32_t x, uint32_t c, uint32_t* over) {
    const uint32_t hi = 0x80808080u;
    const uint32_t d = (x | hi) - (c & ~hi);
    const uint32_t ge = ((x & ~c) | (~(x ^ c) & d)) & hi;
    const uint32_t m = (ge >> 7) * 0xFFu;                        // 0xFF in every byte that is above the bound
    *over |= m;
    return (x & ~m) | ((c - 0x01010101u) & m);
}

// bytes [a0 a1 b0 b1] / [a2 a3 b2 b3] of a and b (byte 0 first): the two steps of a 4 x 4 byte transposition
__host__ __device__ inline uint32_t zip_lo(uint32_t a, uint32_t b, int step) {
#if defined(__HIP_DEVICE_COMPILE__)
    return step == 1 ? __builtin_amdgcn_perm(b, a, 0x05010400u) : __builtin_amdgcn_perm(b, a, 0x05040100u);
#else
    return step == 1 ? ((a & 0xFFu) | ((b & 0xFFu) << 8) | ((a & 0xFF00u) << 8) | ((b & 0xFF00u) << 16))
                     : ((a & 0xFFFFu) | (b << 16));
#endif
}
__host__ __device__ inline uint32_t zip_hi(uint32_t a, uint32_t b, int step) {
#if defined(__HIP_DEVICE_COMPILE__)
    return step == 1 ? __builtin_amdgcn_perm(b, a, 0x07030602u) : __builtin_amdgcn_perm(b, a, 0x07060302u);
#else
    return step == 1 ? (((a >> 16) & 0xFFu) | (((b >> 16) & 0xFFu) << 8) | ((a >> 24) << 16) | ((b >> 24) << 24))
                     : ((a >> 16) | (b & 0xFFFF0000u));
#endif
}
// r[k] holds bytes (k, 0..3) of a 4 x 4 block; afterwards r[j] holds bytes (0..3, j)
__host__ __device__ inline void transpose4x4(uint32_t r[4]) {
    const uint32_t a = zip_lo(r[0], r[1], 1), b = zip_hi(r[0], r[1], 1), c = zip_lo(r[2], r[3], 1), d = zip_hi(r[2], r[3], 1);
    r[0] = zip_lo(a, c, 2); r[1] = zip_hi(a, c, 2); r[2] = zip_lo(b, d, 2); r[3] = zip_hi(b, d, 2);
}

// n volumes from src (layout FSGM_COST_LAYOUT_HWD or _DHW, any byte alignment) into dst (u8 [n][H][W][D], 16-byte aligned),
// every byte min(byte, bound); *flag = 1 (flag may be NULL) when some byte was above the bound.  bound 1..255.
void launch_sgm_ingest(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int W, int H, int D, int layout, int bound,
                       uint32_t* flag);
// the LDS the launcher asks for (static, per workgroup)
size_t sgm_ingest_lds_bytes(int layout);

}  // namespace fsgm
